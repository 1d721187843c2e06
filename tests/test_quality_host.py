"""dd_frame_quality and the quality module without a GPU: refused arguments (no launch), the struct mirrors against a C compile of the
header, the exported names, the command-line switches, and the file matching of quality.targets_of_frame."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from deepdenoiser_amd import _lib, configs, openexr, quality
from deepdenoiser_amd.architecture import Architecture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(lib, pairs, n=None, H=16, W=16, thr=4096, records=8192, scratch=16384, maps=None):
    """(pointers are made-up addresses: every call here is refused before anything is dereferenced or launched)"""
    table = (_lib.QualityPair * max(len(pairs), 1))(*pairs)
    return lib.dd_frame_quality(table, len(pairs) if n is None else n, H, W, thr, 1.0, 1e-2, maps, records, scratch, None)


def test_refused_arguments(lib):
    ok = _lib.QualityPair(1 << 20, 2 << 20, 3, 3, 3)
    cases = (
        (lambda: _call(lib, [ok], n=0), b"n_pairs"),
        (lambda: _call(lib, [ok] * 33), b"n_pairs"),
        (lambda: _call(lib, [_lib.QualityPair(1 << 20, 2 << 20, 3, 3, 2)]), b"channels"),
        (lambda: _call(lib, [_lib.QualityPair(1 << 20, 2 << 20, 4, 4, 4)]), b"channels"),
        (lambda: _call(lib, [_lib.QualityPair(1 << 20, 2 << 20, 2, 3, 3)]), b"ld"),
        (lambda: _call(lib, [ok, _lib.QualityPair(1 << 20, 2 << 20, 1, 0, 1)]), b"ld"),
        (lambda: _call(lib, [ok], H=0), b"shape"),
        (lambda: _call(lib, [ok], W=-3), b"shape"),
        (lambda: _call(lib, [_lib.QualityPair(None, 2 << 20, 3, 3, 3)]), b"null pred / target"),
        (lambda: _call(lib, [ok, _lib.QualityPair(1 << 20, None, 3, 3, 3)]), b"null pred / target"),
        (lambda: _call(lib, [ok], thr=None), b"threshold"),
        (lambda: _call(lib, [ok], records=None), b"records"),
        (lambda: _call(lib, [ok], scratch=None), b"scratch"),
        (lambda: lib.dd_frame_quality(None, 1, 16, 16, 4096, 1.0, 1e-2, None, 8192, 16384, None), b"null pair table"),
    )
    for call, word in cases:
        assert call() < 0 and word in lib.dd_last_error(), lib.dd_last_error()
    assert lib.dd_frame_quality_scratch_bytes(0, 16, 16) < 0 and lib.dd_frame_quality_scratch_bytes(33, 16, 16) < 0
    assert lib.dd_frame_quality_scratch_bytes(1, 0, 16) < 0 and lib.dd_frame_quality_scratch_bytes(1, 16, 0) < 0
    T, rec = quality.TILE, ctypes.sizeof(_lib.QualityRecord)
    assert lib.dd_frame_quality_scratch_bytes(1, 1, 1) == rec
    assert lib.dd_frame_quality_scratch_bytes(3, T, T + 1) == 3 * 2 * rec
    assert lib.dd_frame_quality_scratch_bytes(25, 1080, 1920) == 25 * (-(-1080 // T)) * (-(-1920 // T)) * rec


def test_struct_sizes_and_constants_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(dd_quality_pair), sizeof(dd_quality_record), offsetof(dd_quality_record, se),
  offsetof(dd_quality_record, ssim_sum), offsetof(dd_quality_record, max_abs), DD_QUALITY_MAX_PAIRS, DD_QUALITY_TILE); return 0; }
'''
    c = tmp_path / "t.c"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "t")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "t")]).split()]
    R = _lib.QualityRecord
    assert got == [ctypes.sizeof(_lib.QualityPair), ctypes.sizeof(R), R.se.offset, R.ssim_sum.offset, R.max_abs.offset, _lib.QUALITY_MAX_PAIRS, _lib.QUALITY_TILE]
    assert ctypes.sizeof(R) == 72 and ctypes.sizeof(R) % 8 == 0


def test_new_names_are_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dd_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(dd_frame_quality[a-z0-9_]*)\s*\(", text)))
    assert names == ["dd_frame_quality", "dd_frame_quality_scratch_bytes"]
    for n in names:
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    from deepdenoiser_amd import build
    assert "dd_quality.hip" in build.SOURCES and set(build.NO_SCRATCH["dd_quality.hip"]) == {"frame_quality_kernel", "frame_quality_finalize_kernel"}


def test_command_lines_accept_the_new_switches():
    from deepdenoiser_amd import compare, predict
    a = predict.parser().parse_args(["a.json", "--input", "in", "--target", "gt", "--exposure", "2.5", "--quality_json", "q.json", "--ssim_png"])
    assert (a.target, a.exposure, a.quality_json, a.ssim_png) == ("gt", 2.5, "q.json", True)
    a = predict.parser().parse_args(["a.json", "--input", "in"])
    assert (a.target, a.exposure, a.quality_json, a.ssim_png) == (None, 1.0, None, False)
    c = compare.parser().parse_args(["a.exr", "b.npy", "--exposure", "0.5"])
    assert (c.image, c.reference, c.exposure) == ("a.exr", "b.npy", 0.5)
    assert compare.parser().parse_args(["a", "b"]).exposure == 1.0


def test_compare_loads_exr_and_npy(tmp_path):
    from deepdenoiser_amd import compare
    img = np.random.default_rng(0).random((5, 7, 3)).astype(np.float32)
    openexr.write_image(str(tmp_path / "a.exr"), img)
    np.save(tmp_path / "b.npy", img[..., 0])
    assert np.array_equal(compare.load_image(str(tmp_path / "a.exr")), img)
    assert compare.load_image(str(tmp_path / "b.npy")).shape == (5, 7, 1)


def _write_targets(directory, arch, skip=()):
    rng = np.random.default_rng(1)
    for f in quality.target_passes(arch):
        if f.name not in skip:
            openexr.write_image(os.path.join(directory, "gt_%s_0001.exr" % f.name), rng.random((6, 9, 3)).astype(np.float32))


def test_targets_of_frame_matches_files_by_pass_name(tmp_path):
    """(on the host: recombine=False stops in front of the device part, the dd_recombine launch that tests/test_gpu_quality.py covers)"""
    arch = Architecture(configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE"), device="cpu")
    passes = quality.target_passes(arch)
    assert passes and all(f.is_target and f.load_data for f in passes)
    names = quality.target_names(arch)
    assert names[:len(passes)] == ["prediction/" + f.name for f in passes]
    assert names[len(passes):] == ["prediction/Diffuse", "prediction/Glossy", "prediction/Subsurface", "prediction/Transmission", "Combined"]
    d = tmp_path / "gt"
    d.mkdir()
    _write_targets(str(d), arch)
    openexr.write_image(str(d / "gt_Normal_0001.exr"), np.zeros((6, 9, 3), dtype=np.float32))      # an auxiliary pass: not a target, not read
    got = quality.targets_of_frame(str(d), arch, device="cpu", recombine=False)
    assert list(got) == names[:len(passes)]
    for f in passes:
        t = got["prediction/" + f.name]
        assert tuple(t.shape) == (6, 9, f.number_of_channels) and t.stride(1) == 3
        assert np.array_equal(t.numpy(), openexr.read_image(str(d / ("gt_%s_0001.exr" % f.name)))[..., :f.number_of_channels])
    # 'Diffuse Color' is not taken for 'Diffuse Direct' and the like: every file was matched to its own pass
    assert not np.array_equal(got["prediction/Diffuse Color"].numpy(), got["prediction/Diffuse Direct"].numpy())
    # a missing pass is an error that names it
    os.remove(d / "gt_Glossy Direct_0001.exr")
    with pytest.raises(openexr.ExrError, match="Glossy Direct"):
        quality.targets_of_frame(str(d), arch, device="cpu", recombine=False)
    # without every member of the recombination there is no combined feature and no 'Combined'
    combined = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Glossy"}
    small = Architecture(configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", combined=combined), device="cpu")
    small_names = quality.target_names(small)
    assert "Combined" not in small_names and not [n for n in small_names if n in ("prediction/Diffuse", "prediction/Glossy")]
    assert list(quality.targets_of_frame(str(d), small, device="cpu", recombine=False)) == small_names
