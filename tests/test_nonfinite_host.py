"""Host side of the NaN / Inf scan and repair (no GPU): the command-line options, the ctypes mirror of dd_nonfinite_desc, and the argument
checks of dd_nonfinite_scan / dd_nonfinite_repair, which return a status before any launch."""
import ctypes
import os
import subprocess

import pytest

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_parser_accepts_the_new_options_and_keeps_its_defaults():
    from deepdenoiser_amd import predict
    a = predict.parser().parse_args(["architecture.json", "--input", "frames"])
    assert a.nonfinite == "keep" and a.nonfinite_png is False
    assert (a.tile_size, a.tile_overlap_size, a.dtype, a.tiles_per_batch, a.exr, a.data_format) == (128, 14, "f16", 256, False, "channels_first")
    b = predict.parser().parse_args(["architecture.json", "--input", "frames", "--nonfinite", "repair", "--nonfinite_png"])
    assert b.nonfinite == "repair" and b.nonfinite_png is True
    assert predict.parser().parse_args(["architecture.json", "--nonfinite", "error"]).nonfinite == "error"
    with pytest.raises(SystemExit):
        predict.parser().parse_args(["architecture.json", "--nonfinite", "drop"])


def test_predictor_refuses_unknown_modes_before_it_touches_a_device():
    from deepdenoiser_amd.prediction import Predictor
    with pytest.raises(ValueError, match="nonfinite"):
        Predictor(None, nonfinite="drop")
    with pytest.raises(ValueError, match="radius"):
        Predictor(None, nonfinite="repair", nonfinite_radius=5)


def test_struct_size_matches_the_header(tmp_path):
    """the method of test_abi.py::test_struct_sizes_match_header on the new structs"""
    c = tmp_path / "t.c"
    c.write_text('#include <stdio.h>\n#include "dd_hip.h"\n'
                 'int main(void){ printf("%zu %zu %d\\n", sizeof(dd_nonfinite_plane), sizeof(dd_nonfinite_desc), DD_NONFINITE_MAX_PLANES); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    plane, desc, planes = (int(x) for x in subprocess.check_output([exe]).split())
    assert (plane, desc, planes) == (ctypes.sizeof(_lib.NonfinitePlane), ctypes.sizeof(_lib.NonfiniteDesc), _lib.NONFINITE_MAX_PLANES)


def _desc(n_planes=1, C=3, ld=3):
    d = _lib.NonfiniteDesc()
    d.n_planes = n_planes
    for i in range(min(n_planes, _lib.NONFINITE_MAX_PLANES)):
        d.plane[i].data, d.plane[i].mask, d.plane[i].C, d.plane[i].ld = 64, 128, C, ld      # never dereferenced: validation fails first
    return d


def test_bad_arguments_return_a_status_and_set_the_error(lib):
    counts = ctypes.c_void_p(256)
    assert lib.dd_nonfinite_scan(None, 1, 8, 8, counts, None) == -1
    assert b"dd_nonfinite_scan" in lib.dd_last_error() and b"null" in lib.dd_last_error()
    assert lib.dd_nonfinite_repair(None, 1, 8, 8, 2, counts, None) == -1
    assert b"dd_nonfinite_repair" in lib.dd_last_error() and b"null" in lib.dd_last_error()
    assert lib.dd_nonfinite_scan(ctypes.byref(_desc()), 1, 8, 8, None, None) == -1
    assert b"counts" in lib.dd_last_error()
    for bad, word in ((_desc(C=2, ld=3), b"channels"), (_desc(C=4, ld=4), b"channels"), (_desc(C=3, ld=2), b"ld"), (_desc(n_planes=33), b"planes"),
                      (_desc(n_planes=0), b"planes")):
        assert lib.dd_nonfinite_scan(ctypes.byref(bad), 1, 8, 8, counts, None) == -1
        assert word in lib.dd_last_error(), lib.dd_last_error()
        assert lib.dd_nonfinite_repair(ctypes.byref(bad), 1, 8, 8, 2, counts, None) == -1
    for radius in (0, 5, -1):
        assert lib.dd_nonfinite_repair(ctypes.byref(_desc()), 1, 8, 8, radius, counts, None) == -1
        assert b"radius" in lib.dd_last_error()
    assert lib.dd_nonfinite_scan(ctypes.byref(_desc()), 0, 8, 8, counts, None) == -1
    assert lib.dd_nonfinite_scan(ctypes.byref(_desc()), 4, 32768, 32768, counts, None) == -1      # 2^32 pixels
    assert b"32-bit" in lib.dd_last_error()
    d = _desc()
    d.plane[0].mask = None
    assert lib.dd_nonfinite_scan(ctypes.byref(d), 1, 8, 8, counts, None) == -1
