"""dd_sample_tiles without a GPU: the ctypes mirrors of its structs against a C compile of include/dd_hip.h, and every host-side refusal
(validation fails before any launch; the pointers are never dereferenced)."""
import ctypes
import os
import subprocess

import numpy as np

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_offsets_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %d %zu %zu %zu %zu %zu\n", sizeof(dd_tile_record), sizeof(dd_tile_pass), sizeof(dd_tile_sampler_desc), DD_TILE_MAX_PASSES,
  offsetof(dd_tile_record, draw), offsetof(dd_tile_pass, C), offsetof(dd_tile_pass, from_target), offsetof(dd_tile_sampler_desc, plane_hw),
  offsetof(dd_tile_sampler_desc, pass)); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    R, P, D = _lib.TileRecord, _lib.TilePass, _lib.TileSamplerDesc
    assert got == [ctypes.sizeof(R), ctypes.sizeof(P), ctypes.sizeof(D), _lib.TILE_MAX_PASSES, R.draw.offset, P.C.offset, P.from_target.offset,
                   D.plane_hw.offset, D.pass_.offset]
    from deepdenoiser_amd.frame_bank import RECORD_DTYPE
    assert RECORD_DTYPE.itemsize == ctypes.sizeof(R) == 64
    assert RECORD_DTYPE.fields["flip"][1] == R.draw.offset and RECORD_DTYPE.fields["normal_rotation"][1] == R.draw.offset + _lib.AugmentDraw.normal_rotation.offset
    assert np.dtype(RECORD_DTYPE).fields["x0"][1] == R.x0.offset


def _desc(n_passes=2):
    d = _lib.TileSamplerDesc()
    d.n_passes, d.n_planes, d.plane_hw = n_passes, 3, 4096
    for k in range(min(n_passes, _lib.TILE_MAX_PASSES)):
        p = d.pass_[k]
        p.planes, p.dst, p.C, p.kind, p.ld_dst, p.from_target = 8192 + 256 * k, 65536 + 4096 * k, 3, _lib.AUG_RGB, 3, k & 1
    return d


def test_host_side_refusals(lib):
    records = ctypes.c_void_p(1 << 20)

    def call(d, rec=records, B=2, T=16, flip=0, rotate=1, permute=1, normal=1):
        return lib.dd_sample_tiles(ctypes.byref(d) if d is not None else None, rec, B, T, flip, rotate, permute, normal, None)

    def refused(word, *a, **k):
        assert call(*a, **k) == -1
        assert word in lib.dd_last_error(), lib.dd_last_error()
    # null pointers: the descriptor, the records, the size table, a pass's plane array, a pass's destination
    refused(b"null", None)
    refused(b"null", _desc(), rec=None)
    d = _desc()
    d.plane_hw = None
    refused(b"null", d)
    for field in ("planes", "dst"):
        d = _desc()
        setattr(d.pass_[1], field, None)
        refused(b"null", d)
    # C not 1 or 3
    for C in (0, 2, 4):
        d = _desc()
        d.pass_[0].C, d.pass_[0].ld_dst, d.pass_[0].kind = C, 4, _lib.AUG_PLAIN
        refused(b"C=%d" % C, d)
    # a non-plain kind with C != 3, and a kind that does not exist
    for kind in (_lib.AUG_RGB, _lib.AUG_NORMAL, _lib.AUG_SCREEN_NORMAL):
        d = _desc()
        d.pass_[1].C, d.pass_[1].kind = 1, kind
        refused(b"needs 3 channels", d)
    for kind in (-1, 4):
        d = _desc()
        d.pass_[0].kind = kind
        refused(b"kind", d)
    # ld_dst < C
    d = _desc()
    d.pass_[0].ld_dst = 2
    refused(b"ld_dst", d)
    # flip together with a world-space normal pass, as dd_augment refuses it
    d = _desc()
    d.pass_[1].kind = _lib.AUG_NORMAL
    refused(b"normals", d, flip=1)
    # T < 1, B < 1
    refused(b"T=0", _desc(), T=0)
    refused(b"T=-3", _desc(), T=-3)
    refused(b"B=0", _desc(), B=0)
    # more passes than the descriptor holds, and none
    refused(b"n_passes=%d" % (_lib.TILE_MAX_PASSES + 1), _desc(_lib.TILE_MAX_PASSES + 1))
    refused(b"n_passes=0", _desc(0))
    d = _desc()
    d.n_planes = 0
    refused(b"n_planes=0", d)
