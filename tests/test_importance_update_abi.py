"""dd_importance_update without a GPU: the ctypes mirrors of its structs against a C compile of include/dd_hip.h, the exported symbol, the
build lists, and every host-side refusal (validation fails before any launch; the pointers are never dereferenced)."""
import ctypes
import os
import re
import subprocess

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_offsets_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dd_importance_update_pass), sizeof(dd_importance_update_desc),
  DD_IMPORTANCE_MAX_PASSES, offsetof(dd_importance_update_pass, pred), offsetof(dd_importance_update_pass, target),
  offsetof(dd_importance_update_pass, pred_ld), offsetof(dd_importance_update_pass, target_ld), offsetof(dd_importance_update_desc, n_planes),
  offsetof(dd_importance_update_desc, plane_hw), offsetof(dd_importance_update_desc, cell_base), offsetof(dd_importance_update_desc, epsilon),
  offsetof(dd_importance_update_desc, pass)); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P, D = _lib.ImportanceUpdatePass, _lib.ImportanceUpdateDesc
    assert have == [ctypes.sizeof(P), ctypes.sizeof(D), _lib.IMPORTANCE_MAX_PASSES, P.pred.offset, P.target.offset, P.pred_ld.offset,
                    P.target_ld.offset, D.n_planes.offset, D.plane_hw.offset, D.cell_base.offset, D.epsilon.offset, D.pass_.offset]
    assert ctypes.sizeof(P) == 24 and D.n_passes.offset == 0
    # the records are dd_sample_tiles' own: 64 bytes, the target plane at 4, the origin at 8 and 12, flip and rotate at 16 and 20
    from deepdenoiser_amd.frame_bank import RECORD_DTYPE
    assert RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.TileRecord) == 64
    assert [RECORD_DTYPE.fields[k][1] for k in ("target_plane", "y0", "x0", "flip", "rotate")] == [4, 8, 12, 16, 20]


def test_symbol_is_declared_built_and_exported(lib):
    assert "dd_importance_update" in _lib.SYMBOLS and hasattr(lib, "dd_importance_update")
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    assert re.search(r"\bint dd_importance_update\(const dd_importance_update_desc\* desc, const dd_tile_record\* records, int B, int T, int G,", header)
    from deepdenoiser_amd import build
    assert "dd_importance_update.hip" in build.SOURCES and build.NO_SCRATCH["dd_importance_update.hip"] == ("importance_update_kernel",)
    assert os.path.isfile(os.path.join(build.CSRC, "dd_importance_update.hip"))
    # the older kernel's file keeps its one kernel
    assert build.NO_SCRATCH["dd_frame_importance.hip"] == ("frame_importance_kernel",)


def _desc(n_passes=2):
    d = _lib.ImportanceUpdateDesc()
    d.n_passes, d.n_planes, d.plane_hw, d.cell_base, d.epsilon = n_passes, 3, 4096, 4352, 1e-2
    for k in range(min(max(n_passes, 0), _lib.IMPORTANCE_MAX_PASSES)):
        d.pass_[k].pred, d.pass_[k].target, d.pass_[k].pred_ld, d.pass_[k].target_ld = 8192 + 256 * k, 65536 + 256 * k, 3 + k, 3
    return d


def test_host_side_refusals(lib):
    records, sums, counts = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(1 << 22)

    def call(d, table=records, B=4, T=32, G=16, acc_sum=sums, acc_count=counts):
        return lib.dd_importance_update(ctypes.byref(d) if d is not None else None, table, B, T, G, 1, 1, acc_sum, acc_count, None)

    def refused(word, *a, **k):
        assert call(*a, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    # null pointers: the descriptor, the records, either accumulator, the size table, cell_base, a pass's prediction or target
    refused(b"null", None)
    refused(b"null", _desc(), table=None)
    refused(b"null", _desc(), acc_sum=None)
    refused(b"null", _desc(), acc_count=None)
    for field in ("plane_hw", "cell_base"):
        d = _desc()
        setattr(d, field, None)
        refused(b"null", d)
    for field in ("pred", "target"):
        d = _desc()
        setattr(d.pass_[1], field, None)
        refused(b"null", d)
    # n_passes outside 1 .. DD_IMPORTANCE_MAX_PASSES
    refused(b"n_passes=0", _desc(0))
    refused(b"n_passes=-1", _desc(-1))
    refused(b"n_passes=%d" % (_lib.IMPORTANCE_MAX_PASSES + 1), _desc(_lib.IMPORTANCE_MAX_PASSES + 1))
    # pred_ld or target_ld below 3
    d = _desc()
    d.pass_[0].pred_ld = 2
    refused(b"pred_ld=2", d)
    d = _desc()
    d.pass_[1].target_ld = 1
    refused(b"target_ld=1", d)
    # G outside 1 .. 64 or not a divisor of T
    for G in (0, -4, 65):
        refused(b"G=%d" % G, _desc(), G=G)
    refused(b"G=12", _desc(), G=12)
    refused(b"G=64", _desc(), G=64)                             # (in range, but 32 % 64 != 0)
    assert call(_desc(), T=0) < 0 and b"T=0" in lib.dd_last_error()
    # T < 1, B < 1, n_planes < 1
    refused(b"T=-32", _desc(), T=-32)
    refused(b"B=0", _desc(), B=0)
    refused(b"B=-1", _desc(), B=-1)
    d = _desc()
    d.n_planes = 0
    refused(b"n_planes=0", d)
    # epsilon <= 0 or not finite
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        d = _desc()
        d.epsilon = eps
        refused(b"epsilon", d)
