"""dd_importance_cells without a GPU: the ctypes mirrors of its structs against a C compile of include/dd_hip.h, the exported symbol, the build
lists, and every host-side refusal (validation fails before any launch; the pointers are never dereferenced)."""
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
int main(void){ printf("%zu %zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dd_importance_cell), sizeof(dd_importance_pass),
  sizeof(dd_importance_desc), DD_IMPORTANCE_MAX_PASSES, offsetof(dd_importance_cell, source_plane0), offsetof(dd_importance_cell, target_plane),
  offsetof(dd_importance_cell, y0), offsetof(dd_importance_cell, x0), offsetof(dd_importance_desc, n_planes), offsetof(dd_importance_desc, plane_hw),
  offsetof(dd_importance_desc, n_sources), offsetof(dd_importance_desc, epsilon), offsetof(dd_importance_desc, pass)); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    K, P, D = _lib.ImportanceCell, _lib.ImportancePass, _lib.ImportanceDesc
    assert have == [ctypes.sizeof(K), ctypes.sizeof(P), ctypes.sizeof(D), _lib.IMPORTANCE_MAX_PASSES, K.source_plane0.offset, K.target_plane.offset,
                    K.y0.offset, K.x0.offset, D.n_planes.offset, D.plane_hw.offset, D.n_sources.offset, D.epsilon.offset, D.pass_.offset]
    assert ctypes.sizeof(K) == 16 and _lib.IMPORTANCE_MAX_PASSES == 16
    from deepdenoiser_amd.frame_importance import CELL_DTYPE
    assert CELL_DTYPE.itemsize == 16
    assert [CELL_DTYPE.fields[k][1] for k in ("source_plane0", "target_plane", "y0", "x0")] == [K.source_plane0.offset, K.target_plane.offset,
                                                                                                K.y0.offset, K.x0.offset]


def test_symbol_is_declared_built_and_exported(lib):
    assert "dd_importance_cells" in _lib.SYMBOLS and hasattr(lib, "dd_importance_cells")
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    assert re.search(r"\bint dd_importance_cells\(const dd_importance_desc\*", header)
    from deepdenoiser_amd import build
    assert "dd_frame_importance.hip" in build.SOURCES and build.NO_SCRATCH["dd_frame_importance.hip"] == ("frame_importance_kernel",)


def _desc(n_passes=2):
    d = _lib.ImportanceDesc()
    d.n_passes, d.n_planes, d.plane_hw, d.n_sources, d.epsilon = n_passes, 3, 4096, 2, 1e-2
    for k in range(min(max(n_passes, 0), _lib.IMPORTANCE_MAX_PASSES)):
        d.pass_[k].planes = 8192 + 256 * k
    return d


def test_host_side_refusals(lib):
    cells, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def call(d, table=cells, n=4, G=16, dst=out):
        return lib.dd_importance_cells(ctypes.byref(d) if d is not None else None, table, n, G, dst, None)

    def refused(word, *a, **k):
        assert call(*a, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    # null pointers: the descriptor, the cell table, the output, the size table, a pass's plane array
    refused(b"null", None)
    refused(b"null", _desc(), table=None)
    refused(b"null", _desc(), dst=None)
    d = _desc()
    d.plane_hw = None
    refused(b"null", d)
    d = _desc()
    d.pass_[1].planes = None
    refused(b"null", d)
    # n_passes outside 1 .. DD_IMPORTANCE_MAX_PASSES
    refused(b"n_passes=0", _desc(0))
    refused(b"n_passes=-1", _desc(-1))
    refused(b"n_passes=%d" % (_lib.IMPORTANCE_MAX_PASSES + 1), _desc(_lib.IMPORTANCE_MAX_PASSES + 1))
    # n_planes < 1, n_sources < 1
    d = _desc()
    d.n_planes = 0
    refused(b"n_planes=0", d)
    for bad in (0, -2):
        d = _desc()
        d.n_sources = bad
        refused(b"n_sources=%d" % bad, d)
    # G outside 1 .. 64, n_cells < 1
    for G in (0, -4, 65):
        refused(b"G=%d" % G, _desc(), G=G)
    refused(b"n_cells=0", _desc(), n=0)
    refused(b"n_cells=-2", _desc(), n=-2)
    # epsilon <= 0 or not finite
    for eps in (0.0, -1e-2, float("inf"), float("nan")):
        d = _desc()
        d.epsilon = eps
        refused(b"epsilon", d)
