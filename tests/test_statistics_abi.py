"""dd_tile_statistics without a GPU: the ctypes mirrors of its structs and the row layout against a C compile of include/dd_hip.h, the
exported symbol, and every host-side refusal (validation fails before any launch; the pointers are never dereferenced)."""
import ctypes
import os
import re
import subprocess

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_offsets_and_row_layout_match_header(tmp_path):
    fields = ["DD_STAT_" + n.upper() for n in _lib.STAT_FIELD_NAMES]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %d %d %zu %zu %zu %zu %zu %zu\n", sizeof(dd_stat_window), sizeof(dd_stat_pass), sizeof(dd_stat_desc), DD_STAT_MAX_PASSES,
  DD_STAT_FIELDS, offsetof(dd_stat_window, mask_plane), offsetof(dd_stat_window, x0), offsetof(dd_stat_pass, mask_planes), offsetof(dd_stat_pass, C),
  offsetof(dd_stat_desc, plane_hw), offsetof(dd_stat_desc, pass));
  printf("''' + " ".join(["%d"] * len(fields)) + r'''\n", ''' + ", ".join(fields) + r'''); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    first, second = subprocess.check_output([exe]).decode().splitlines()
    W, P, D = _lib.StatWindow, _lib.StatPass, _lib.StatDesc
    assert [int(x) for x in first.split()] == [ctypes.sizeof(W), ctypes.sizeof(P), ctypes.sizeof(D), _lib.STAT_MAX_PASSES, _lib.STAT_FIELDS,
                                               W.mask_plane.offset, W.x0.offset, P.mask_planes.offset, P.C.offset, D.plane_hw.offset, D.pass_.offset]
    assert [int(x) for x in second.split()] == list(range(_lib.STAT_FIELDS))      # STAT_FIELD_NAMES is the enum's order
    assert ctypes.sizeof(W) == 16
    from deepdenoiser_amd.statistics import WINDOW_DTYPE
    assert [WINDOW_DTYPE.fields[k][1] for k in ("plane", "mask_plane", "y0", "x0")] == [W.plane.offset, W.mask_plane.offset, W.y0.offset, W.x0.offset]


def test_symbol_is_declared_built_and_exported(lib):
    assert "dd_tile_statistics" in _lib.SYMBOLS and hasattr(lib, "dd_tile_statistics")
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    assert re.search(r"\bint dd_tile_statistics\(const dd_stat_desc\*", header)
    from deepdenoiser_amd import build
    assert "dd_frame_statistics.hip" in build.SOURCES and build.NO_SCRATCH["dd_frame_statistics.hip"] == ("frame_statistics_kernel",)


def _desc(n_passes=3):
    d = _lib.StatDesc()
    d.n_passes, d.n_planes, d.plane_hw = n_passes, 3, 4096
    for k in range(min(n_passes, _lib.STAT_MAX_PASSES)):
        p = d.pass_[k]
        p.planes, p.mask_planes, p.C, p.is_alpha = 8192 + 256 * k, (65536 if k == 0 else None), (3 if k < 2 else 1), int(k == 2)
    return d


def test_host_side_refusals(lib):
    windows, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)

    def call(d, win=windows, n=4, T=16, dst=out):
        return lib.dd_tile_statistics(ctypes.byref(d) if d is not None else None, win, n, T, dst, None)

    def refused(word, *a, **k):
        assert call(*a, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    # null pointers: the descriptor, the window table, the output, the size table, a pass's plane array
    refused(b"null", None)
    refused(b"null", _desc(), win=None)
    refused(b"null", _desc(), dst=None)
    d = _desc()
    d.plane_hw = None
    refused(b"null", d)
    d = _desc()
    d.pass_[1].planes = None
    refused(b"null", d)
    # n_passes outside 1 .. DD_STAT_MAX_PASSES
    refused(b"n_passes=0", _desc(0))
    refused(b"n_passes=-1", _desc(-1))
    refused(b"n_passes=%d" % (_lib.STAT_MAX_PASSES + 1), _desc(_lib.STAT_MAX_PASSES + 1))
    # C not 1 or 3
    for C in (0, 2, 4):
        d = _desc()
        d.pass_[1].C = C
        refused(b"C=%d" % C, d)
    # a mask pass on a pass with C != 3
    d = _desc()
    d.pass_[2].mask_planes = 65536
    refused(b"mask", d)
    # T < 1, n_windows < 1
    refused(b"T=0", _desc(), T=0)
    refused(b"T=-3", _desc(), T=-3)
    refused(b"n_windows=0", _desc(), n=0)
    refused(b"n_windows=-2", _desc(), n=-2)
    d = _desc()
    d.n_planes = 0
    refused(b"n_planes=0", d)
