"""dd_exr_inflate without a GPU: the ctypes and numpy mirrors of its record against a C compile of include/dd_hip.h, the status constants, the
exported symbol, the build lists, and every host-side refusal (validation reads the HOST copy of the table and fails before any launch; the
device pointers are never dereferenced)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from deepdenoiser_amd import _lib, openexr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("OK", "HEADER", "TRUNCATED", "BLOCK_TYPE", "STORED", "LENGTHS", "SYMBOL", "DISTANCE", "OVERRUN", "SHORT", "CHECK", "RECORD")


def test_struct_and_status_constants_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu", sizeof(dd_exr_stream), offsetof(dd_exr_stream, src_offset), offsetof(dd_exr_stream, dst_offset),
  offsetof(dd_exr_stream, src_bytes), offsetof(dd_exr_stream, dst_bytes));
  printf(" %d %d %d %d %d %d %d %d %d %d %d %d\n", ''' + ", ".join("DD_INFLATE_" + n for n in NAMES) + r'''); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.ExrStream
    assert have[:5] == [ctypes.sizeof(S), S.src_offset.offset, S.dst_offset.offset, S.src_bytes.offset, S.dst_bytes.offset] == [24, 0, 8, 16, 20]
    assert have[5:] == [getattr(_lib, "INFLATE_" + n) for n in NAMES] == list(range(12))
    assert _lib.INFLATE_STATUS_NAMES == NAMES
    dtype = openexr.STREAM_DTYPE
    assert dtype.itemsize == ctypes.sizeof(S)
    assert [(name, dtype.fields[name][1]) for name in dtype.names] == [(name, getattr(S, name).offset) for name, _ in S._fields_]


def test_symbol_is_declared_built_and_exported(lib):
    assert "dd_exr_inflate" in _lib.SYMBOLS and hasattr(lib, "dd_exr_inflate")
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    assert re.search(r"\bint dd_exr_inflate\(const dd_exr_stream\* streams_host, const dd_exr_stream\* streams, int n_streams", header)
    comment = header[header.index("csrc/dd_exr_inflate.hip"):header.index("#define DD_INFLATE_OK")]
    assert "OpenEXRDirectory.py:125-151" in comment and "cv2.imdecode" in comment
    from deepdenoiser_amd import build
    assert "dd_exr_inflate.hip" in build.SOURCES and "dd_inflate_core.h" in build.HEADERS
    assert build.NO_SCRATCH["dd_exr_inflate.hip"] == ("exr_inflate_kernel",)
    assert build.NO_SCRATCH["dd_exr_decode.hip"] == ("exr_reconstruct_kernel",)          # (nothing was added to the sibling)
    for name in ("dd_exr_inflate.hip", "dd_inflate_core.h"):
        source = open(os.path.join(build.CSRC, name)).read()
        assert "asm" not in source.replace("assembly", "")                                # plain C++ only


def _table(n=2):
    streams = (_lib.ExrStream * n)()
    for k, s in enumerate(streams):
        s.src_offset, s.dst_offset, s.src_bytes, s.dst_bytes = 100 * k, 112 * k, 100, 100
    return streams


def test_host_side_refusals(lib):
    fake_table, src, staged, status = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4))

    def call(streams, n=2, table_dev=fake_table, source=src, src_total=200, buf=staged, staged_bytes=224, out=status):
        return lib.dd_exr_inflate(streams, table_dev, n, source, src_total, buf, staged_bytes, out, None)

    def refused(word, field=None, value=None, index=1, **k):
        streams = _table()
        if field:
            setattr(streams[index], field, value)
        assert call(streams, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    # no streams: a no-op, whatever else is passed
    assert lib.dd_exr_inflate(None, None, 0, None, 0, None, 0, None, None) == 0
    refused(b"n_streams=-1", n=-1)
    assert call(None) < 0 and b"null" in lib.dd_last_error()
    refused(b"null", table_dev=None)
    refused(b"null", source=None)
    refused(b"null", buf=None)
    refused(b"null", out=None)
    for n in (0, -5):
        refused(b"src_bytes=%d" % n, "src_bytes", n)
    for n in (0, -1, (1 << 30) + 1):
        refused(b"dst_bytes=%d" % n, "dst_bytes", n)
    refused(b"src_offset=101", "src_offset", 101)
    refused(b"src_offset=-1", "src_offset", -1)
    refused(b"source bytes", src_total=199)
    refused(b"dst_offset=-16", "dst_offset", -16)
    refused(b"dst_offset=120", "dst_offset", 120)
    refused(b"not 16-byte aligned", "dst_offset", 8, index=0)
    refused(b"staged bytes", staged_bytes=223)             # (100 bytes own 112)
    refused(b"dst_offset=128", "dst_offset", 128)
    # the numpy table of the decoder is read the same way
    table = np.zeros(1, dtype=openexr.STREAM_DTYPE)
    table[0] = (0, 0, 0, 16)
    assert lib.dd_exr_inflate(table.ctypes.data, fake_table, 1, src, 100, staged, 16, status, None) < 0
    assert b"src_bytes=0" in lib.dd_last_error()
