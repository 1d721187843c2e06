"""dd_exr_pack and dd_exr_deflate without a GPU: the ctypes and numpy mirrors of their records against a C compile of include/dd_hip.h, the
status constants, the exported symbols, the build lists, and every host-side refusal (validation reads the HOST copy of the tables and fails
before any launch; the device pointers are never dereferenced)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from deepdenoiser_amd import _lib, openexr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structs_and_status_constants_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu", sizeof(dd_exr_deflate_stream), offsetof(dd_exr_deflate_stream, src_offset), offsetof(dd_exr_deflate_stream, dst_offset),
  offsetof(dd_exr_deflate_stream, src_bytes), offsetof(dd_exr_deflate_stream, dst_capacity));
  printf(" %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_exr_source), offsetof(dd_exr_source, src), offsetof(dd_exr_source, H), offsetof(dd_exr_source, W),
  offsetof(dd_exr_source, C), offsetof(dd_exr_source, n_channels), offsetof(dd_exr_source, type), offsetof(dd_exr_source, src_channel));
  printf(" %d %d %d %d\n", DD_DEFLATE_OK, DD_DEFLATE_RAW, DD_DEFLATE_RECORD, DD_EXR_MAX_CHANNELS); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S, F = _lib.ExrDeflateStream, _lib.ExrSource
    assert have[:5] == [ctypes.sizeof(S), S.src_offset.offset, S.dst_offset.offset, S.src_bytes.offset, S.dst_capacity.offset] == [24, 0, 8, 16, 20]
    assert have[5:13] == [ctypes.sizeof(F), F.src.offset, F.H.offset, F.W.offset, F.C.offset, F.n_channels.offset, F.type.offset,
                          F.src_channel.offset] == [88, 0, 8, 12, 16, 20, 24, 56]
    assert have[13:] == [_lib.DEFLATE_OK, _lib.DEFLATE_RAW, _lib.DEFLATE_RECORD, _lib.EXR_MAX_CHANNELS] == [0, 1, 2, 8]
    assert [openexr.DEFLATE_OK, openexr.DEFLATE_RAW, openexr.DEFLATE_RECORD] == [0, 1, 2]
    assert _lib.DEFLATE_STATUS_NAMES == ("OK", "RAW", "RECORD")
    for dtype, struct in ((openexr.DEFLATE_STREAM_DTYPE, S), (openexr.SOURCE_DTYPE, F)):
        assert dtype.itemsize == ctypes.sizeof(struct)
        assert [(name, dtype.fields[name][1]) for name in dtype.names] == [(name, getattr(struct, name).offset) for name, _ in struct._fields_]


def test_symbols_are_declared_built_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    for name in ("dd_exr_pack", "dd_exr_deflate", "dd_exr_deflate_workspace"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint dd_exr_pack\(const dd_exr_chunk\* chunks_host, const dd_exr_chunk\* chunks, int n_chunks, const dd_exr_source\* sources_host", header)
    assert re.search(r"\bint dd_exr_deflate\(const dd_exr_deflate_stream\* streams_host, const dd_exr_deflate_stream\* streams, int n_streams", header)
    for start, end in (("csrc/dd_exr_encode.hip", "} dd_exr_source;"), ("csrc/dd_exr_deflate.hip", "#define DD_DEFLATE_OK")):
        comment = header[header.index(start):header.index(end)]
        assert "Prediction.py:483-510" in comment and "write_exr" in comment
    from deepdenoiser_amd import build
    assert "dd_exr_encode.hip" in build.SOURCES and "dd_exr_deflate.hip" in build.SOURCES and "dd_deflate_core.h" in build.HEADERS
    assert build.NO_SCRATCH["dd_exr_encode.hip"] == ("exr_pack_kernel",)
    assert build.NO_SCRATCH["dd_exr_deflate.hip"] == ("exr_deflate_kernel",)
    assert build.NO_SCRATCH["dd_exr_inflate.hip"] == ("exr_inflate_kernel",)              # (nothing was added to the siblings)
    assert build.NO_SCRATCH["dd_exr_decode.hip"] == ("exr_reconstruct_kernel",)
    for name in ("dd_exr_encode.hip", "dd_exr_deflate.hip", "dd_deflate_core.h"):
        source = open(os.path.join(build.CSRC, name)).read()
        assert "asm" not in source.replace("assembly", "")                                # plain C++ only
    assert lib.dd_exr_deflate_workspace(3) == 3 * 4 * _lib.DEFLATE_BLOCK_TOKENS and lib.dd_exr_deflate_workspace(0) == 0
    core = open(os.path.join(build.CSRC, "dd_deflate_core.h")).read()
    assert re.search(r"#define DD_DEFLATE_BLOCK_TOKENS %d\b" % _lib.DEFLATE_BLOCK_TOKENS, core)


def test_deflate_host_side_refusals(lib):
    fake_table, src, out, work, status, sizes = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6))
    need = lib.dd_exr_deflate_workspace(2)

    def table():
        streams = (_lib.ExrDeflateStream * 2)()
        for k, s in enumerate(streams):
            s.src_offset, s.dst_offset, s.src_bytes, s.dst_capacity = 112 * k, 112 * k, 100, 99
        return streams

    def call(streams, n=2, table_dev=fake_table, source=src, src_total=224, buf=out, out_bytes=224, workspace=work, workspace_bytes=need, st=status, sz=sizes):
        return lib.dd_exr_deflate(streams, table_dev, n, source, src_total, buf, out_bytes, workspace, workspace_bytes, st, sz, None)

    def refused(word, field=None, value=None, index=1, **k):
        streams = table()
        if field:
            setattr(streams[index], field, value)
        assert call(streams, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    assert lib.dd_exr_deflate(None, None, 0, None, 0, None, 0, None, 0, None, None, None) == 0      # no streams: a no-op
    refused(b"n_streams=-1", n=-1)
    assert call(None) < 0 and b"null" in lib.dd_last_error()
    for name in ("table_dev", "source", "buf", "workspace", "st", "sz"):
        refused(b"null", **{name: None})
    refused(b"workspace_bytes", workspace_bytes=need - 1)
    refused(b"aligned", buf=ctypes.c_void_p((3 << 20) + 8))
    refused(b"aligned", workspace=ctypes.c_void_p((4 << 20) + 2))
    for n in (0, -5, (1 << 30) + 1):
        refused(b"src_bytes=%d" % n, "src_bytes", n)
    refused(b"dst_capacity=-1", "dst_capacity", -1)
    refused(b"src_offset=125", "src_offset", 125)
    refused(b"src_offset=-1", "src_offset", -1)
    refused(b"source bytes", src_total=211)
    refused(b"dst_offset=-16", "dst_offset", -16)
    refused(b"not 16-byte aligned", "dst_offset", 8, index=0)
    refused(b"output bytes", out_bytes=223)                 # (a capacity of 99 owns 112)
    refused(b"dst_offset=128", "dst_offset", 128)
    refused(b"overlap", buf=ctypes.c_void_p((2 << 20) + 16))
    # the numpy table of the encoder is read the same way
    record = np.zeros(1, dtype=openexr.DEFLATE_STREAM_DTYPE)
    record[0] = (0, 0, 0, 16)
    assert lib.dd_exr_deflate(record.ctypes.data, fake_table, 1, src, 100, out, 16, work, need, status, sizes, None) < 0
    assert b"src_bytes=0" in lib.dd_last_error()


def test_pack_host_side_refusals(lib):
    fake_chunks, fake_sources, staged = (ctypes.c_void_p(k << 20) for k in (1, 2, 3))

    def tables():
        sources = (_lib.ExrSource * 1)()
        f = sources[0]
        f.src, f.H, f.W, f.C, f.n_channels = 7 << 20, 20, 5, 3, 3
        for c in range(3):
            f.type[c], f.src_channel[c] = 2, 2 - c
        chunks = (_lib.ExrChunk * 2)()
        chunks[0].offset, chunks[0].file, chunks[0].row0, chunks[0].rows, chunks[0].coded = 0, 0, 0, 16, 1         # 16 * 60 = 960 bytes
        chunks[1].offset, chunks[1].file, chunks[1].row0, chunks[1].rows, chunks[1].coded = 960, 0, 16, 4, 1      # 240 bytes
        return chunks, sources

    def call(chunks, sources, n=2, chunks_dev=fake_chunks, sources_dev=fake_sources, n_sources=1, buf=staged, staged_bytes=1200):
        return lib.dd_exr_pack(chunks, chunks_dev, n, sources, sources_dev, n_sources, buf, staged_bytes, None)

    def refused(word, change=None, **k):
        chunks, sources = tables()
        if change:
            change(chunks, sources[0])
        assert call(chunks, sources, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()

    def setter(what, field, value, index=1):
        def change(chunks, f):
            target = f if what == "source" else chunks[index]
            if isinstance(field, tuple):
                getattr(target, field[0])[field[1]] = value
            else:
                setattr(target, field, value)
        return change
    assert lib.dd_exr_pack(None, None, 0, None, None, 0, None, 0, None) == 0            # no chunks: a no-op
    refused(b"n_chunks=-1", n=-1)
    chunks, sources = tables()
    assert call(None, sources) < 0 and b"null" in lib.dd_last_error()
    assert call(chunks, None) < 0 and b"null" in lib.dd_last_error()
    refused(b"null", chunks_dev=None)
    refused(b"null", sources_dev=None)
    refused(b"null", buf=None)
    refused(b"aligned", buf=ctypes.c_void_p((3 << 20) + 4))
    refused(b"n_sources=0", n_sources=0)
    refused(b"null plane", setter("source", "src", None))
    refused(b"H=0", setter("source", "H", 0))
    refused(b"W=0", setter("source", "W", 0))
    for c in (0, 33):
        refused(b"C=%d" % c, setter("source", "C", c))
    for n in (0, 9):
        refused(b"n_channels=%d" % n, setter("source", "n_channels", n))
    for t in (0, 3, -1):                                                               # UINT is refused: the planes are fp32
        refused(b"pixel type=%d" % t, setter("source", ("type", 1), t))
    for s in (-1, 3):
        refused(b"src_channel=%d" % s, setter("source", ("src_channel", 2), s))
    for rows in (0, 17):
        refused(b"rows=%d" % rows, setter("chunk", "rows", rows))
    for k in (-1, 1):
        refused(b"file=%d" % k, setter("chunk", "file", k))
    refused(b"row0=17", setter("chunk", "row0", 17))
    refused(b"row0=-1", setter("chunk", "row0", -1))
    refused(b"offset=968", setter("chunk", "offset", 968))
    refused(b"offset=-16", setter("chunk", "offset", -16))
    refused(b"staged bytes", staged_bytes=1199)
    # the numpy tables of the encoder are read the same way
    chunk = np.zeros(1, dtype=openexr.CHUNK_DTYPE)
    chunk[0] = (0, 0, 0, 1, 1)
    source = np.zeros(1, dtype=openexr.SOURCE_DTYPE)
    source[0]["src"], source[0]["H"], source[0]["W"], source[0]["C"], source[0]["n_channels"] = 7 << 20, 1, 4, 1, 1
    source[0]["type"][0] = 0
    assert lib.dd_exr_pack(chunk.ctypes.data, fake_chunks, 1, source.ctypes.data, fake_sources, 1, staged, 16, None) < 0
    assert b"pixel type=0" in lib.dd_last_error()
