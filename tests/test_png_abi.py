"""dd_png_pack and dd_png_deflate without a GPU: the ctypes and numpy mirrors of their records against a C compile of include/dd_hip.h, the
exported symbols, the build lists, every host-side refusal (validation reads the HOST copy of the tables and fails before any launch; the
device pointers are never dereferenced), the parser rules of predict, and plan_png / assemble_png with RAW segments in every position."""
import ctypes
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_ref as P
from deepdenoiser_amd import _lib, png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structs_and_constants_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_png_image), offsetof(dd_png_image, src), offsetof(dd_png_image, H), offsetof(dd_png_image, W),
  offsetof(dd_png_image, C), offsetof(dd_png_image, n_channels), offsetof(dd_png_image, src_channel), offsetof(dd_png_image, exposure));
  printf(" %zu %zu %zu %zu %zu %zu", sizeof(dd_png_segment), offsetof(dd_png_segment, offset), offsetof(dd_png_segment, image), offsetof(dd_png_segment, y0),
  offsetof(dd_png_segment, rows), offsetof(dd_png_segment, reserved));
  printf(" %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_png_stream), offsetof(dd_png_stream, src_offset), offsetof(dd_png_stream, dst_offset),
  offsetof(dd_png_stream, src_bytes), offsetof(dd_png_stream, dst_capacity), offsetof(dd_png_stream, last), offsetof(dd_png_stream, reserved));
  printf(" %d %d %d\n", DD_PNG_MAX_ROW_BYTES, DD_PNG_STAGE_BYTES, DD_PREVIEW_THRESHOLDS); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    F, G, S = _lib.PngImage, _lib.PngSegment, _lib.PngStream
    assert have[:8] == [ctypes.sizeof(F), F.src.offset, F.H.offset, F.W.offset, F.C.offset, F.n_channels.offset, F.src_channel.offset,
                        F.exposure.offset] == [40, 0, 8, 12, 16, 20, 24, 36]
    assert have[8:14] == [ctypes.sizeof(G), G.offset.offset, G.image.offset, G.y0.offset, G.rows.offset, G.reserved.offset] == [24, 0, 8, 12, 16, 20]
    assert have[14:21] == [ctypes.sizeof(S), S.src_offset.offset, S.dst_offset.offset, S.src_bytes.offset, S.dst_capacity.offset, S.last.offset,
                           S.reserved.offset] == [32, 0, 8, 16, 20, 24, 28]
    assert have[21:] == [_lib.PNG_MAX_ROW_BYTES, _lib.PNG_STAGE_BYTES, _lib.PREVIEW_THRESHOLDS] == [12288, 36864, 255]
    assert (png.MAX_ROW_BYTES, png.STAGE_BYTES) == (12288, 36864) and [png.DEFLATE_OK, png.DEFLATE_RAW, png.DEFLATE_RECORD] == [0, 1, 2]
    for dtype, struct in ((png.IMAGE_DTYPE, F), (png.SEGMENT_DTYPE, G), (png.STREAM_DTYPE, S)):
        assert dtype.itemsize == ctypes.sizeof(struct)
        assert [(name, dtype.fields[name][1]) for name in dtype.names] == [(name, getattr(struct, name).offset) for name, _ in struct._fields_]
    core = open(os.path.join(ROOT, "deepdenoiser_amd", "csrc", "dd_png_core.h")).read()
    assert re.search(r"#define DD_PNG_THRESHOLDS 255\b", core)


def test_symbols_are_declared_built_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    for name in ("dd_png_pack", "dd_png_deflate", "dd_png_deflate_workspace"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint dd_png_pack\(const dd_png_segment\* segments_host, const dd_png_segment\* segments, int n_segments, const dd_png_image\* images_host", header)
    assert re.search(r"\bint dd_png_deflate\(const dd_png_stream\* streams_host, const dd_png_stream\* streams, int n_streams", header)
    for start, end in (("(csrc/dd_png_encode.hip, row coder", "} dd_png_image;"), ("(csrc/dd_png_encode.hip, coder core", "} dd_png_stream;")):
        comment = header[header.index(start):header.index(end)]
        assert "Prediction.py:483-510" in comment and "cv2.imwrite" in comment and "Refused with a negative status" in comment
    from deepdenoiser_amd import build
    assert "dd_png_encode.hip" in build.SOURCES and "dd_png_core.h" in build.HEADERS and "dd_deflate_core.h" in build.HEADERS
    assert build.NO_SCRATCH["dd_png_encode.hip"] == ("png_pack_kernel", "png_deflate_kernel")
    assert build.NO_SCRATCH["dd_exr_encode.hip"] == ("exr_pack_kernel",) and build.NO_SCRATCH["dd_exr_deflate.hip"] == ("exr_deflate_kernel",)
    for name in ("dd_png_encode.hip", "dd_png_core.h"):
        source = open(os.path.join(build.CSRC, name)).read()
        assert "asm" not in source.replace("assembly", "")                                # plain C++ only
    assert lib.dd_png_deflate_workspace(3) == 3 * 4 * _lib.DEFLATE_BLOCK_TOKENS and lib.dd_png_deflate_workspace(0) == 0


def test_deflate_host_side_refusals(lib):
    fake_table, src, out, work, status, sizes, adler = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6, 7))
    need = lib.dd_png_deflate_workspace(2)

    def table():
        streams = (_lib.PngStream * 2)()
        for k, s in enumerate(streams):
            s.src_offset, s.dst_offset, s.src_bytes, s.dst_capacity, s.last = 112 * k, 112 * k, 100, 99, k
        return streams

    def call(streams, n=2, table_dev=fake_table, source=src, src_total=224, buf=out, out_bytes=224, workspace=work, workspace_bytes=need, st=status, sz=sizes,
             ad=adler):
        return lib.dd_png_deflate(streams, table_dev, n, source, src_total, buf, out_bytes, workspace, workspace_bytes, st, sz, ad, None)

    def refused(word, field=None, value=None, index=1, **k):
        streams = table()
        if field:
            setattr(streams[index], field, value)
        assert call(streams, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()
    assert lib.dd_png_deflate(None, None, 0, None, 0, None, 0, None, 0, None, None, None, None) == 0      # no streams: a no-op
    refused(b"n_streams=-1", n=-1)
    assert call(None) < 0 and b"null" in lib.dd_last_error()
    for name in ("table_dev", "source", "buf", "workspace", "st", "sz", "ad"):
        refused(b"null", **{name: None})
    refused(b"workspace_bytes", workspace_bytes=need - 1)
    refused(b"aligned", buf=ctypes.c_void_p((3 << 20) + 8))
    refused(b"aligned", workspace=ctypes.c_void_p((4 << 20) + 2))
    for n in (0, -5, (1 << 30) + 1):
        refused(b"src_bytes=%d" % n, "src_bytes", n)
    refused(b"dst_capacity=-1", "dst_capacity", -1)
    for flag in (2, -1):
        refused(b"last=%d" % flag, "last", flag)
    refused(b"src_offset=125", "src_offset", 125)
    refused(b"src_offset=-1", "src_offset", -1)
    refused(b"source bytes", src_total=211)
    refused(b"dst_offset=-16", "dst_offset", -16)
    refused(b"not 16-byte aligned", "dst_offset", 8, index=0)
    refused(b"output bytes", out_bytes=223)                 # (a capacity of 99 owns 112)
    refused(b"dst_offset=128", "dst_offset", 128)
    refused(b"overlap", buf=ctypes.c_void_p((2 << 20) + 16))
    # the numpy table of the encoder is read the same way
    record = np.zeros(1, dtype=png.STREAM_DTYPE)
    record[0] = (0, 0, 0, 16, 1, 0)
    assert lib.dd_png_deflate(record.ctypes.data, fake_table, 1, src, 100, out, 16, work, need, status, sizes, adler, None) < 0
    assert b"src_bytes=0" in lib.dd_last_error()


def test_pack_host_side_refusals(lib):
    fake_segments, fake_images, thresholds, staged = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4))

    def tables():
        images = (_lib.PngImage * 1)()
        f = images[0]
        f.src, f.H, f.W, f.C, f.n_channels, f.exposure = 7 << 20, 20, 5, 4, 3, 1.0
        for c in range(3):
            f.src_channel[c] = 2 - c
        segments = (_lib.PngSegment * 2)()
        segments[0].offset, segments[0].image, segments[0].y0, segments[0].rows = 0, 0, 0, 16           # 16 * 16 = 256 bytes
        segments[1].offset, segments[1].image, segments[1].y0, segments[1].rows = 256, 0, 16, 4         # 64 bytes
        return segments, images

    def call(segments, images, n=2, segments_dev=fake_segments, images_dev=fake_images, n_images=1, table=thresholds, buf=staged, staged_bytes=320):
        return lib.dd_png_pack(segments, segments_dev, n, images, images_dev, n_images, table, buf, staged_bytes, None)

    def refused(word, change=None, **k):
        segments, images = tables()
        if change:
            change(segments, images[0])
        assert call(segments, images, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()

    def setter(what, field, value, index=1):
        def change(segments, f):
            target = f if what == "image" else segments[index]
            if isinstance(field, tuple):
                getattr(target, field[0])[field[1]] = value
            else:
                setattr(target, field, value)
        return change
    assert lib.dd_png_pack(None, None, 0, None, None, 0, None, None, 0, None) == 0            # no segments: a no-op
    refused(b"n_segments=-1", n=-1)
    segments, images = tables()
    assert call(None, images) < 0 and b"null" in lib.dd_last_error()
    assert call(segments, None) < 0 and b"null" in lib.dd_last_error()
    refused(b"null", segments_dev=None)
    refused(b"null", images_dev=None)
    refused(b"null", buf=None)
    refused(b"thresholds is null", table=None)
    refused(b"4-byte aligned", table=ctypes.c_void_p((3 << 20) + 2))
    refused(b"aligned", buf=ctypes.c_void_p((4 << 20) + 4))
    refused(b"n_images=0", n_images=0)
    refused(b"staged_bytes=8", staged_bytes=8)
    refused(b"null plane", setter("image", "src", None))
    refused(b"H=0", setter("image", "H", 0))
    refused(b"W=0", setter("image", "W", 0))
    for c in (0, 33):
        refused(b"C=%d" % c, setter("image", "C", c))
    for n in (0, 2, 4):
        refused(b"n_channels=%d" % n, setter("image", "n_channels", n))
    for s in (-1, 4):
        refused(b"src_channel=%d" % s, setter("image", ("src_channel", 2), s))
    refused(b"a row of 12291 bytes", setter("image", "W", 4097))                          # too wide for the pack kernel's LDS
    refused(b"overlap", setter("image", "src", (4 << 20) - 16))                           # the plane runs into the staged buffer
    refused(b"overlap", setter("image", "src", (4 << 20) + 304))
    for rows in (0, -1):
        refused(b"rows=%d" % rows, setter("segment", "rows", rows))
    for k in (-1, 1):
        refused(b"image=%d" % k, setter("segment", "image", k))
    refused(b"y0=17", setter("segment", "y0", 17))
    refused(b"y0=-1", setter("segment", "y0", -1))
    refused(b"offset=264", setter("segment", "offset", 264))
    refused(b"offset=-16", setter("segment", "offset", -16))
    refused(b"staged bytes", staged_bytes=319)

    def tall(segments, f):                                                                # 2400 rows of 16 bytes: more than the kernel stages
        f.H, segments[1].y0, segments[1].rows = 4000, 16, 2400
    refused(b"the pack kernel stages", tall, staged_bytes=1 << 16)
    # the numpy tables of the encoder are read the same way
    plan = png.plan_png("x.png", 20, 5, 3, segment_rows=16)
    layout = png._tables_layout([plan])
    host = np.zeros(layout["bytes"], dtype=np.uint8)
    png.fill_tables(host, layout, [plan], [7 << 20], [4], [1.0], src_channels=[(2, 1, 5)])
    assert lib.dd_png_pack(host.ctypes.data, fake_segments, 2, host[layout["images_at"]:].ctypes.data, fake_images, 1, thresholds, staged, layout["total"], None) < 0
    assert b"src_channel=5" in lib.dd_last_error()


def test_predict_parser_rules(capsys):
    from deepdenoiser_amd import predict
    parser = predict.parser()
    for bad, word in ((["a.json", "--png_encode", "device"], "--png_encode device needs --png"), (["a.json", "--png", "--png_encode", "gpu"], "invalid choice")):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
        assert word in capsys.readouterr().err
    args = parser.parse_args(["a.json"])
    assert (args.png, args.png_encode, args.exposure) == (False, "host", 1.0)             # the defaults stay
    args = parser.parse_args(["a.json", "--png", "--png_encode", "device", "--exposure", "2.5"])
    assert (args.png, args.png_encode, args.exposure) == (True, "device", 2.5)
    assert parser.parse_args(["a.json", "--png"]).png_encode == "host"
    assert "--png_encode" in parser.format_help()
    exposure = next(a for a in parser._actions if a.dest == "exposure")
    assert "--png" in exposure.help and "--target" in exposure.help


def test_plan_png_layout():
    plan = png.plan_png("x.png", 1080, 1920, 3)
    assert plan.segment_rows == 6 and plan.row_bytes == 5761 and len(plan.segments) == 180     # 6 rows are the first to reach 32 KiB
    assert all(offset % 16 == 0 for offset in plan.offsets) and plan.slot_bytes == 180 * 34576
    assert png.plan_png("x.png", 1080, 1920, 1).segment_rows == 18
    assert png.plan_png("x.png", 50, 4096, 3).segment_rows == 2                                # capped by what the kernel stages
    plan = png.plan_png("x.png", 17, 21, 3, segment_rows=8)
    assert plan.segments == [(0, 8), (8, 8), (16, 1)] and plan.raw_bytes == [512, 512, 64] and plan.offsets == [0, 512, 1024] and plan.slot_bytes == 1088
    streams = plan.stream_table(base=32)
    assert streams["last"].tolist() == [0, 0, 1] and streams["dst_capacity"].tolist() == [511, 511, 63] and streams["src_offset"].tolist() == [32, 544, 1056]
    for bad in (dict(height=0, width=4, n_channels=3), dict(height=4, width=4, n_channels=2), dict(height=4, width=4097, n_channels=3),
                dict(height=4, width=4, n_channels=3, segment_rows=0), dict(height=4000, width=5, n_channels=3, segment_rows=2400)):
        with pytest.raises(png.PngError):
            png.plan_png("x.png", **bad)


def _slots_of(plan, rows, raw):
    """statuses, sizes, adlers, slots and staged of `plan` with zlib's Z_SYNC_FLUSH bodies standing in for the device's; `raw`: the RAW segments"""
    slots, staged = np.full(plan.slot_bytes, 0xA5, dtype=np.uint8), np.full(plan.slot_bytes, 0x5A, dtype=np.uint8)
    statuses, sizes, adlers = [], [], []
    for k, ((y0, count), at) in enumerate(zip(plan.segments, plan.offsets)):
        t = rows[y0:y0 + count].tobytes()
        staged[at:at + len(t)] = np.frombuffer(t, dtype=np.uint8)
        adlers.append(zlib.adler32(t))
        if k in raw:
            statuses.append(png.DEFLATE_RAW)
            sizes.append(0)
            continue
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        body = c.compress(t) + (c.flush() if k == len(plan.segments) - 1 else c.flush(zlib.Z_SYNC_FLUSH))
        assert len(body) < len(t)
        slots[at:at + len(body)] = np.frombuffer(body, dtype=np.uint8)
        statuses.append(png.DEFLATE_OK)
        sizes.append(len(body))
    return statuses, sizes, adlers, slots, staged


def test_assemble_png_with_raw_segments_in_every_position():
    image = P.noisy_gradient(40, 67, 3, noise=0.0)
    rows = P.filtered_rows(image)
    plan = png.plan_png("x.png", 40, 67, 3, segment_rows=10)
    assert len(plan.segments) == 4
    for raw in ((), (0,), (1,), (2,), (3,), (0, 3), (1, 2), (0, 1, 2, 3)):
        statuses, sizes, adlers, slots, staged = _slots_of(plan, rows, raw)
        data = png.assemble_png(plan, statuses, sizes, adlers, slots, staged)
        have = P.decode(data)
        assert have["chunks"] == [b"IHDR", b"sRGB", b"IDAT", b"IEND"] and have["idat"][:2] == b"\x78\x01"
        assert zlib.decompress(have["idat"]) == rows.tobytes(), raw
        assert np.array_equal(have["image"], P.quantise(image)), raw
        copied = slots.copy()                                       # the encoder's arrangement: the RAW bytes stand in the slots themselves
        for k in raw:
            at, n = plan.offsets[k], plan.raw_bytes[k]
            copied[at:at + n] = staged[at:at + n]
        assert png.assemble_png(plan, statuses, sizes, adlers, copied) == data
    # a RAW segment longer than one stored block
    big = P.all_filters_image(30, 1000, 3)
    rows = png.filtered_rows(big)
    plan = png.plan_png("x.png", 30, 1000, 3, segment_rows=12)
    assert plan.raw_bytes[0] > 65535 // 2 and max(plan.raw_bytes) <= png.STAGE_BYTES
    statuses, sizes, adlers, slots, staged = _slots_of(plan, rows, (0, 1, 2))
    assert zlib.decompress(P.decode(png.assemble_png(plan, statuses, sizes, adlers, slots, staged))["idat"]) == rows.tobytes()
    assert len(png.stored_blocks(b"\x01" * 70000, True)) == 70000 + 10 and zlib.decompress(png.stored_blocks(b"\x01" * 70000, True), -15) == b"\x01" * 70000
    # what the device may not have returned
    statuses, sizes, adlers, slots, staged = _slots_of(plan, rows, (0, 1, 2))
    with pytest.raises(png.PngError):
        png.assemble_png(plan, [png.DEFLATE_RECORD] + statuses[1:], sizes, adlers, slots, staged)
    plan = png.plan_png("x.png", 40, 67, 3, segment_rows=10)
    statuses, sizes, adlers, slots, staged = _slots_of(plan, P.filtered_rows(image), ())
    with pytest.raises(png.PngError):
        png.assemble_png(plan, statuses, [plan.raw_bytes[0]] + sizes[1:], adlers, slots, staged)
    broken = slots.copy()
    broken[plan.offsets[0] + sizes[0] - 1] = 0
    with pytest.raises(png.PngError):
        png.assemble_png(plan, statuses, sizes, adlers, broken, staged)


def test_save_predictions_host_pngs(tmp_path):
    from deepdenoiser_amd import openexr
    predictions = {"prediction/Diffuse": P.noisy_gradient(9, 13, 3), "prediction/Depth": P.noisy_gradient(9, 13, 1), "Combined": P.edge_image(9, 13, 3)}
    plain, pictures = tmp_path / "plain", tmp_path / "pictures"
    plain.mkdir()
    pictures.mkdir()
    written = openexr.save_predictions(str(plain), predictions)
    assert sorted(os.listdir(plain)) == ["Combined.npy", "Depth.npy", "Diffuse.npy"] and len(written) == 3      # without png nothing changes
    written = openexr.save_predictions(str(pictures), predictions, png=True, exposure=2.5)
    assert sorted(os.path.basename(p) for p in written) == ["Combined.npy", "Combined.png", "Depth.npy", "Depth.png", "Diffuse.npy", "Diffuse.png"]
    for key, value in predictions.items():
        name = key.split("/")[-1]
        assert open(plain / (name + ".npy"), "rb").read() == open(pictures / (name + ".npy"), "rb").read()
        assert np.array_equal(P.decode(open(pictures / (name + ".png"), "rb").read())["image"], P.quantise(np.load(pictures / (name + ".npy")), 2.5))
    with pytest.raises(ValueError):
        openexr.save_predictions(str(plain), predictions, png_encode="device")
    with pytest.raises(ValueError):
        openexr.save_predictions(str(plain), predictions, png=True, png_encode="gpu")
    with pytest.raises(ValueError):                                 # the device path takes device tensors
        openexr.save_predictions(str(plain), predictions, png=True, png_encode="device")
