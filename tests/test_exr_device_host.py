"""The host half of the device EXR decoder without a GPU: openexr.plan_file plus the numpy restatement of the kernel (tests/exr_device_ref.py)
must give the bits of openexr.read_image(path)[..., :channels] for every file of the fixture list, and every malformed file the message
read_exr gives."""
import struct
import types
import zlib

import numpy as np
import pytest

import exr_device_ref as R
from deepdenoiser_amd import openexr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return R.fixtures(str(tmp_path_factory.mktemp("exr_device_host")))


def test_plan_and_restated_kernel_equal_read_image(files):
    assert len(files) >= 40
    for name, path, channels in files:
        want = openexr.read_image(path)[..., :channels]
        plane, count, plan = R.decode_ref(path, channels)
        assert plane.shape == want.shape and plane.dtype == np.float32, name
        assert np.array_equal(R.bits(plane), R.bits(want)), name
        assert count == int(np.count_nonzero(~np.isfinite(want))), name
        # the staged layout the kernel's wide loads rely on
        assert all(int(o) % 16 == 0 for o in plan.chunks["offset"]) and plan.staged_bytes % 16 == 0, name
        ends = [int(ck["offset"]) + expected for ck, (_, _, expected) in zip(plan.chunks, plan.pieces)]
        assert all(e <= int(nxt) for e, nxt in zip(ends, list(plan.chunks["offset"][1:]) + [plan.staged_bytes])), name


def test_the_fixtures_hold_what_they_are_meant_to(files):
    by_name = {name: path for name, path, _ in files}
    kinds = R.chunk_kinds(by_name["zip_with_raw_chunk"])
    assert kinds == [True, False, True]                                        # chunk 1 (rows 16 .. 31: random bits) did not shrink
    kinds = R.chunk_kinds(by_name["rle_coded_and_raw"])
    assert [k for k, coded in enumerate(kinds) if coded] == [0, 3, 4, 9] and len(kinds) == 12
    assert not any(R.chunk_kinds(by_name["rle_37x21"]))                        # the smooth image is stored raw under RLE in all 37 lines
    assert all(R.chunk_kinds(by_name["zip_37x21"])) and len(R.chunk_kinds(by_name["zip_37x21"])) == 3
    plan = openexr.plan_file(by_name["zip_20x1100_rgba"])
    assert max(expected for _, _, expected in plan.pieces) == 16 * 1100 * 16 > 160 * 1024      # larger than LDS
    assert plan.dst_masks == [0, 4, 2, 1] and plan.types == [2, 2, 2, 2]      # A, B, G, R in file order; A is skipped
    assert openexr.plan_file(by_name["single_y_replicated"], 3).dst_masks == [7]
    assert openexr.plan_file(by_name["single_y_one_channel"], 1).dst_masks == [1]
    assert openexr.plan_file(by_name["rgb_first_two"], 2).dst_masks == [0, 2, 1]
    assert openexr.plan_file(by_name["data_window_moved"]).chunks["row0"].tolist() == [0, 16, 32]
    half = openexr.read_image(by_name["half_every_pattern"])[..., 0]
    assert np.array_equal(half.astype(np.float16).view(np.uint16)[~np.isnan(half)], np.arange(65536, dtype=np.uint16)[~np.isnan(half.reshape(-1))])


def test_the_restated_kernel_skips_what_the_kernel_skips():
    staged = np.zeros(64, dtype=np.uint8)
    file = (2, 3, 1, [2], [1])
    table = np.zeros(5, dtype=openexr.CHUNK_DTYPE)
    table[0] = (0, 1, 0, 1, 0)       # file index out of range
    table[1] = (0, 0, 2, 1, 0)       # rows outside [0, H)
    table[2] = (0, 0, -1, 1, 0)
    table[3] = (8, 0, 0, 1, 0)       # offset not aligned
    table[4] = (64, 0, 0, 1, 0)      # leaves the staged bytes
    planes, counts = R.reconstruct(staged + 0x7F, table, [file])
    assert not planes[0].any() and counts == [0]


# ---------------------------------------------------------------------------------------------------- malformed files: read_exr's messages
def _both(path):
    with pytest.raises(openexr.ExrError) as host:
        openexr.read_exr(path)
    with pytest.raises(openexr.ExrError) as device:
        plan = openexr.plan_file(path)
        plan.inflate(np.zeros(max(plan.staged_bytes, 16), dtype=np.uint8))
    assert str(device.value) == str(host.value)
    return str(host.value)


def _single_chunk_file(tmp_path, compression, name):
    path = str(tmp_path / name)
    openexr.write_image(path, R.smooth(1 if compression != openexr.ZIP_COMPRESSION else 8, 40, 3), compression)
    if compression == openexr.RLE_COMPRESSION:
        openexr.write_image(path, np.full((1, 40, 3), 0.5, dtype=np.float32), compression)
    buf = open(path, "rb").read()
    head, pos = openexr._parse_header(buf)
    (off,) = struct.unpack_from("<Q", buf, pos)
    return path, buf, off


def test_malformed_files_raise_the_messages_of_read_exr(tmp_path):
    good = str(tmp_path / "good.exr")
    openexr.write_image(good, R.smooth(37, 21, 3))
    buf = open(good, "rb").read()
    head, pos = openexr._parse_header(buf)
    offsets = struct.unpack_from("<3Q", buf, pos)

    def variant(name, data):
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        return path
    assert "too short" in _both(variant("short.exr", buf[:6]))
    assert "truncated or malformed header" in _both(variant("header.exr", buf[:40]))
    assert "truncated offset table" in _both(variant("table.exr", buf[:pos + 12]))
    assert "past the end of the file" in _both(variant("offset.exr", buf[:offsets[2] + 4]))
    assert "bad chunk" in _both(variant("cut.exr", buf[:-5]))
    moved = bytearray(buf)
    struct.pack_into("<i", moved, offsets[1], -16)
    assert "bad chunk (y -16" in _both(variant("y.exr", bytes(moved)))
    struct.pack_into("<i", moved, offsets[1], 48)
    assert "bad chunk (y 48" in _both(variant("y2.exr", bytes(moved)))
    assert "magic" in _both(variant("magic.exr", b"\1\2\3\4" + buf[4:]))
    # a chunk that inflates / run-length decodes to the wrong size; a NONE chunk of the wrong size
    path, one, off = _single_chunk_file(tmp_path, openexr.ZIP_COMPRESSION, "zip1.exr")
    wrong = zlib.compress(b"\0" * 100)
    assert "chunk expands to 100 bytes, expected 3840" in _both(variant("inflated.exr", one[:off] + struct.pack("<ii", 0, len(wrong)) + wrong))
    path, one, off = _single_chunk_file(tmp_path, openexr.RLE_COMPRESSION, "rle1.exr")
    assert R.chunk_kinds(path) == [True]
    wrong = bytes([9, 7])                                                       # a run of ten bytes
    assert "run-length coded chunk expands to 10 bytes, expected 480" in _both(variant("run.exr", one[:off] + struct.pack("<ii", 0, len(wrong)) + wrong))
    path, one, off = _single_chunk_file(tmp_path, openexr.NO_COMPRESSION, "none1.exr")
    assert "chunk of 100 bytes where 480 are expected" in _both(variant("none.exr", one[:off] + struct.pack("<ii", 0, 100) + b"\0" * 100))
    # no R, G, B among several channels
    path = str(tmp_path / "xy.exr")
    openexr.write_exr(path, {"X": np.zeros((2, 2), np.float32), "Z": np.zeros((2, 2), np.float32)})
    with pytest.raises(openexr.ExrError) as host:
        openexr.read_image(path)
    with pytest.raises(openexr.ExrError) as device:
        openexr.plan_file(path)
    assert str(device.value) == str(host.value) and "no R, G, B channels" in str(host.value)
    # unsupported codecs and layouts keep their message too
    piz = bytearray(buf)
    at = piz.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    piz[at] = 4
    assert "compression PIZ is not supported" in _both(variant("piz.exr", bytes(piz)))


# ---------------------------------------------------------------------------------------------------- the opt-in
def test_device_decode_needs_a_gpu_and_host_stays_the_default():
    from deepdenoiser_amd import predict, statistics, train
    from deepdenoiser_amd.frame_bank import FrameBank
    with pytest.raises(ValueError):
        openexr.DeviceDecoder("cpu")
    frame_set = types.SimpleNamespace(tile=8, number_of_sources_per_example=1, source_spps=[4], scenes=[])
    with pytest.raises(ValueError):
        FrameBank.for_passes(frame_set, {"Normal": 3}, {}, 4, device="cpu", decode="device")
    with pytest.raises(ValueError):
        FrameBank.for_passes(frame_set, {"Normal": 3}, {}, 4, device="cpu", decode="elsewhere")
    assert FrameBank.for_passes(frame_set, {"Normal": 3}, {}, 4, device="cpu").decode == "host"
    for parser, argv in ((train.parser(), ["t.json"]), (statistics.parser(), ["t.json"]), (predict.parser(), ["a.json"])):
        assert parser.parse_args(argv).exr_decode == "host"
        assert parser.parse_args(argv + ["--exr_decode", "device"]).exr_decode == "device"
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--exr_decode", "gpu"])
    assert openexr.CHUNK_DTYPE.itemsize == 24 and openexr.FILE_DTYPE.itemsize == 88
    with pytest.raises(ValueError):
        openexr.plan_file("nothing.exr", 0)
