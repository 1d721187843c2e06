"""The host half of the device EXR encoder without a device: plan_write's header and slot layout, assemble fed with streams made by zlib (and
some chunks marked RAW) read back bit-identical by read_exr, the usage errors of --exr_encode / --exr_type, and HALF output through the
unchanged host writer."""
import zlib

import numpy as np
import pytest

from deepdenoiser_amd import openexr, predict

from exr_device_ref import bits, random_finite_bits, smooth

COMPRESSIONS = {"zip": openexr.ZIP_COMPRESSION, "zips": openexr.ZIPS_COMPRESSION, "none": openexr.NO_COMPRESSION}


@pytest.mark.parametrize("compression", sorted(COMPRESSIONS))
@pytest.mark.parametrize("names,types", [(["R", "G", "B"], ["float"] * 3), (["Y"], ["half"]), (["b.G", "a.R", "c.B", "A"], ["half", "float", "half", "float"])])
def test_header_equals_write_exr(tmp_path, compression, names, types):
    img = smooth(21, 9, len(names), seed=3)
    path = str(tmp_path / "host.exr")
    chans = {n: np.ascontiguousarray(img[..., k]).astype(np.float16 if t == "half" else np.float32) for k, (n, t) in enumerate(zip(names, types))}
    openexr.write_exr(path, chans, COMPRESSIONS[compression])
    plan = openexr.plan_write(path, 21, 9, names, types, COMPRESSIONS[compression])
    written = open(path, "rb").read()
    assert written[:len(plan.header)] == plan.header
    head, pos = openexr._parse_header(written)
    assert pos == len(plan.header)
    assert plan.names == sorted(names) and plan.src_channels == [names.index(n) for n in plan.names]


@pytest.mark.parametrize("compression,lines", [("zip", 16), ("zips", 1), ("none", 1)])
def test_slot_layout(compression, lines):
    H, W = 37, 21
    plan = openexr.plan_write("x.exr", H, W, ["R", "G", "B"], ["half", "float", "half"], COMPRESSIONS[compression])
    row_bytes = W * (2 + 4 + 2)
    n_chunks = (H + lines - 1) // lines
    assert len(plan.chunks) == len(plan.raw_bytes) == n_chunks
    assert plan.coded == (compression != "none")
    at = 0
    for k, (record, n) in enumerate(zip(plan.chunks, plan.raw_bytes)):
        rows = min(lines, H - k * lines)
        assert (int(record["offset"]), int(record["row0"]), int(record["rows"]), int(record["coded"])) == (at, k * lines, rows, int(plan.coded))
        assert n == rows * row_bytes and at % 16 == 0
        at += (n + 15) // 16 * 16
    assert plan.slot_bytes == at
    assert plan.raw_bytes[-1] == (H - (n_chunks - 1) * lines) * row_bytes          # the short last chunk (37 = 2 * 16 + 5)
    streams = plan.streams()
    assert list(streams["src_offset"]) == list(streams["dst_offset"]) == list(plan.chunks["offset"])
    assert list(streams["src_bytes"]) == plan.raw_bytes and list(streams["dst_capacity"]) == [n - 1 for n in plan.raw_bytes]


def test_plan_refusals():
    with pytest.raises(openexr.ExrError):
        openexr.plan_write("x.exr", 4, 4, ["Y"], ["float"], openexr.RLE_COMPRESSION)
    with pytest.raises(ValueError):
        openexr.plan_write("x.exr", 4, 4, ["Y"], ["uint"])
    with pytest.raises(openexr.ExrError):
        openexr.plan_write("x.exr", 0, 4, ["Y"], ["float"])
    with pytest.raises(openexr.ExrError):
        openexr.plan_write("x.exr", 4, 4, ["Y", "Y"], ["float", "float"])


def _fill(plan, chans, force_raw=()):
    """what the two launches leave in the file's slots, made with numpy and zlib -> (statuses, sizes, slots)"""
    arrs = [chans[n] for n in plan.names]
    slots = np.full(plan.slot_bytes, 0xA5, dtype=np.uint8)
    statuses, sizes = [], []
    for k, (record, n) in enumerate(zip(plan.chunks, plan.raw_bytes)):
        raw = b"".join(a[r].tobytes() for r in range(record["row0"], record["row0"] + record["rows"]) for a in arrs)
        assert len(raw) == n
        stream = zlib.compress(openexr._interleave_and_predict(raw), 1) if plan.coded else raw
        at = int(record["offset"])
        if plan.coded and len(stream) < n and k not in force_raw:
            statuses.append(openexr.DEFLATE_OK)
            sizes.append(len(stream))
            slots[at:at + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
        else:
            statuses.append(openexr.DEFLATE_RAW)
            sizes.append(0)
            slots[at:at + n] = np.frombuffer(raw, dtype=np.uint8)
    return statuses, sizes, slots


@pytest.mark.parametrize("compression", sorted(COMPRESSIONS))
def test_assemble_reads_back_bit_identical(tmp_path, compression):
    img = smooth(37, 21, 3, seed=9)
    img[16:32] = random_finite_bits(np.random.default_rng(2), (16, 21, 3))        # (under ZIP this chunk does not shrink)
    names, types = ["R", "G", "B"], ["float", "half", "float"]
    with np.errstate(over="ignore"):
        chans = {"R": img[..., 0].copy(), "G": img[..., 1].astype(np.float16), "B": img[..., 2].copy()}
    plan = openexr.plan_write(str(tmp_path / "a.exr"), 37, 21, names, types, COMPRESSIONS[compression])
    statuses, sizes, slots = _fill(plan, chans, force_raw=(0,))
    if compression == "zip":
        assert statuses[0] == openexr.DEFLATE_RAW and statuses[2] == openexr.DEFLATE_OK      # (chunk 0 marked RAW although it shrinks)
    data = openexr.assemble(plan, statuses, sizes, slots)
    open(plan.path, "wb").write(data)
    planes, head = openexr.read_exr(plan.path)
    assert head["compression"] == COMPRESSIONS[compression]
    for name in names:
        assert np.array_equal(bits(planes[name]), bits(chans[name].astype(np.float32))), name
    if plan.coded:                                                                # a status that is neither OK nor RAW is no file
        with pytest.raises(openexr.ExrError):
            openexr.assemble(plan, [openexr.DEFLATE_RECORD] * len(statuses), sizes, slots)


def test_assemble_of_compressible_chunks_equals_the_host_writer_with_the_same_streams(tmp_path):
    """with zlib's default level in the slots the file is write_exr's, byte for byte"""
    img = (np.round(smooth(20, 13, 3, seed=4) * 64) / 64).astype(np.float32)      # (few distinct values: every chunk shrinks)
    host, path = str(tmp_path / "host.exr"), str(tmp_path / "planned.exr")
    openexr.write_image(host, img)
    plan = openexr.plan_write(path, 20, 13, ["R", "G", "B"], ["float"] * 3, src_channels=[0, 1, 2])
    arrs = [np.ascontiguousarray(img[..., "RGB".index(n)]) for n in plan.names]
    slots, statuses, sizes = np.zeros(plan.slot_bytes, dtype=np.uint8), [], []
    for record, n in zip(plan.chunks, plan.raw_bytes):
        raw = b"".join(a[r].tobytes() for r in range(record["row0"], record["row0"] + record["rows"]) for a in arrs)
        stream = zlib.compress(openexr._interleave_and_predict(raw))
        assert len(stream) < n
        slots[record["offset"]:record["offset"] + len(stream)] = np.frombuffer(stream, dtype=np.uint8)
        statuses.append(0)
        sizes.append(len(stream))
    assert openexr.assemble(plan, statuses, sizes, slots) == open(host, "rb").read()


def test_usage_errors_of_the_new_options(capsys):
    parser = predict.parser()
    for bad, word in ((["a.json", "--exr_encode", "device"], "--exr_encode device needs --exr"), (["a.json", "--exr_type", "half"], "--exr_type half needs --exr"),
                      (["a.json", "--exr", "--exr_encode", "gpu"], "invalid choice"), (["a.json", "--exr", "--exr_type", "uint"], "invalid choice")):
        with pytest.raises(SystemExit) as stop:
            parser.parse_args(bad)
        assert stop.value.code == 2 and word in capsys.readouterr().err
    args = parser.parse_args(["a.json"])
    assert (args.exr, args.exr_encode, args.exr_type) == (False, "host", "float")                 # the defaults stay
    args = parser.parse_args(["a.json", "--exr", "--exr_encode", "device", "--exr_type", "half"])
    assert (args.exr_encode, args.exr_type) == ("device", "half")
    assert parser.parse_args(["a.json", "--exr", "--exr_type", "half"]).exr_encode == "host"


def test_save_predictions_arguments(tmp_path):
    img = smooth(5, 4, 3, seed=1)
    with pytest.raises(ValueError):
        openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": img}, as_exr=False, encode="device")
    with pytest.raises(ValueError):
        openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": img}, as_exr=True, encode="gpu")
    with pytest.raises(ValueError):
        openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": img}, as_exr=True, pixel_type="uint")
    with pytest.raises(ValueError):                                                                  # numpy predictions have no device
        openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": img}, as_exr=True, encode="device")
    with pytest.raises(ValueError):                                                                  # a device that is no GPU, before anything is allocated
        openexr.DeviceEncoder("cpu")


def test_half_on_the_host_path_round_trips_to_float16(tmp_path):
    rng = np.random.default_rng(5)
    colour = (smooth(19, 7, 3, seed=2) * np.exp(3 * rng.standard_normal((19, 7, 3)))).astype(np.float32)
    colour[0, 0] = (65504.0, 65520.0, 1e6)
    colour[1, 0] = (1e-7, -6e-8, 0.0)
    alpha = rng.random((19, 7, 1)).astype(np.float32)
    written = openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": colour, "Alpha": alpha}, as_exr=True, pixel_type="half")
    assert [p.rsplit("/", 1)[-1] for p in written] == ["Diffuse.npy", "Diffuse.exr", "Alpha.npy", "Alpha.exr"]
    assert np.array_equal(bits(np.load(written[0])), bits(colour)) and np.array_equal(bits(np.load(written[2])), bits(alpha))      # .npy as ever
    with np.errstate(over="ignore"):
        want = colour.astype(np.float16).astype(np.float32)
    assert np.array_equal(bits(openexr.read_image(written[1])), bits(want))
    planes, _ = openexr.read_exr(written[3])
    assert list(planes) == ["Y"] and np.array_equal(bits(planes["Y"]), bits(alpha[..., 0].astype(np.float16).astype(np.float32)))
    # and the default is what it was: FLOAT channels, bit-identical
    again = openexr.save_predictions(str(tmp_path), {"prediction/Diffuse": colour}, as_exr=True)
    assert np.array_equal(bits(openexr.read_image(again[1])), bits(colour))
