"""Image summaries, host side (no GPU): the threshold table of metrics.preview_thresholds against the sRGB transfer function, the PNG
codec and the Summary.Value.image field of summaries.py, metrics.preview_plan, and tests/preview_ref.py against itself on the cases the
device test uses."""
import io
import struct
import zlib

import numpy as np
import pytest

import preview_ref as PR
from deepdenoiser_amd import configs, summaries
from deepdenoiser_amd import metrics as M
from deepdenoiser_amd import tfrecords as R
from deepdenoiser_amd.architecture import Architecture


# ---------------------------------------------------------------------------------------------------------------- thresholds
def test_thresholds_are_the_srgb_steps():
    t = M.preview_thresholds()
    assert t.dtype == np.float32 and t.shape == (255,)
    assert (np.diff(t) > 0).all() and t[0] > 0 and t[-1] < 1
    x = np.random.default_rng(0).uniform(-0.1, 1.1, 196608).astype(np.float32)
    got = np.searchsorted(t, x, side="right")
    want = np.floor(255.0 * M.srgb_oetf(np.clip(x.astype(np.float64), 0.0, 1.0)) + 0.5).astype(np.int64)
    band = PR.near_threshold(x, t, 1e-6)
    print("%d of %d values disagree, %d lie within a relative 1e-6 of a threshold" % ((got != want).sum(), x.size, band.sum()))
    assert (got == want)[~band].all()
    assert band.sum() <= 1e-3 * x.size
    assert got.min() == 0 and got.max() == 255 and (got[x < 0] == 0).all() and (got[x >= 1] == 255).all()
    assert abs(got.astype(np.int64) - want).max() <= 1
    # the ends of the table and its neighbours in fp32
    for k in (0, 1, 127, 253, 254):
        below, above = np.nextafter(t[k], np.float32(-np.inf)), np.nextafter(t[k], np.float32(np.inf))
        assert list(np.searchsorted(t, [below, t[k], above], side="right")) == [k, k + 1, k + 1]


def test_oetf_round_trip():
    y = np.linspace(0.0, 1.0, 4097)
    assert np.abs(M.srgb_oetf(M.srgb_inverse_oetf(y)) - y).max() < 1e-12
    assert M.srgb_oetf(0.0) == 0.0 and abs(M.srgb_oetf(1.0) - 1.0) < 1e-15


# ---------------------------------------------------------------------------------------------------------------- PNG
def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (33, 35, 3), (1, 1), (3, 5), (4, 9, 1)])
def test_png_round_trip(shape):
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    back = summaries.decode_png(summaries.encode_png(a))
    assert back.dtype == np.uint8 and np.array_equal(back, a.reshape(back.shape))
    assert back.shape == ((shape[0], shape[1], 3) if shape[2:] == (3,) else shape[:2])


def test_png_bytes_assembled_by_hand():
    """a 2 x 1 RGB image (width 2, height 1) and a 1 x 2 gray one, chunk by chunk from the PNG specification"""
    rgb = np.array([[[255, 0, 128], [1, 2, 3]]], dtype=np.uint8)
    want = (b"\x89PNG\r\n\x1a\n"
            + _chunk(b"IHDR", struct.pack(">II", 2, 1) + bytes([8, 2, 0, 0, 0]))       # width, height, depth 8, colour type 2 (RGB), no interlace
            + _chunk(b"IDAT", zlib.compress(bytes([0, 255, 0, 128, 1, 2, 3])))         # one row: filter type 0, then the pixels
            + _chunk(b"IEND", b""))
    assert summaries.encode_png(rgb) == want
    gray = np.array([[7], [9]], dtype=np.uint8)
    want = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">II", 1, 2) + bytes([8, 0, 0, 0, 0]))
            + _chunk(b"IDAT", zlib.compress(bytes([0, 7, 0, 9]))) + _chunk(b"IEND", b""))
    assert summaries.encode_png(gray) == want


def test_png_refuses_what_it_does_not_read():
    good = summaries.encode_png(np.zeros((2, 2, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        summaries.decode_png(b"not a png at all")
    with pytest.raises(ValueError):
        summaries.decode_png(good[:-5])
    broken = bytearray(good)
    broken[20] ^= 1      # inside IHDR: its CRC no longer holds
    with pytest.raises(ValueError):
        summaries.decode_png(bytes(broken))
    sixteen = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">II", 1, 1) + bytes([16, 0, 0, 0, 0]))
               + _chunk(b"IDAT", zlib.compress(bytes([0, 0, 0]))) + _chunk(b"IEND", b""))
    with pytest.raises(ValueError):
        summaries.decode_png(sixteen)
    filtered = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">II", 1, 1) + bytes([8, 0, 0, 0, 0]))
                + _chunk(b"IDAT", zlib.compress(bytes([1, 5]))) + _chunk(b"IEND", b""))
    with pytest.raises(ValueError):
        summaries.decode_png(filtered)
    for bad in (np.zeros((2, 2, 3), dtype=np.float32), np.zeros((2, 2, 2), dtype=np.uint8), np.zeros((0, 2, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            summaries.encode_png(bad)


def test_png_decodes_in_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for shape in ((5, 7, 3), (1, 1, 3), (6, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        im = Image.open(io.BytesIO(summaries.encode_png(a)))
        assert im.mode == ("RGB" if len(shape) == 3 else "L") and im.size == (shape[1], shape[0])
        assert np.array_equal(np.asarray(im), a)


# ---------------------------------------------------------------------------------------------------------------- events
_HISTO = {"min": -1.0, "max": 2.0, "num": 3.0, "sum": 1.5, "sum_squares": 5.25, "bucket_limit": [0.0, 1.0, 1.7976931348623157e308],
          "bucket": [1.0, 0.0, 2.0]}
# encode_event of the commit before images existed, for the three calls below
_BEFORE = (
    "0900000000004a934010072a99010a0b0a046c6f7373150000803e0a140a0d6c6561726e696e675f72617465156f12833a0a680a03642f312a6109000000000000f0bf"
    "11000000000000004019000000000000084021000000000000f83f29000000000000154032180000000000000000000000000000f03fffffffffffffef7f3a18000000"
    "000000f03f000000000000000000000000000000400a0a0a036d2f311500000040",
    "0900000000000000401a0d627261696e2e4576656e743a32",
    "09000000000000084010012a00",
)


def test_events_without_images_are_byte_identical():
    calls = (dict(wall_time=1234.5, step=7, scalars=[("loss", 0.25), ("learning_rate", 1e-3)], histograms=[("d/1", _HISTO)], tracked=[("m/1", 2.0)]),
             dict(wall_time=2.0, file_version="brain.Event:2"),
             dict(wall_time=3.0, step=1, scalars=[]))
    for kw, want in zip(calls, _BEFORE):
        assert summaries.encode_event(**kw).hex() == want
        assert summaries.encode_event(images=None, **kw).hex() == want and summaries.encode_event(images=[], **kw).hex() == want


def _varint(n):
    out = b""
    while True:
        b, n = n & 0x7F, n >> 7
        out += bytes([b | (0x80 if n else 0)])
        if not n:
            return out


def _ld(num, data):      # a length-delimited field
    return _varint((num << 3) | 2) + _varint(len(data)) + data


def test_image_event_bytes_assembled_by_hand():
    """Event { wall_time = 1 (double), step = 2 (varint), summary = 5 { value = 1 { tag = 1, image = 4 { height = 1, width = 2, colorspace = 3,
    encoded_image_string = 4 } } } } from event.proto / summary.proto; images come behind every other value."""
    png = summaries.encode_png(np.arange(300 * 2 * 3, dtype=np.uint8).reshape(300, 2, 3))      # height 300: a two-byte varint
    image = b"\x08" + _varint(300) + b"\x10" + _varint(2) + b"\x18" + _varint(3) + _ld(4, png)
    value = _ld(1, b"previews/combined/image/0") + _ld(4, image)
    scalar = _ld(1, b"loss") + b"\x15" + struct.pack("<f", 0.5)
    want = b"\x09" + struct.pack("<d", 10.0) + b"\x10" + _varint(5) + _ld(5, _ld(1, scalar) + _ld(1, value))
    got = summaries.encode_event(10.0, step=5, scalars=[("loss", 0.5)], images=[("previews/combined/image/0", 300, 2, png)])
    assert got == want
    assert summaries.encode_event(10.0, step=5, scalars=[("loss", 0.5)], images=[("previews/combined/image/0", 300, 2, 3, png)]) == want
    only = summaries.encode_event(10.0, step=5, images=[summaries.image_summary("g", np.zeros((2, 4), dtype=np.uint8))])
    gray = b"\x08\x02\x10\x04\x18\x01" + _ld(4, summaries.encode_png(np.zeros((2, 4), dtype=np.uint8)))
    assert only == b"\x09" + struct.pack("<d", 10.0) + b"\x10\x05" + _ld(5, _ld(1, _ld(1, b"g") + _ld(4, gray)))


def test_image_events_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 256, (5, 21, 3), dtype=np.uint8), rng.integers(0, 256, (3, 4), dtype=np.uint8)
    with summaries.EventFileWriter(str(tmp_path)) as w:
        w.add_scalars(1, [("loss", 1.0)])
        w.add_images(2, [summaries.image_summary("previews/a/image/0", a), summaries.image_summary("previews/b/image", b)])
        w.add_summaries(3, [("loss", 2.0)], [("d/1", _HISTO)], [("m/1", 3.0)])
        path = w.path
    events = summaries.read_events(path)
    assert [e["step"] for e in events] == [0, 1, 2, 3] and events[0]["file_version"] == summaries.FILE_VERSION
    assert [e["tags"] for e in events] == [[], ["loss"], ["previews/a/image/0", "previews/b/image"], ["loss", "d/1", "m/1"]]
    assert events[2]["scalars"] == [] and events[2]["histograms"] == [] and events[1]["images"] == [] and events[3]["images"] == []
    images = summaries.read_images(path)
    assert [(s, t) for s, t, _ in images] == [(2, "previews/a/image/0"), (2, "previews/b/image")]
    for (_, _, im), want, cs in zip(images, (a, b), (3, 1)):
        assert (im["height"], im["width"], im["colorspace"]) == (want.shape[0], want.shape[1], cs)
        assert np.array_equal(summaries.decode_png(im["png"]), want)
    assert summaries.read_scalars(path) == [(1, "loss", 1.0), (3, "loss", 2.0), (3, "m/1", 3.0)]
    # the framing is the TFRecord framing every other event has
    assert sum(1 for _ in R.read_records(path)) == 4


# ---------------------------------------------------------------------------------------------------------------- plan
_COMBINED = ["Diffuse", "Glossy", "Subsurface", "Transmission"]
_PASSES = ["Diffuse Color", "Diffuse Direct", "Diffuse Indirect", "Glossy Color", "Glossy Direct", "Glossy Indirect", "Subsurface Color",
           "Subsurface Direct", "Subsurface Indirect", "Transmission Color", "Transmission Direct", "Transmission Indirect", "Volume Direct",
           "Volume Indirect", "Emission", "Environment", "Alpha"]


def test_preview_plan_of_the_example_architecture():
    arch = Architecture(configs.example_architecture(), device="cpu")
    tj = configs.training()
    plan = M.preview_plan(arch, tj, "combined")
    assert [e.source for e in plan] == [("image", "Combined")] + [("combined", c) for c in _COMBINED]
    assert [e.name for e in plan] == ["combined", "combined_diffuse", "combined_glossy", "combined_subsurface", "combined_transmission"]
    every = M.preview_plan(arch, tj, "all")
    assert every[:len(plan)] == plan
    assert sorted(e.source[1] for e in every[len(plan):]) == sorted(_PASSES) and all(e.source[0] == "feature" for e in every[len(plan):])
    assert [e.source[1] for e in every[len(plan):]] == [f.name for f in arch.feature_predictions if f.is_target and f.load_data]
    assert every[len(plan) + [e.source[1] for e in every[len(plan):]].index("Volume Direct")].name == "volume_direct"
    assert len({e.name for e in every}) == len(every)
    assert M.preview_tags("combined_diffuse", 3) == ["previews/combined_diffuse/image/%d" % k for k in range(3)]
    assert M.preview_tags("combined", 1) == ["previews/combined/image"]
    with pytest.raises(ValueError):
        M.preview_plan(arch, tj, "some")


def test_preview_plan_falls_back_to_the_passes():
    """features only: "combined" means "all"; one triple without the rest of the image: the triple alone"""
    aj = configs.architecture(combined={"Emission": {"Color": "Emission", "Direct": "", "Indirect": ""},
                                        "Environment": {"Color": "Environment", "Direct": "", "Indirect": ""}})
    arch = Architecture(aj, device="cpu")
    want = [M.PreviewEntry("emission", ("feature", "Emission")), M.PreviewEntry("environment", ("feature", "Environment"))]
    assert M.preview_plan(arch, configs.training(), "combined") == want == M.preview_plan(arch, configs.training(), "all")
    one = Architecture(configs.architecture(combined={"Diffuse": configs._FULL_COMBINED["Diffuse"]}), device="cpu")
    assert M.preview_plan(one, None, "combined") == [M.PreviewEntry("combined_diffuse", ("combined", "Diffuse"))]
    assert [e.source for e in M.preview_plan(one, None, "all")] == [("combined", "Diffuse"), ("feature", "Diffuse Color"), ("feature", "Diffuse Direct"),
                                                                    ("feature", "Diffuse Indirect")]


def test_panel_mask():
    assert M.preview_panel_mask(("source", "prediction", "target")) == 7 and M.preview_panel_mask(["difference", "target"]) == 12
    for bad in ((), ("sauce",)):
        with pytest.raises(ValueError):
            M.preview_panel_mask(bad)
    assert M.PREVIEW_PANELS == PR.PANELS


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def test_reference_mosaic_layout_and_specials():
    t = M.preview_thresholds()
    c = PR.case(PR.SMALL, 3, 2, 3)
    sides = PR.dyadic_sides(c, 1)
    assert PR.slots_of(c) == [0, 1, 2, 3, 4, PR.MAX_FEATURES, PR.IMAGE_SLOT]
    out = PR.mosaics(c, sides, PR.slots_of(c), 15, [2, 0, 2], t, kind="SMAPE")
    assert out.shape == (7, 3 * 2, 4 * 3, 3) and out.dtype == np.uint8
    assert np.array_equal(out[:, 0:2], out[:, 4:6]) and not np.array_equal(out[:, 0:2], out[:, 2:4])
    # panel 1 of slot 0 is the prediction of feature 0
    assert np.array_equal(out[0][:2, 3:6], PR.quantise(sides["prediction"][0][2], t))
    # the 1-channel pass is gray; so is every difference panel
    assert (out[4][..., 0] == out[4][..., 1]).all() and (out[:, :, 9:, 0] == out[:, :, 9:, 2]).all()
    # combined = colour x (direct + indirect), by hand for one pixel
    p = sides["target"]
    want = p[0][0, 1, 2] * (p[1][0, 1, 2] + p[2][0, 1, 2])
    assert np.array_equal(out[5][2 + 1, 6 + 2], np.searchsorted(t, want, side="right"))
    v = np.array([[np.nan, 0.5, 0.5], [np.inf, -np.inf, 0.0], [1.0, t[254], np.nextafter(t[254], np.float32(0))], [-1.0, 2.0, t[0]]])
    assert PR.quantise(v, t).tolist() == [[255, 0, 255], [255, 0, 0], [255, 255, 254], [0, 255, 1]]


def test_reference_difference_kinds():
    c = PR.case({"nch": [3, 1], "combined": [], "image": None}, 1, 1, 2)
    sides = {"source": None, "prediction": [np.array([[[[1.0, 0.5, -0.25], [2.0, 0.0, 0.0]]]]), np.array([[[[0.5], [0.25]]]])],
             "target": [np.array([[[[0.5, 0.5, 0.25], [0.0, 0.0, 1.0]]]]), np.array([[[[1.0], [0.25]]]])]}
    want = {"DIFFERENCE": ([0.0, 1.0], [0.5, 0.0]), "ABSOLUTE": ([1.0, 3.0], [0.5, 0.0]), "SQUARED": ([0.5, 5.0], [0.25, 0.0]),
            "SMOOTH_ABSOLUTE": ([0.25, 2.0], [0.125, 0.0])}
    for kind, (f0, f1) in want.items():
        for slot, w in ((0, f0), (1, f1)):
            got = PR.panel_values(c, sides, slot, "difference", [0], kind=kind, error_gain=2.0)
            assert got.shape == (1, 2, 3) and got[0, :, 0].tolist() == [2.0 * x for x in w], (kind, slot)
    got = PR.panel_values(c, sides, 0, "difference", [0], kind="SMAPE")[0, :, 0]
    want = [0.5 / 1.51 + 0.0 + 0.5 / 0.51, 2.0 / 2.01 + 0.0 + 1.0 / 1.01]
    assert np.abs(got - want).max() < 1e-6
