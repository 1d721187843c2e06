"""The reference helpers of the PNG tests (tests/png_ref.py) against what does not depend on this project: summaries.decode_png on type-0
files, Pillow where it is installed, zlib's Adler-32 and its Z_SYNC_FLUSH segments; and the host path of deepdenoiser_amd/png.py against the
reference: the byte of every threshold edge, the five filters, the file."""
import struct
import zlib

import numpy as np
import pytest

import png_ref as P
from deepdenoiser_amd import png, summaries


def _sync_flush_file(image, exposure, segment_rows):
    """a file whose IDAT is put together from zlib Z_SYNC_FLUSH segments, as the device's is from its own"""
    rows = P.filtered_rows(image, exposure)
    bodies, adlers, lengths = [], [], []
    for y0 in range(0, rows.shape[0], segment_rows):
        t = rows[y0:y0 + segment_rows].tobytes()
        last = y0 + segment_rows >= rows.shape[0]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        bodies.append(c.compress(t) + (c.flush() if last else c.flush(zlib.Z_SYNC_FLUSH)))
        adlers.append(zlib.adler32(t))
        lengths.append(len(t))
    n = 1 if np.asarray(image).ndim == 2 else np.asarray(image).shape[2]
    return png.file_bytes(rows.shape[0], (rows.shape[1] - 1) // n, n, P.stream_of(bodies, adlers, lengths))


def test_decoder_agrees_with_decode_png_on_type_0_files():
    rng = np.random.default_rng(1)
    for shape in ((5, 7, 3), (4, 9), (1, 1, 3), (13, 2)):
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        data = summaries.encode_png(a)
        have = P.decode(data)
        want = summaries.decode_png(data)
        assert np.array_equal(have["image"].reshape(want.shape), want) and np.array_equal(want, a)
        assert have["filters"] == [0] * shape[0] and have["chunks"] == [b"IHDR", b"IDAT", b"IEND"]
    broken = bytearray(summaries.encode_png(np.zeros((2, 2), dtype=np.uint8)))
    broken[-5] ^= 1
    with pytest.raises(AssertionError):
        P.decode(bytes(broken))


def test_unfilter_inverts_every_filter_type():
    rng = np.random.default_rng(2)
    for n in (1, 3):
        q = rng.integers(0, 256, size=(6, 9, n), dtype=np.uint8)
        flat, up = q.reshape(6, 9 * n).astype(int).tolist(), [0] * (9 * n)
        for kind in range(5):                                     # every row forced to one type
            rows = np.zeros((6, 1 + 9 * n), dtype=np.uint8)
            up = [0] * (9 * n)
            for y in range(6):
                cur = flat[y]
                for i in range(9 * n):
                    a, b, c = (cur[i - n] if i >= n else 0), up[i], (up[i - n] if i >= n else 0)
                    rows[y, 1 + i] = (cur[i] - (0, a, b, (a + b) // 2, P._paeth(a, b, c))[kind]) % 256
                rows[y, 0] = kind
                up = cur
            image, kinds = P.unfilter(rows, 9, n)
            assert np.array_equal(image, q) and kinds == [kind] * 6


def test_the_reference_picks_each_of_the_five_filter_types():
    seen = set()
    for name, image, exposure, _ in P.images():
        rows = P.filtered_rows(image, exposure)
        seen.update(int(k) for k in rows[:, 0])
        assert np.array_equal(png.filtered_rows(image, exposure), rows), name
        assert np.array_equal(P.unfilter(rows, image.shape[1], image.shape[2])[0], P.quantise(image, exposure)), name
    assert seen == {0, 1, 2, 3, 4}
    alone = P.filtered_rows(P.all_filters_image(17, 21, 3))
    assert set(int(k) for k in alone[:, 0]) == {0, 1, 2, 3, 4}    # uniform random bytes at 17 x 21 do it alone


def test_threshold_edges():
    t = P.THRESHOLDS
    below, above = np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf))
    k = np.arange(1, 256)
    for quantise in (P.quantise, png.quantise):
        assert np.array_equal(quantise(t.reshape(1, 255, 1))[0, :, 0], k)                 # at the entry: it counts
        assert np.array_equal(quantise(above.reshape(1, 255, 1))[0, :, 0], k)
        assert np.array_equal(quantise(below.reshape(1, 255, 1))[0, :, 0], k - 1)         # just below: it does not
        special = np.array([np.inf, -np.inf, -1.0, -0.0, 0.0, np.nan, 1e30, -1e-30], dtype=np.float32).reshape(1, 8, 1)
        assert quantise(special)[0, :, 0].tolist() == [255, 0, 0, 0, 0, 0, 255, 0]        # a NaN gray sample is 0
        rgb = np.array([[[0.5, np.nan, 0.5], [np.nan, np.nan, np.nan], [np.inf, -np.inf, -0.0], [1.0, 0.0, 1.0]]], dtype=np.float32)
        assert quantise(rgb)[0].tolist() == [[255, 0, 255], [255, 0, 255], [255, 0, 0], [255, 0, 255]]
        # exposure 2.5: one fp32 multiply, then the same count
        values = P.edge_values().reshape(1, -1, 1)
        with np.errstate(over="ignore", invalid="ignore"):
            scaled = (values * np.float32(2.5)).astype(np.float32)
        assert np.array_equal(quantise(values, 2.5), quantise(scaled, 1.0))
        assert not np.array_equal(quantise(values, 2.5), quantise(values, 1.0))
    image = P.edge_image(38, 21, 3)
    assert np.array_equal(P.quantise(image, 2.5), png.quantise(image, 2.5))


def test_adler_combine_equals_adler32_of_the_concatenation():
    rng = np.random.default_rng(3)
    for lengths in ((1, 1), (5, 70000), (70000, 3), (65521, 65521, 1), (100000, 200000, 65522), (1, 2, 3, 4, 5)):
        parts = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lengths]
        parts[0] = b"\xff" * lengths[0]                            # (large sums)
        for combine in (P.adler_combine, png.adler_combine):
            adler = 1
            for t in parts:
                adler = combine(adler, zlib.adler32(t), len(t))
            assert adler == zlib.adler32(b"".join(parts)), lengths


def test_encode_host_files_decode_to_the_reference():
    for name, image, exposure, segment_rows in P.images():
        data = png.encode_host(image, exposure)
        have = P.decode(data)
        assert have["chunks"] == [b"IHDR", b"sRGB", b"IDAT", b"IEND"] and have["srgb"] == b"\x00", name
        assert np.array_equal(have["image"], P.quantise(image, exposure)), name
        assert np.array_equal(have["rows"], P.filtered_rows(image, exposure)), name
        assert struct.unpack(">IIBBBBB", data[16:29]) == (image.shape[1], image.shape[0], 8, 2 if image.shape[2] == 3 else 0, 0, 0, 0)
        assert np.array_equal(P.decode(_sync_flush_file(image, exposure, segment_rows))["image"], P.quantise(image, exposure)), name
    gray = P.noisy_gradient(9, 5, 1)[:, :, 0]                    # [H, W] is a gray pass
    assert np.array_equal(P.decode(png.encode_host(gray))["image"], P.quantise(gray))
    for bad in (np.zeros((3, 3, 2), dtype=np.float32), np.zeros((0, 3, 3), dtype=np.float32), np.zeros(3, dtype=np.float32)):
        with pytest.raises(png.PngError):
            png.encode_host(bad)


def test_pillow_opens_the_files():
    Image = pytest.importorskip("PIL.Image")
    import io
    for name, image, exposure, segment_rows in P.images():
        want = P.quantise(image, exposure)
        for data in (png.encode_host(image, exposure), _sync_flush_file(image, exposure, segment_rows)):
            picture = Image.open(io.BytesIO(data))
            picture.load()
            assert picture.mode == ("RGB" if image.shape[2] == 3 else "L"), name
            assert np.array_equal(np.asarray(picture).reshape(want.shape), want), name
