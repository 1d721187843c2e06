"""Reference helpers of the PNG tests (TEST INFRASTRUCTURE ONLY): the picture of deepdenoiser_amd/png.py stated a second time and plainly -- a
count against the threshold table per sample, the five row filters byte by byte -- their inverse (an unfilter for all five types), a
whole-file decoder that checks every CRC, the Adler-32 combine, the test images every PNG test walks, and the corpus / result files of
tests/png_core_main.cpp."""
import hashlib
import struct
import zlib

import numpy as np

from deepdenoiser_amd.metrics import preview_thresholds
from deepdenoiser_amd.summaries import PNG_SIGNATURE

OK, RAW, RECORD = 0, 1, 2
THRESHOLDS = preview_thresholds()


# ---------------------------------------------------------------------------------------------------- the picture
def quantise(image, exposure=1.0):
    """uint8 [H, W, n] of fp32 [H, W, n]: per sample the number of table entries <= sample * exposure (fp32); NaN rules as in png.py"""
    a = np.asarray(image, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        v = (a * np.float32(exposure)).astype(np.float32)
        q = (THRESHOLDS[None, None, None, :] <= v[..., None]).sum(axis=3).astype(np.uint8)      # (a comparison with a NaN is false: 0)
    if a.shape[2] == 3:
        q[np.isnan(v).any(axis=2)] = (255, 0, 255)
    return q


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_row(cur, up, bpp):
    """-> (type, filtered bytes) of one row: cur / up lists of ints (up: zeros for the first row)"""
    n = len(cur)
    rows = []
    for kind in range(5):
        out = []
        for i in range(n):
            a = cur[i - bpp] if i >= bpp else 0
            b = up[i]
            c = up[i - bpp] if i >= bpp else 0
            predicted = (0, a, b, (a + b) // 2, _paeth(a, b, c))[kind]
            out.append((cur[i] - predicted) % 256)
        rows.append(out)
    costs = [sum(v if v < 128 else 256 - v for v in row) for row in rows]
    best = costs.index(min(costs))                                 # (the first minimum: the lowest type)
    return best, rows[best]


def filter_image(q):
    """uint8 [H, 1 + W * n] of a uint8 picture [H, W, n]"""
    H, W, n = q.shape
    flat = q.reshape(H, W * n).astype(int).tolist()
    out, up = np.zeros((H, 1 + W * n), dtype=np.uint8), [0] * (W * n)
    for y in range(H):
        kind, row = filter_row(flat[y], up, n)
        out[y, 0] = kind
        out[y, 1:] = row
        up = flat[y]
    return out


def filtered_rows(image, exposure=1.0):
    return filter_image(quantise(image, exposure))


def unfilter(rows, width, n):
    """uint8 [H, W, n] of filtered rows uint8 [H, 1 + W * n], all five filter types -> (picture, the types)"""
    rows = np.asarray(rows, dtype=np.uint8)
    H = rows.shape[0]
    out, up, kinds = np.zeros((H, width * n), dtype=np.uint8), [0] * (width * n), []
    for y in range(H):
        kind, data = int(rows[y, 0]), rows[y, 1:].astype(int).tolist()
        if kind > 4:
            raise ValueError("row %d: filter type %d" % (y, kind))
        cur = []
        for i, x in enumerate(data):
            a = cur[i - n] if i >= n else 0
            b = up[i]
            c = up[i - n] if i >= n else 0
            cur.append((x + (0, a, b, (a + b) // 2, _paeth(a, b, c))[kind]) % 256)
        out[y] = cur
        up = cur
        kinds.append(kind)
    return out.reshape(H, width, n), kinds


def decode(data):
    """A PNG file -> {"image": uint8 [H, W, n], "filters": [type per row], "chunks": [kinds], "idat": the payload, "rows": the inflated
    IDAT as uint8 [H, 1 + W * n]}.  Every chunk CRC is checked; 8-bit gray / RGB without interlacing only."""
    data = bytes(data)
    assert data[:8] == PNG_SIGNATURE, "not a PNG"
    at, chunks, idat, ihdr, srgb = 8, [], b"", None, None
    while at < len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and at + 12 + n <= len(data), "truncated chunk %r" % kind
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == (zlib.crc32(kind + body) & 0xFFFFFFFF), "bad CRC in %r" % kind
        chunks.append(kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"sRGB":
            srgb = body
        at += 12 + n
    assert chunks and chunks[0] == b"IHDR" and chunks[-1] == b"IEND" and at == len(data), chunks
    w, h, depth, colour, compression, filt, interlace = ihdr
    assert depth == 8 and colour in (0, 2) and not compression and not filt and not interlace, ihdr
    n = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert raw.size == h * (1 + w * n), "%d bytes of image data, %d expected" % (raw.size, h * (1 + w * n))
    rows = raw.reshape(h, 1 + w * n)
    image, kinds = unfilter(rows, w, n)
    return {"image": image, "filters": kinds, "chunks": chunks, "idat": idat, "rows": rows, "srgb": srgb}


def adler_combine(adler1, adler2, len2):
    adler1, adler2, len2 = int(adler1), int(adler2), int(len2)      # (numpy's 32-bit scalars would wrap)
    a1, b1, a2, b2 = adler1 & 0xffff, adler1 >> 16, adler2 & 0xffff, adler2 >> 16
    return (((b1 + b2 + len2 * (a1 - 1)) % 65521) << 16) | ((a1 + a2 - 1) % 65521)


def stream_of(bodies, adlers, lengths):
    """78 01, the bodies, the combined Adler-32: the IDAT payload"""
    adler = 1
    for a, n in zip(adlers, lengths):
        adler = adler_combine(adler, a, n)
    return b"\x78\x01" + b"".join(bodies) + struct.pack(">I", adler)


# ---------------------------------------------------------------------------------------------------- the test images
def floats_of_bytes(q):
    """fp32 samples whose byte (exposure 1) is q: 0 -> 0.0, k -> the table's entry k - 1 (exactly k entries are <= it)"""
    table = np.concatenate([[np.float32(0)], THRESHOLDS]).astype(np.float32)
    return table[np.asarray(q, dtype=np.int64)]


def edge_values():
    """every table value, the fp32 numbers next below and above it, +-inf, NaN, negatives, -0.0, and the same divided by 2.5"""
    t = THRESHOLDS
    special = np.array([np.inf, -np.inf, np.nan, -1.0, -1e-30, -0.0, 0.0, 1.0, 1e30, 0.5], dtype=np.float32)
    ones = np.concatenate([t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)), special]).astype(np.float32)
    return np.concatenate([ones, (ones / np.float32(2.5)).astype(np.float32)])


def edge_image(height, width, n):
    """[height, width, n] filled with edge_values() over and over (a NaN lands in different channels of different pixels)"""
    return np.resize(edge_values(), (height, width, n)).astype(np.float32)


def all_filters_image(height, width, n, seed=7):
    """uniform random bytes as fp32 samples: at 17 x 21 the rows pick every one of the five filter types"""
    q = np.random.default_rng(seed).integers(0, 256, size=(height, width, n), dtype=np.uint8)
    return floats_of_bytes(q)


def noisy_gradient(height, width, n, seed=11, noise=0.02):
    """a smooth image plus mild noise, like a denoised pass"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    img = np.stack([0.05 + 0.6 * x / max(width, 2) + 0.2 * (c + 1) * y / max(height, 2) for c in range(n)], axis=-1).astype(np.float32)
    return (img + noise * rng.standard_normal(img.shape).astype(np.float32)).astype(np.float32)


_IMAGES = []


def images():
    """[(name, fp32 [H, W, n], exposure, segment_rows)] -- built once, never changed"""
    if _IMAGES:
        return _IMAGES
    n_edge = len(edge_values())
    out = [
        ("edge_rgb", edge_image(-(-n_edge // (21 * 3)) + 1, 21, 3), 1.0, 8),
        ("edge_gray_x2.5", edge_image(-(-n_edge // 21) + 1, 21, 1), 2.5, 16),
        ("filters_rgb_17x21", all_filters_image(17, 21, 3), 1.0, 3),
        ("filters_gray_17x21", all_filters_image(17, 21, 1, seed=8), 1.0, 8),
        ("gradient_rgb_53x67", noisy_gradient(53, 67, 3), 1.0, 16),
        ("gradient_gray_17x21", noisy_gradient(17, 21, 1, seed=12), 1.0, 5),
        ("smooth_rgb_96x128", noisy_gradient(96, 128, 3, seed=13, noise=0.0), 1.0, 24),
        ("one_pixel", np.full((1, 1, 3), 0.18, dtype=np.float32), 1.0, 1),
        ("noise_rgb_64x64", all_filters_image(64, 64, 3, seed=9), 1.0, 16),
        ("constant_rgb_9x16", np.full((9, 16, 3), 0.18, dtype=np.float32), 2.5, 3),
    ]
    _IMAGES.extend(out)
    return _IMAGES


def cut(lengths_total, pieces):
    """`pieces` segment lengths that sum to lengths_total, as even as whole bytes allow, none empty (lengths_total >= pieces)"""
    base, rest = divmod(lengths_total, pieces)
    return [base + (1 if k < rest else 0) for k in range(pieces)]


def byte_jobs():
    """the enumerated inputs of the device deflate (tests/exr_deflate_inputs.py) cut into 2 to 5 segments (fewer where there are fewer bytes)
    -> [(bytes, [segment lengths])]"""
    import exr_deflate_inputs as D
    return [(t, cut(len(t), min(2 + k % 4, len(t)))) for k, (_, t) in enumerate(D.enumerated())]


def job_names():
    """the names of the jobs of tests/png_core_main.cpp, the keys of tests/golden/png_segments.json: the images, then the byte inputs"""
    import exr_deflate_inputs as D
    return ["image " + name for name, _, _, _ in images()] + ["bytes " + name for name, _ in D.enumerated()]


def image_segment_lengths(image, segment_rows):
    row = 1 + image.shape[1] * image.shape[2]
    return [min(segment_rows, image.shape[0] - y0) * row for y0 in range(0, image.shape[0], segment_rows)]


# ---------------------------------------------------------------------------------------------------- tests/png_core_main.cpp
def write_corpus(path, image_jobs, byte_jobs):
    """image_jobs: [(fp32 [H, W, C], n, src_channel, exposure, segment_rows)]; byte_jobs: [(bytes, [segment lengths])]"""
    with open(path, "wb") as f:
        f.write(THRESHOLDS.astype("<f4").tobytes())
        f.write(struct.pack("<I", len(image_jobs) + len(byte_jobs)))
        for plane, n, channels, exposure, segment_rows in image_jobs:
            plane = np.ascontiguousarray(plane, dtype="<f4")
            channels = list(channels) + [0] * (3 - len(channels))
            f.write(struct.pack("<IiiiiiiifI", 0, plane.shape[0], plane.shape[1], plane.shape[2], n, channels[0], channels[1], channels[2], exposure, segment_rows))
            f.write(plane.tobytes())
        for data, lengths in byte_jobs:
            assert sum(lengths) == len(data) and min(lengths) >= 1
            f.write(struct.pack("<III", 1, len(data), len(lengths)) + struct.pack("<%dI" % len(lengths), *lengths) + data)


def read_results(path, count):
    """-> [(filtered bytes (b"" for a byte job), [(status, size, adler, body)])]"""
    buf, at, out = open(path, "rb").read(), 0, []
    for _ in range(count):
        n, = struct.unpack_from("<I", buf, at)
        filtered = buf[at + 4:at + 4 + n]
        at += 4 + n
        segments, = struct.unpack_from("<I", buf, at)
        at += 4
        have = []
        for _ in range(segments):
            status, size, adler = struct.unpack_from("<iiI", buf, at)
            at += 12
            have.append((status, size, adler, buf[at:at + size]))
            at += size
        out.append((filtered, have))
    assert at == len(buf)
    return out


def digest(segments):
    """what tests/golden/png_segments.json records of a job: per segment its status, size, Adler-32 and the SHA-256 of its body"""
    return [{"status": int(s), "size": int(n), "adler": int(a), "sha256": hashlib.sha256(bytes(body)).hexdigest() if s == OK else ""} for s, n, a, body in segments]
