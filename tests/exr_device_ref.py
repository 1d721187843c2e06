"""The device EXR decoder restated in numpy, and the files its tests read (TEST INFRASTRUCTURE ONLY).

reconstruct() is csrc/dd_exr_decode.hip line by line in numpy: the staged bytes of a batch plus the chunk and file tables give the planes and
the non-finite counts.  With openexr.plan_file in front of it, it is the whole device path without a device, so the host half is tested on a
machine without a GPU; the yardstick is always openexr.read_image(path)[..., :channels], compared as uint32 (bit equality).

fixtures() writes every file of the issue's list into a directory; the CPU and the GPU tests walk the same list."""
import os
import struct

import numpy as np

from deepdenoiser_amd import openexr

_SIZE = {0: 4, 1: 2, 2: 4}
_DTYPE = {0: np.dtype("<u4"), 1: np.dtype("<f2"), 2: np.dtype("<f4")}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def reconstruct(staged, chunks, files):
    """staged: uint8 [staged_bytes]; chunks: openexr.CHUNK_DTYPE records; files: [(H, W, C, types, dst_masks)].
    -> ([float32 [H, W, C] plane per file], [non-finite count per file]).  Unwritten samples stay zero."""
    planes = [np.zeros((H, W, C), dtype=np.float32) for H, W, C, _, _ in files]
    counts = [0] * len(files)
    for ck in chunks:
        k, rows, row0, at = int(ck["file"]), int(ck["rows"]), int(ck["row0"]), int(ck["offset"])
        if not 0 <= k < len(files):
            continue
        H, W, C, types, masks = files[k]
        if not (1 <= rows <= 16 and 0 <= row0 <= H - rows):
            continue
        row_bytes = sum(W * _SIZE[t] for t in types)
        n = rows * row_bytes
        n16 = (n + 15) // 16 * 16
        if at < 0 or at % 16 or at > len(staged) - n16:
            continue
        t = staged[at:at + n]
        if ck["coded"]:
            i = np.arange(n)
            s = ((np.cumsum(t.astype(np.int64)) + 128 * (i & 1)) & 0xFF).astype(np.uint8)
            half = (n + 1) // 2
            original = np.empty(n, dtype=np.uint8)
            original[0::2] = s[:half]
            original[1::2] = s[half:]
        else:
            original = np.array(t)
        plane_bits = planes[k].view(np.uint32)
        for r in range(rows):
            p, done = r * row_bytes, set()
            for c, (ptype, mask) in enumerate(zip(types, masks)):
                raw = original[p:p + W * _SIZE[ptype]].view(_DTYPE[ptype])
                p += W * _SIZE[ptype]
                values = raw.view(np.uint32) if ptype == 2 else raw.astype(np.float32).view(np.uint32)
                for d in range(C):
                    if (mask >> d) & 1 and d not in done:
                        done.add(d)
                        plane_bits[row0 + r, :, d] = values
                        counts[k] += int(np.count_nonzero((values & 0x7F800000) == 0x7F800000))
    return planes, counts


def decode_ref(path, channels):
    """plan_file + inflate + reconstruct of one file -> (plane, count, plan)."""
    plan = openexr.plan_file(path, channels)
    staged = np.full(max(plan.staged_bytes, 16), 0xA5, dtype=np.uint8)      # (the padding between chunks is never zero-filled by the decoder)
    plan.inflate(staged)
    planes, counts = reconstruct(staged, plan.chunks, [(plan.height, plan.width, plan.channels, plan.types, plan.dst_masks)])
    return planes[0], counts[0], plan


def chunk_kinds(path):
    """[True where the chunk is coded, False where it is stored raw], from the chunk sizes in the file itself."""
    buf = open(path, "rb").read()
    head, pos = openexr._parse_header(buf)
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    lines = openexr._LINES[head["compression"]]
    row_bytes = sum(W * _SIZE[t] for _, t in head["channels"])
    out = []
    for off in struct.unpack_from("<%dQ" % ((H + lines - 1) // lines), buf, pos):
        y, size = struct.unpack_from("<ii", buf, off)
        out.append(size != min(lines, H - (y - y0)) * row_bytes)
    return out


def move_data_window(path, x0, y0):
    """Re-pack dataWindow and every chunk's y so that the window starts at (x0, y0): the pixels stay the same."""
    buf = bytearray(open(path, "rb").read())
    head, pos = openexr._parse_header(bytes(buf))
    ox0, oy0, ox1, oy1 = head["data_window"]
    at = buf.index(b"dataWindow\0box2i\0") + len(b"dataWindow\0box2i\0") + 4
    struct.pack_into("<4i", buf, at, x0, y0, x0 + (ox1 - ox0), y0 + (oy1 - oy0))
    H = oy1 - oy0 + 1
    lines = openexr._LINES[head["compression"]]
    for off in struct.unpack_from("<%dQ" % ((H + lines - 1) // lines), buf, pos):
        (y,) = struct.unpack_from("<i", buf, off)
        struct.pack_into("<i", buf, off, y - oy0 + y0)
    open(path, "wb").write(bytes(buf))


def smooth(h, w, c, seed=0):
    """A smooth ramp with a little noise in the low mantissa bits: deflates well, does not run-length code."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([0.25 + 0.01 * y + 0.003 * x * (k + 1) for k in range(c)], axis=-1).astype(np.float32)
    return (img * (1 + 1e-6 * rng.standard_normal(img.shape))).astype(np.float32)


def random_finite_bits(rng, shape):
    """float32 of uniformly random bit patterns, the non-finite ones replaced."""
    u = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7F800000) == 0x7F800000] = 0x3F800000
    return u.view(np.float32)


COMPRESSIONS = {"none": openexr.NO_COMPRESSION, "rle": openexr.RLE_COMPRESSION, "zips": openexr.ZIPS_COMPRESSION, "zip": openexr.ZIP_COMPRESSION}
SIZES = ((1, 1), (5, 3), (37, 21), (16, 300))


def _rgb(img):
    return {c: np.ascontiguousarray(img[..., i]) for i, c in enumerate("RGB")}


def raw_in_zip_image():
    img = smooth(37, 21, 3, seed=5)
    img[16:32] = random_finite_bits(np.random.default_rng(6), (16, 21, 3))
    return img


def rle_mixed_image():
    """Rows 0, 3, 4 and 9 hold one value whose even bytes are equal and whose odd bytes are equal (after the byte split the deltas run: the
    row is run-length coded); the others are smooth (stored raw under RLE)."""
    img = smooth(12, 21, 3, seed=7)
    for r, v in ((0, 0x00000000), (3, 0x3F3F3F3F), (4, 0xC1C0C1C0), (9, 0x42424242)):
        img.view(np.uint32)[r] = v
    return img


def fixtures(directory):
    """Writes the files and returns [(id, path, channels)]."""
    os.makedirs(directory, exist_ok=True)
    out = []

    def add(name, chans, channels=3, compression=openexr.ZIP_COMPRESSION):
        path = os.path.join(directory, name + ".exr")
        openexr.write_exr(path, chans, compression)
        out.append((name, path, channels))
        return path
    # ---- compression and size
    for cname, comp in COMPRESSIONS.items():
        for h, w in SIZES:
            add("%s_%dx%d" % (cname, h, w), _rgb(smooth(h, w, 3, seed=h + w)), 3, comp)
        add("%s_1x1_y" % cname, {"Y": np.full((1, 1), 0.375, dtype=np.float32)}, 1, comp)
        big = smooth(20, 1100, 4, seed=11)
        add("%s_20x1100_rgba" % cname, {c: np.ascontiguousarray(big[..., i]) for i, c in enumerate("RGBA")}, 3, comp)
    # ---- a raw chunk inside a ZIP file; coded and raw chunks under RLE
    add("zip_with_raw_chunk", _rgb(raw_in_zip_image()), 3, openexr.ZIP_COMPRESSION)
    add("rle_coded_and_raw", _rgb(rle_mixed_image()), 3, openexr.RLE_COMPRESSION)
    # ---- pixel types
    every_half = np.arange(65536, dtype=np.uint16).view(np.float16).reshape(256, 256)
    add("half_every_pattern", {"Y": every_half}, 1)
    uints = np.array([[0, 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31, 2 ** 32 - 1]], dtype=np.uint32)
    add("uint_roundings", {"Y": uints}, 1, openexr.ZIPS_COMPRESSION)
    rng = np.random.default_rng(21)
    mixed = {"R": rng.standard_normal((9, 13)).astype(np.float16), "G": rng.standard_normal((9, 13)).astype(np.float32),
             "B": rng.integers(0, 2 ** 32, size=(9, 13), dtype=np.uint64).astype(np.uint32)}
    add("mixed_half_float_uint", mixed, 3)
    add("mixed_half_float_uint_none", mixed, 3, openexr.NO_COMPRESSION)
    # ---- channel selection
    img = smooth(7, 9, 4, seed=31)
    add("layer_prefixed", {"ViewLayer.Combined.%s" % c: np.ascontiguousarray(img[..., i]) for i, c in enumerate("RGB")}, 3)
    add("lower_case", {c: np.ascontiguousarray(img[..., i]) for i, c in enumerate("rgb")}, 3)
    add("rgba_alpha_skipped", {c: np.ascontiguousarray(img[..., i]) for i, c in enumerate("RGBA")}, 3)
    add("single_y_one_channel", {"Y": np.ascontiguousarray(img[..., 0])}, 1)
    add("single_y_replicated", {"Y": np.ascontiguousarray(img[..., 1])}, 3)
    add("sorted_b_g_r", _rgb(img[..., :3]), 3)                                   # (stored in name order: B, G, R)
    add("sorted_r_g_b", {"a.R": np.ascontiguousarray(img[..., 0]), "b.G": np.ascontiguousarray(img[..., 1]), "c.B": np.ascontiguousarray(img[..., 2])}, 3)
    add("rgb_first_two", _rgb(img[..., :3]), 2)
    # ---- non-finite samples
    dirty = smooth(19, 10, 3, seed=41)
    dirty[0, 0, 0], dirty[5, 3, 1], dirty[18, 9, 2], dirty[7, 7, 0] = np.nan, np.inf, -np.inf, np.nan
    dirty.view(np.uint32)[7, 7, 0] = 0x7FA12345                                  # a signalling NaN with a payload: the bits are moved
    dirty.view(np.uint32)[8, 1, 2] = 0xFFC00001
    add("nonfinite_float", _rgb(dirty), 3)
    add("nonfinite_float_none", _rgb(dirty), 3, openexr.NO_COMPRESSION)
    dirty_half = smooth(6, 11, 3, seed=43).astype(np.float16)
    dirty_half[0, 1, 0], dirty_half[2, 2, 1], dirty_half[5, 10, 2] = np.nan, np.inf, -np.inf
    add("nonfinite_half", _rgb(dirty_half), 3)
    # ---- a data window that does not start at the origin
    path = add("data_window_moved", _rgb(smooth(37, 21, 3, seed=51)), 3)
    move_data_window(path, 3, -2)
    path = add("data_window_moved_zips", _rgb(smooth(5, 3, 3, seed=52)), 3, openexr.ZIPS_COMPRESSION)
    move_data_window(path, 3, -2)
    return out
