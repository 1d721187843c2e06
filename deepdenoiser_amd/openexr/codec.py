"""The host codec: the container format of the package docstring read and written with numpy and zlib.  No torch, no device library."""
import struct
import zlib

import numpy as np

MAGIC = 20000630
NO_COMPRESSION, RLE_COMPRESSION, ZIPS_COMPRESSION, ZIP_COMPRESSION = 0, 1, 2, 3
_CODEC_NAMES = {0: "NONE", 1: "RLE", 2: "ZIPS", 3: "ZIP", 4: "PIZ", 5: "PXR24", 6: "B44", 7: "B44A", 8: "DWAA", 9: "DWAB"}
_LINES = {NO_COMPRESSION: 1, RLE_COMPRESSION: 1, ZIPS_COMPRESSION: 1, ZIP_COMPRESSION: 16}
_PIXEL = {0: np.dtype("<u4"), 1: np.dtype("<f2"), 2: np.dtype("<f4")}
_PIXEL_CODE = {np.dtype("uint32"): 0, np.dtype("float16"): 1, np.dtype("float32"): 2}


class ExrError(IOError):
    pass


# ---------------------------------------------------------------------------------------------------- chunk codecs
def _undo_predictor_and_interleave(t):
    """bytes after inflate / run-length decoding -> original chunk bytes"""
    d = np.frombuffer(t, dtype=np.uint8).astype(np.int64)
    if d.size == 0:
        return b""
    d[1:] -= 128
    s = (np.cumsum(d) & 0xFF).astype(np.uint8)
    half = (s.size + 1) // 2
    out = np.empty(s.size, dtype=np.uint8)
    out[0::2] = s[:half]
    out[1::2] = s[half:]
    return out.tobytes()


def _interleave_and_predict(raw):
    """original chunk bytes -> bytes handed to deflate / the run-length coder"""
    b = np.frombuffer(raw, dtype=np.uint8)
    if b.size == 0:
        return b""
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int64)
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + 128
    return (d & 0xFF).astype(np.uint8).tobytes()


def _rle_decode(data, expected):
    out, pos, n = bytearray(), 0, len(data)
    while pos < n:
        count = data[pos] - 256 if data[pos] > 127 else data[pos]
        pos += 1
        if count < 0:
            out += data[pos:pos - count]
            pos -= count
        else:
            out += bytes([data[pos]]) * (count + 1)
            pos += 1
    if len(out) != expected:
        raise ExrError("run-length coded chunk expands to %d bytes, expected %d" % (len(out), expected))
    return bytes(out)


def _rle_encode(data):
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i + 1
        while j < n and data[j] == data[i] and j - i < 128:
            j += 1
        if j - i >= 3:                                     # a run
            out += bytes([j - i - 1, data[i]])
            i = j
            continue
        j = i                                               # literals up to the next run of 3 (or 127 bytes)
        while j < n and j - i < 127 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([256 - (j - i)]) + data[i:j]
        i = j
    return bytes(out)


def _decode_chunk(data, compression, expected):
    if len(data) == expected:                               # stored raw because coding did not shrink it (or NO_COMPRESSION)
        return data
    if compression in (ZIP_COMPRESSION, ZIPS_COMPRESSION):
        t = zlib.decompress(data)
    elif compression == RLE_COMPRESSION:
        t = _rle_decode(data, expected)
    else:
        raise ExrError("chunk of %d bytes where %d are expected" % (len(data), expected))
    if len(t) != expected:
        raise ExrError("chunk expands to %d bytes, expected %d" % (len(t), expected))
    return _undo_predictor_and_interleave(t)


# ---------------------------------------------------------------------------------------------------- header
def _cstr(buf, pos):
    end = buf.index(b"\0", pos)
    return buf[pos:end].decode("latin-1"), end + 1


def _parse_header(buf):
    if len(buf) < 8:
        raise ExrError("not an OpenEXR file (too short)")
    magic, version = struct.unpack_from("<ii", buf, 0)
    if magic != MAGIC:
        raise ExrError("not an OpenEXR file (magic %d)" % magic)
    if version & 0xFF != 2:
        raise ExrError("OpenEXR format version %d is not supported" % (version & 0xFF))
    for bit, what in ((0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")):
        if version & bit:
            raise ExrError("%s OpenEXR files are not supported (single-part scan-line files only)" % what)
    pos, attrs = 8, {}
    while True:
        name, pos = _cstr(buf, pos)
        if not name:
            break
        kind, pos = _cstr(buf, pos)
        (size,) = struct.unpack_from("<i", buf, pos)
        pos += 4
        attrs[name] = (kind, buf[pos:pos + size])
        pos += size
    for need in ("channels", "compression", "dataWindow"):
        if need not in attrs:
            raise ExrError("header lacks the %s attribute" % need)
    channels, cp, cl = [], 0, attrs["channels"][1]
    while cl[cp] != 0:
        cname, cp = _cstr(cl, cp)
        ptype, _plinear, xs, ys = struct.unpack_from("<iB3xii", cl, cp)
        cp += 16
        if ptype not in _PIXEL:
            raise ExrError("channel %s: unknown pixel type %d" % (cname, ptype))
        if xs != 1 or ys != 1:
            raise ExrError("channel %s is subsampled (%d x %d); not supported" % (cname, xs, ys))
        channels.append((cname, ptype))
    compression = attrs["compression"][1][0]
    if compression not in _LINES:
        raise ExrError("compression %s is not supported (NONE, RLE, ZIPS, ZIP are)" % _CODEC_NAMES.get(compression, compression))
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    return {"channels": channels, "compression": compression, "data_window": (x0, y0, x1, y1), "attributes": attrs}, pos


def _walk(path, buf):
    """The one walk over a file's bytes, for the host reader and for the device decoder's plan: yields the parsed header first, then per
    chunk (row0, rows, a view of the chunk's data, the bytes it expands to), each chunk checked when it is reached.  The offset table is
    checked only when the first chunk is asked for, so the caller's own checks of the header come before it."""
    try:
        head, pos = _parse_header(buf)
    except (ValueError, struct.error, IndexError) as e:
        raise ExrError("%s: truncated or malformed header (%s)" % (path, e))
    yield head
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    lines = _LINES[head["compression"]]
    n_chunks = (H + lines - 1) // lines
    if pos + 8 * n_chunks > len(buf):
        raise ExrError("%s: truncated offset table" % path)
    row_bytes = sum(W * _PIXEL[t].itemsize for _, t in head["channels"])
    view = memoryview(buf)
    for off in struct.unpack_from("<%dQ" % n_chunks, buf, pos):
        if off + 8 > len(buf):
            raise ExrError("%s: chunk offset %d past the end of the file" % (path, off))
        y, size = struct.unpack_from("<ii", buf, off)
        r0 = y - y0
        nl = min(lines, H - r0)
        if r0 < 0 or nl <= 0 or off + 8 + size > len(buf):
            raise ExrError("%s: bad chunk (y %d, %d bytes)" % (path, y, size))
        yield r0, nl, view[off + 8:off + 8 + size], nl * row_bytes


def read_exr(path):
    """-> ({channel name: [H,W] array (float32 for HALF/FLOAT, uint32 for UINT)}, header dict) of the file's data window."""
    with open(path, "rb") as f:
        buf = f.read()
    walk = _walk(path, buf)
    head = next(walk)
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    chans = head["channels"]                                  # stored sorted by name; the chunk layout follows this order
    planes = {name: np.empty((H, W), dtype=_PIXEL[t]) for name, t in chans}
    for r0, nl, data, expected in walk:
        raw = _decode_chunk(bytes(data), head["compression"], expected)
        p = 0
        for r in range(r0, r0 + nl):
            for name, t in chans:
                planes[name][r] = np.frombuffer(raw, dtype=_PIXEL[t], count=W, offset=p)
                p += W * _PIXEL[t].itemsize
    out = {name: (planes[name] if t == 0 else planes[name].astype(np.float32)) for name, t in chans}
    return out, head


def image_size(path):
    """(height, width) of the file's data window from its header alone (the first 64 KiB; the whole file when the header is longer)."""
    with open(path, "rb") as f:
        buf = f.read(1 << 16)
        try:
            head, _ = _parse_header(buf)
        except (ValueError, IndexError, struct.error):
            head, _ = _parse_header(buf + f.read())
    x0, y0, x1, y1 = head["data_window"]
    return y1 - y0 + 1, x1 - x0 + 1


def read_image(path):
    """What OpenEXRDirectory._load_exr returns (OpenEXRDirectory.py:125-151): float32 [H,W,3] in R,G,B order.  Channel names may carry a
    layer prefix ("ViewLayer.Combined.R"); a file with a single channel (Alpha, Depth written as Y / A / Z / V) is replicated to 3."""
    chans, _ = read_exr(path)
    by_suffix = {}
    for name in chans:
        by_suffix.setdefault(name.rsplit(".", 1)[-1].upper(), name)
    if all(c in by_suffix for c in "RGB"):
        return np.stack([chans[by_suffix[c]] for c in "RGB"], axis=-1).astype(np.float32)
    if len(chans) == 1:
        (only,) = chans.values()
        return np.repeat(only.astype(np.float32)[..., None], 3, axis=-1)
    raise ExrError("%s: no R, G, B channels among %s" % (path, sorted(chans)))


# ---------------------------------------------------------------------------------------------------- writer
def _attr(name, kind, value):
    return name.encode("latin-1") + b"\0" + kind.encode("latin-1") + b"\0" + struct.pack("<i", len(value)) + value


def _header(names, types, compression, width, height):
    """The bytes in front of the offset table, for channels `names` (sorted) with their pixel type codes."""
    chlist = b"".join(n.encode("latin-1") + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in zip(names, types)) + b"\0"
    box = struct.pack("<4i", 0, 0, width - 1, height - 1)
    header = struct.pack("<ii", MAGIC, 2)
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    header += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0")
    header += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0))
    return header + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"


def write_exr(path, channels, compression=ZIP_COMPRESSION):
    """{channel name: [H,W] float32 / float16 / uint32 array} -> single-part scan-line file."""
    if compression not in _LINES:
        raise ExrError("cannot write compression %s" % _CODEC_NAMES.get(compression, compression))
    names = sorted(channels)
    arrs = [np.asarray(channels[n]) for n in names]
    H, W = arrs[0].shape
    for n, a in zip(names, arrs):
        if a.shape != (H, W) or a.dtype not in _PIXEL_CODE:
            raise ExrError("channel %s: need a [%d,%d] float32 / float16 / uint32 array, got %s %s" % (n, H, W, a.shape, a.dtype))
    header = _header(names, [_PIXEL_CODE[a.dtype] for a in arrs], compression, W, H)
    lines = _LINES[compression]
    chunks = []
    for r0 in range(0, H, lines):
        raw = b"".join(a[r].astype(a.dtype.newbyteorder("<"), copy=False).tobytes() for r in range(r0, min(H, r0 + lines)) for a in arrs)
        data = raw
        if compression in (ZIP_COMPRESSION, ZIPS_COMPRESSION):
            data = zlib.compress(_interleave_and_predict(raw))
        elif compression == RLE_COMPRESSION:
            data = _rle_encode(_interleave_and_predict(raw))
        if len(data) >= len(raw):
            data = raw
        chunks.append(struct.pack("<ii", r0, len(data)) + data)
    pos = len(header) + 8 * len(chunks)
    table = b""
    for c in chunks:
        table += struct.pack("<Q", pos)
        pos += len(c)
    with open(path, "wb") as f:
        f.write(header + table + b"".join(chunks))


def _image_channels(shape, who="the writer"):
    """The channel names of an image: [H,W,3] is R, G, B; [H,W] is Y."""
    if len(shape) == 2:
        return ["Y"]
    if len(shape) != 3 or shape[2] != 3:
        raise ExrError("%s takes [H,W,3] or [H,W], got %s" % (who, tuple(shape)))
    return ["R", "G", "B"]


def _image_planes(image, who="the writer"):
    """[H,W,3] or [H,W] array -> the {channel name: [H,W] plane} write_exr takes"""
    names = _image_channels(image.shape, who)
    return {"Y": image} if image.ndim == 2 else {c: np.ascontiguousarray(image[..., i]) for i, c in enumerate(names)}


def write_image(path, image, compression=ZIP_COMPRESSION):
    """[H,W,3] (R,G,B) or [H,W] (written as Y) float array -> .exr with FLOAT channels."""
    return write_exr(path, _image_planes(np.asarray(image, dtype=np.float32), "write_image"), compression)
