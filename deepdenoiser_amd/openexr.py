"""OpenEXR frames without OpenCV / the OpenEXR library: the render-pass images either side of the inference path
(TensorFlow/OpenEXRDirectory.py:54-151 loads one .exr per render pass through cv2.imdecode and hands RGB float32 to Prediction.py:223-252;
SURVEY 8f rank 4).

PARITY UNPINNED: neither OpenCV nor the OpenEXR library is installed and the reference ships no image, so nothing here has been checked
against a file written by Blender.  The container format is restated from the published "OpenEXR File Layout" document:

    int32 magic 20000630 | int32 version (low byte 2; bit 0x200 tiled, 0x800 deep, 0x1000 multi-part)
    header    = attributes (name\\0 type\\0 int32 size, value) ... \\0
                channels (chlist: name\\0 int32 type{0 uint,1 half,2 float} uint8 pLinear 3 reserved int32 xSampling int32 ySampling ... \\0),
                compression (uint8), dataWindow / displayWindow (box2i), lineOrder, pixelAspectRatio, screenWindowCenter, screenWindowWidth
    uint64 offset per chunk, chunks of 1 (none, RLE, ZIPS) or 16 (ZIP) scan lines:
    chunk     = int32 y | int32 size | data;   data = per scan line, per channel in name order, one row of that channel's samples
    ZIP / ZIPS / RLE transform the chunk bytes first: split into even and odd bytes (first half, second half), then byte deltas
    (t[i] - t[i-1] + 128), then deflate (or run-length code); a chunk that would not shrink is stored raw.

Supported: single-part scan-line files, compression NONE / RLE / ZIPS / ZIP (Blender's default), UINT / HALF / FLOAT channels without
subsampling.  Tiled, deep, multi-part files and the PIZ / PXR24 / B44 / DWA codecs raise ExrError naming what was found.
"""
import os
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


def read_exr(path):
    """-> ({channel name: [H,W] array (float32 for HALF/FLOAT, uint32 for UINT)}, header dict) of the file's data window."""
    with open(path, "rb") as f:
        buf = f.read()
    try:
        head, pos = _parse_header(buf)
    except (ValueError, struct.error, IndexError) as e:
        raise ExrError("%s: truncated or malformed header (%s)" % (path, e))
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    chans = head["channels"]                                  # stored sorted by name; the chunk layout follows this order
    lines = _LINES[head["compression"]]
    n_chunks = (H + lines - 1) // lines
    if pos + 8 * n_chunks > len(buf):
        raise ExrError("%s: truncated offset table" % path)
    offsets = struct.unpack_from("<%dQ" % n_chunks, buf, pos)
    row_bytes = sum(W * _PIXEL[t].itemsize for _, t in chans)
    planes = {name: np.empty((H, W), dtype=_PIXEL[t]) for name, t in chans}
    for off in offsets:
        if off + 8 > len(buf):
            raise ExrError("%s: chunk offset %d past the end of the file" % (path, off))
        y, size = struct.unpack_from("<ii", buf, off)
        r0 = y - y0
        nl = min(lines, H - r0)
        if r0 < 0 or nl <= 0 or off + 8 + size > len(buf):
            raise ExrError("%s: bad chunk (y %d, %d bytes)" % (path, y, size))
        raw = _decode_chunk(buf[off + 8:off + 8 + size], head["compression"], nl * row_bytes)
        p = 0
        for r in range(r0, r0 + nl):
            for name, t in chans:
                n = W * _PIXEL[t].itemsize
                planes[name][r] = np.frombuffer(raw, dtype=_PIXEL[t], count=W, offset=p)
                p += n
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


def write_exr(path, channels, compression=ZIP_COMPRESSION):
    """{channel name: [H,W] float32 / float16 / uint32 array} -> single-part scan-line file."""
    if compression not in _LINES:
        raise ExrError("cannot write compression %s" % _CODEC_NAMES.get(compression, compression))
    names = sorted(channels)
    arrs = [np.asarray(channels[n]) for n in names]
    H, W = arrs[0].shape
    chlist = b""
    for n, a in zip(names, arrs):
        if a.shape != (H, W) or a.dtype not in _PIXEL_CODE:
            raise ExrError("channel %s: need a [%d,%d] float32 / float16 / uint32 array, got %s %s" % (n, H, W, a.shape, a.dtype))
        chlist += n.encode("latin-1") + b"\0" + struct.pack("<iB3xii", _PIXEL_CODE[a.dtype], 0, 1, 1)
    chlist += b"\0"
    box = struct.pack("<4i", 0, 0, W - 1, H - 1)
    header = struct.pack("<ii", MAGIC, 2)
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    header += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0")
    header += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0))
    header += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
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


def write_image(path, image, compression=ZIP_COMPRESSION):
    """[H,W,3] (R,G,B) or [H,W] (written as Y) float array -> .exr with FLOAT channels."""
    image = np.asarray(image, dtype=np.float32)
    if image.ndim == 2:
        return write_exr(path, {"Y": image}, compression)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ExrError("write_image takes [H,W,3] or [H,W], got %s" % (image.shape,))
    return write_exr(path, {c: np.ascontiguousarray(image[..., i]) for i, c in enumerate("RGB")}, compression)


# ---------------------------------------------------------------------------------------------------- decode on the device
# The host keeps the header, the offset table and inflate (zlib releases the GIL); the predictor, the byte split, the row / channel split and
# the conversion to fp32 are one dd_exr_reconstruct launch over the staged bytes of many files (csrc/dd_exr_decode.hip).  With
# inflate="device" the host keeps only the header, the offset table and the run-length decode: one dd_exr_inflate launch per batch
# (csrc/dd_exr_inflate.hip) expands the zlib streams of the ZIP / ZIPS chunks into the staged buffer on the device.
_STAGE_ALIGN = 16                                               # a chunk's offset in the staged buffer; it owns the bytes up to the next multiple
CHUNK_DTYPE = np.dtype([("offset", "<i8"), ("file", "<i4"), ("row0", "<i4"), ("rows", "<i4"), ("coded", "<i4")])      # dd_exr_chunk
FILE_DTYPE = np.dtype([("dst", "<u8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("n_channels", "<i4"), ("type", "<i4", (8,)),
                       ("dst_mask", "<u4", (8,))])                                                                       # dd_exr_file
MAX_FILE_CHANNELS = 8                                           # DD_EXR_MAX_CHANNELS
STREAM_DTYPE = np.dtype([("src_offset", "<i8"), ("dst_offset", "<i8"), ("src_bytes", "<i4"), ("dst_bytes", "<i4")])      # dd_exr_stream
MAX_STREAM_BYTES = 1 << 30                                      # dd_exr_inflate refuses a stream that expands to more


def _align(n):
    return (n + _STAGE_ALIGN - 1) // _STAGE_ALIGN * _STAGE_ALIGN


class FilePlan:
    """What plan_file found in one file.  height, width, channels: the plane [height, width, channels] the file decodes to; types /
    dst_masks: per file channel (header order) its pixel type and the set of plane channels it is written to (bit d = channel d);
    chunks: CHUNK_DTYPE records with offsets relative to the file's staged bytes (`file` left 0); staged_bytes: how many there are;
    pieces: per chunk (the chunk's bytes in the file, coded flag, bytes after inflate)."""

    def __init__(self, path, height, width, channels, types, dst_masks, compression, chunks, staged_bytes, pieces):
        self.path, self.height, self.width, self.channels, self.types, self.dst_masks = path, height, width, channels, types, dst_masks
        self.compression, self.chunks, self.staged_bytes, self.pieces = compression, chunks, staged_bytes, pieces
        self._source = None

    def inflate(self, out):
        """Write the post-inflate bytes of every chunk into `out` (a uint8 array of at least staged_bytes) at the chunks' offsets: a coded
        chunk as deflate / the run-length coder saw it, a raw one as it is.  Raises what read_exr raises for a chunk of the wrong size."""
        for record, (data, coded, expected) in zip(self.chunks, self.pieces):
            if not coded:
                t = data
            elif self.compression == RLE_COMPRESSION:
                t = _rle_decode(bytes(data), expected)
            else:
                t = zlib.decompress(data)
                if len(t) != expected:
                    raise ExrError("chunk expands to %d bytes, expected %d" % (len(t), expected))
            at = int(record["offset"])
            out[at:at + expected] = np.frombuffer(t, dtype=np.uint8)


    def source_layout(self):
        """What inflate="device" uploads of this file instead of its inflated image -> (source_bytes, streams, runs, places, refused).
        The zlib stream of every coded ZIP / ZIPS chunk is packed as it is in the file: `streams` are STREAM_DTYPE records, src_offset
        relative to the file's source bytes, dst_offset to its staged bytes.  Every other chunk -- stored raw, or run-length coded (the host
        keeps _rle_decode) -- is `plain`: its post-inflate bytes go into the source bytes, and a run of consecutive plain chunks is laid out
        there exactly as in the staged image (16-byte aligned pieces), so that ONE device copy per run moves it to its place: `runs` are
        (source offset, staged offset, bytes).  places: per chunk its offset in the source bytes.  refused: a stream dd_exr_inflate does not
        take (no bytes, or more than MAX_STREAM_BYTES to write); such a file is left to the host path."""
        if self._source is None:
            zipped = self.compression in (ZIP_COMPRESSION, ZIPS_COMPRESSION)
            streams, runs, places, at, refused, plain_before = [], [], [], 0, False, False
            for record, (data, coded, expected) in zip(self.chunks, self.pieces):
                dst = int(record["offset"])
                if coded and zipped:
                    refused = refused or len(data) < 1 or expected > MAX_STREAM_BYTES
                    places.append(at)
                    streams.append((at, dst, len(data), expected))
                    at += len(data)
                    plain_before = False
                else:
                    if not plain_before:
                        at = _align(at)
                        runs.append([at, dst, 0])
                    places.append(at)
                    runs[-1][2] += _align(expected)
                    at += _align(expected)
                    plain_before = True
            table = np.zeros(len(streams), dtype=STREAM_DTYPE)
            if streams and not refused:
                table[:] = streams
            self._source = (at, table, [tuple(r) for r in runs], places, refused)
        return self._source

    def fill_source(self, out):
        """Write the source bytes of source_layout() into `out` (a uint8 array of at least that many): copies, and the run-length decode.
        Raises what inflate() raises for a run-length coded chunk of the wrong size."""
        zipped = self.compression in (ZIP_COMPRESSION, ZIPS_COMPRESSION)
        for at, (data, coded, expected) in zip(self.source_layout()[3], self.pieces):
            t = _rle_decode(bytes(data), expected) if coded and not zipped else data
            out[at:at + len(t)] = np.frombuffer(t, dtype=np.uint8)


def _batch_layout(plans):
    """the arithmetic of pack_batch: where everything lies"""
    source_bases, staged_bases, source_at, staged_at = [], [], 0, 0
    for p in plans:
        source_bases.append(source_at)
        staged_bases.append(staged_at)
        source_at = _align(source_at + p.source_layout()[0])
        staged_at += p.staged_bytes
    n_streams = sum(len(p.source_layout()[1]) for p in plans)
    n_chunks = sum(len(p.chunks) for p in plans)
    layout = {"source_bases": source_bases, "staged_bases": staged_bases, "source_bytes": max(source_at, _STAGE_ALIGN),
              "staged_bytes": max(staged_at, _STAGE_ALIGN), "n_streams": n_streams, "n_chunks": n_chunks}
    layout["streams_at"] = _align(layout["source_bytes"])
    layout["chunks_at"] = _align(layout["streams_at"] + n_streams * STREAM_DTYPE.itemsize)
    layout["files_at"] = _align(layout["chunks_at"] + n_chunks * CHUNK_DTYPE.itemsize)
    layout["total"] = layout["files_at"] + len(plans) * FILE_DTYPE.itemsize
    layout["runs"] = [(src + sb, dst + db, n) for p, sb, db in zip(plans, source_bases, staged_bases) for src, dst, n in p.source_layout()[2]]
    layout["owners"] = [k for k, p in enumerate(plans) for _ in range(len(p.source_layout()[1]))]
    return layout


def pack_batch(plans):
    """The upload buffer of one batch of inflate="device", in plain numpy (DeviceDecoder lays its pinned buffer out the same way):
    source bytes of every file | stream table | chunk table.  -> (buffer uint8, layout) with layout = {"source_bases", "staged_bases",
    "source_bytes", "staged_bytes", "streams_at", "n_streams", "chunks_at", "n_chunks", "files_at", "total", "runs": [(source offset,
    staged offset, bytes)] of the whole batch, "owners": per stream the index of its plan}.  The file table's place is reserved; its rows hold
    device pointers and are written by the decoder."""
    layout = _batch_layout(plans)
    buffer = np.zeros(layout["total"], dtype=np.uint8)
    fill_batch_tables(buffer, layout, plans)
    for p, base in zip(plans, layout["source_bases"]):
        p.fill_source(buffer[base:base + p.source_layout()[0]])
    return buffer, layout


def fill_batch_tables(buffer, layout, plans):
    """The stream and the chunk table of pack_batch's layout, written into `buffer`: offsets made absolute, a chunk's `file` the index of
    its plan."""
    streams = buffer[layout["streams_at"]:layout["streams_at"] + layout["n_streams"] * STREAM_DTYPE.itemsize].view(STREAM_DTYPE)
    chunks = buffer[layout["chunks_at"]:layout["chunks_at"] + layout["n_chunks"] * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
    ns = nc = 0
    for slot, (p, source_base, staged_base) in enumerate(zip(plans, layout["source_bases"], layout["staged_bases"])):
        table = p.source_layout()[1]
        part = streams[ns:ns + len(table)]
        part[:] = table
        part["src_offset"] += source_base
        part["dst_offset"] += staged_base
        ns += len(table)
        part = chunks[nc:nc + len(p.chunks)]
        part[:] = p.chunks
        part["offset"] += staged_base
        part["file"] = slot
        nc += len(p.chunks)
    return streams, chunks


def _destination_masks(path, names, channels):
    """read_image's channel choice as one destination set per file channel: R, G, B by the case-insensitive suffix after the last '.', else the
    single channel replicated, then [..., :channels]."""
    by_suffix = {}
    for k, name in enumerate(names):
        by_suffix.setdefault(name.rsplit(".", 1)[-1].upper(), k)
    masks = [0] * len(names)
    if all(c in by_suffix for c in "RGB"):
        for d, c in enumerate("RGB"[:channels]):
            masks[by_suffix[c]] |= 1 << d
    elif len(names) == 1:
        masks[0] = (1 << channels) - 1
    else:
        raise ExrError("%s: no R, G, B channels among %s" % (path, sorted(set(names))))
    return masks


def plan_file(path, channels=3):
    """The host half of a device decode of `path` into the plane read_image(path)[..., :channels]: header, offset table and chunk checks of
    read_exr (the same ExrError texts), no inflate yet and no device.  -> FilePlan."""
    if channels < 1:
        raise ValueError("channels=%d" % channels)
    channels = min(int(channels), 3)
    with open(path, "rb") as f:
        buf = f.read()
    try:
        head, pos = _parse_header(buf)
    except (ValueError, struct.error, IndexError) as e:
        raise ExrError("%s: truncated or malformed header (%s)" % (path, e))
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    if W < 1 or H < 1:
        raise ExrError("%s: empty data window (%d x %d)" % (path, W, H))
    chans = head["channels"]
    if len(chans) > MAX_FILE_CHANNELS:
        raise ExrError("%s: %d channels; the device decoder takes at most %d" % (path, len(chans), MAX_FILE_CHANNELS))
    compression = head["compression"]
    lines = _LINES[compression]
    n_chunks = (H + lines - 1) // lines
    if pos + 8 * n_chunks > len(buf):
        raise ExrError("%s: truncated offset table" % path)
    offsets = struct.unpack_from("<%dQ" % n_chunks, buf, pos)
    row_bytes = sum(W * _PIXEL[t].itemsize for _, t in chans)
    view = memoryview(buf)
    records, pieces, at = np.zeros(n_chunks, dtype=CHUNK_DTYPE), [], 0
    for k, off in enumerate(offsets):
        if off + 8 > len(buf):
            raise ExrError("%s: chunk offset %d past the end of the file" % (path, off))
        y, size = struct.unpack_from("<ii", buf, off)
        r0 = y - y0
        nl = min(lines, H - r0)
        if r0 < 0 or nl <= 0 or off + 8 + size > len(buf):
            raise ExrError("%s: bad chunk (y %d, %d bytes)" % (path, y, size))
        expected = nl * row_bytes
        coded = size != expected                                # (as _decode_chunk: a chunk of the full size is stored raw)
        if coded and compression == NO_COMPRESSION:
            raise ExrError("chunk of %d bytes where %d are expected" % (size, expected))
        records[k] = (at, 0, r0, nl, int(coded))
        pieces.append((view[off + 8:off + 8 + size], coded, expected))
        at += _align(expected)
    masks = _destination_masks(path, [name for name, _ in chans], channels)
    return FilePlan(path, H, W, channels, [t for _, t in chans], masks, compression, records, at, pieces)


class DeviceDecoder:
    """EXR files to fp32 device planes, bit-identical to read_image(path)[..., :channels]: the host inflates on `threads` threads (at most 16)
    into a ring of two pinned buffers, each batch of files is uploaded once and rebuilt by one dd_exr_reconstruct launch, and the inflate of a
    batch overlaps the upload and the launch of the one before.  A batch holds files whose staged bytes stay under `max_staged_bytes` (a
    larger file goes alone).
    inflate="device": the host only reads the files.  A batch's pinned buffer holds the zlib streams of the coded ZIP / ZIPS chunks as they
    are in the files, the bytes of raw chunks and the run-length decoded bytes of RLE chunks (FilePlan.source_layout), the stream table and
    the two tables of before: about the size of the files, not of the planes.  After the one upload, one dd_exr_inflate launch expands every
    stream into a device-only staged buffer, one device copy per run of consecutive raw / RLE chunks puts those in place, and the
    dd_exr_reconstruct launch follows on the same stream.  The per-stream statuses are read with the counts, in the one synchronisation at
    the end; a file with a stream that is not OK is redone through the host path (`host_fallbacks` counts them), so a corrupt file raises
    what inflate="host" raises and a stream the device refused but zlib accepts still decodes."""
    RING = 2
    time_launches = False                                       # measurements: keep (start, end) events around every launch in `events`
                                                                # (and around every dd_exr_inflate launch in `inflate_events`)

    def __init__(self, device, max_staged_bytes=256 << 20, threads=4, inflate="host"):
        import torch
        self.device = torch.device(device)
        if inflate not in ("host", "device"):
            raise ValueError("inflate=%r (host or device)" % (inflate,))
        if self.device.type != "cuda":
            raise ValueError("EXR files are decoded on a GPU: %s is none" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_staged_bytes = max(int(max_staged_bytes), _STAGE_ALIGN)
        self.threads = max(1, min(int(threads), 16))
        self._pinned = [None] * self.RING                       # [pinned uint8 tensor, the event after its upload]
        self._staged = None                                     # the device copy; batches follow one another on one stream
        self._image = None                                      # inflate="device": the staged image, never on the host
        self.inflate = inflate
        self.launches = 0
        self.inflate_launches = 0
        self.host_fallbacks = 0                                 # files redone on the host because a stream's status was not OK
        self.uploaded_bytes = 0
        self.inflate_seconds = 0.0                              # wall time decode() spent waiting for the host jobs (inflate, or copies + RLE)
        self.events = []
        self.inflate_events = []

    def _buffers(self, slot, nbytes, image_bytes=0):
        import torch
        if image_bytes and (self._image is None or self._image.numel() < image_bytes):
            self._image = torch.empty(image_bytes, dtype=torch.uint8, device=self.device)
        entry = self._pinned[slot]
        if entry is not None and entry[1] is not None:
            entry[1].synchronize()                              # (the upload out of this buffer, RING batches ago)
        if entry is None or entry[0].numel() < nbytes:
            entry = self._pinned[slot] = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), None]
        if self._staged is None or self._staged.numel() < nbytes:
            self._staged = torch.empty(nbytes, dtype=torch.uint8, device=self.device)      # (the caching allocator keeps the old one alive for
        return entry                                                                      #  the launches that still read it)

    def release(self):
        """Give the pinned ring and the device staging buffer back (the counters stay)."""
        import torch
        torch.cuda.synchronize(self.device)
        self._pinned, self._staged, self._image = [None] * self.RING, None, None

    def _on_host(self, lib, L, plan, stream):
        """One file through the host path on its own: plan.inflate, an upload and a dd_exr_reconstruct launch into a fresh plane with a
        fresh count -> (plane, count).  Raises what plan.inflate raises."""
        import torch
        n = len(plan.chunks)
        chunks_at = _align(max(plan.staged_bytes, _STAGE_ALIGN))
        files_at = _align(chunks_at + n * CHUNK_DTYPE.itemsize)
        host = np.zeros(files_at + FILE_DTYPE.itemsize, dtype=np.uint8)
        plan.inflate(host[:plan.staged_bytes])
        plane = torch.empty((plan.height, plan.width, plan.channels), dtype=torch.float32, device=self.device)
        chunk_table = host[chunks_at:chunks_at + n * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
        chunk_table[:] = plan.chunks
        row = host[files_at:].view(FILE_DTYPE)[0]
        row["dst"], row["H"], row["W"], row["C"], row["n_channels"] = plane.data_ptr(), plan.height, plan.width, plan.channels, len(plan.types)
        row["type"][:len(plan.types)] = plan.types
        row["dst_mask"][:len(plan.types)] = plan.dst_masks
        dev = torch.from_numpy(host).to(self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        L.check(lib.dd_exr_reconstruct(host[chunks_at:].ctypes.data, dev.data_ptr() + chunks_at, n, host[files_at:].ctypes.data,
                                       dev.data_ptr() + files_at, 1, dev.data_ptr(), chunks_at, count.data_ptr(), stream.cuda_stream))
        self.launches += 1
        return plane, int(count.item())

    def _inflate_batch(self, lib, L, pool, stream, slot, batch, plans, results, planes):
        """One batch of inflate="device" -> (files in table order, their counts on the device, per stream the file it belongs to, the
        statuses on the device), or None when no file of the batch is left."""
        import time

        import torch
        t0 = time.perf_counter()
        failed = set()
        live = [k for k in batch if not plans[k].source_layout()[4]]      # (a refused file is redone on the host with the failed ones)
        layout = None
        while live:
            layout_plans = [plans[k] for k in live]
            layout = _batch_layout(layout_plans)
            entry = self._buffers(slot, layout["total"], layout["staged_bytes"])
            host = entry[0].numpy()
            jobs = [pool.submit(p.fill_source, host[base:base + p.source_layout()[0]]) for p, base in zip(layout_plans, layout["source_bases"])]
            bad = set()
            for k, job in zip(live, jobs):
                try:
                    job.result()
                except ExrError as e:
                    results[k] = e
                    bad.add(k)
            if not bad:
                break
            failed |= bad                                           # (a run-length coded chunk of the wrong size: lay the batch out without the file)
            live = [k for k in live if k not in bad]
        self.inflate_seconds += time.perf_counter() - t0
        if not live:
            return None
        total, staged_bytes = layout["total"], layout["staged_bytes"]
        streams, _ = fill_batch_tables(host, layout, layout_plans)
        file_table = host[layout["files_at"]:total].view(FILE_DTYPE)
        file_table[:] = np.zeros((), dtype=FILE_DTYPE)
        for slot_in_table, k in enumerate(live):
            p = plans[k]
            planes[k] = torch.empty((p.height, p.width, p.channels), dtype=torch.float32, device=self.device)
            row = file_table[slot_in_table]
            row["dst"], row["H"], row["W"], row["C"], row["n_channels"] = planes[k].data_ptr(), p.height, p.width, p.channels, len(p.types)
            row["type"][:len(p.types)] = p.types
            row["dst_mask"][:len(p.types)] = p.dst_masks
        dev, image = self._staged[:total], self._image[:staged_bytes]
        dev.copy_(entry[0][:total], non_blocking=True)
        self.uploaded_bytes += total
        entry[1] = torch.cuda.Event()
        entry[1].record(stream)
        n_streams = layout["n_streams"]
        statuses = torch.empty(n_streams, dtype=torch.int32, device=self.device)
        if n_streams:
            if self.time_launches:
                self.inflate_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                self.inflate_events[-1][0].record(stream)
            L.check(lib.dd_exr_inflate(host[layout["streams_at"]:].ctypes.data, dev.data_ptr() + layout["streams_at"], n_streams, dev.data_ptr(),
                                       layout["source_bytes"], image.data_ptr(), staged_bytes, statuses.data_ptr(), stream.cuda_stream))
            if self.time_launches:
                self.inflate_events[-1][1].record(stream)
            self.inflate_launches += 1
        for src, dst, n in layout["runs"]:                          # raw and run-length decoded chunks: one device copy per run
            image[dst:dst + n].copy_(dev[src:src + n], non_blocking=True)
        if self.time_launches:
            self.events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            self.events[-1][0].record(stream)
        slot_counts = torch.zeros(len(live), dtype=torch.int64, device=self.device)
        L.check(lib.dd_exr_reconstruct(host[layout["chunks_at"]:].ctypes.data, dev.data_ptr() + layout["chunks_at"], layout["n_chunks"],
                                       host[layout["files_at"]:].ctypes.data, dev.data_ptr() + layout["files_at"], len(live),
                                       image.data_ptr(), staged_bytes, slot_counts.data_ptr(), stream.cuda_stream))
        if self.time_launches:
            self.events[-1][1].record(stream)
        self.launches += 1
        return live, slot_counts, [live[o] for o in layout["owners"]], statuses

    def decode(self, requests, errors="raise"):
        """requests: [(path, channels), ...] -> [(tensor [H, W, channels] fp32 on the device, non-finite count), ...] in input order; one
        synchronisation, at the end, to read the counts.  errors 'raise': the ExrError of the first file (in input order) that has one;
        'return': that file's place in the list holds its ExrError and the others are decoded."""
        import concurrent.futures
        import time

        import torch

        from . import _lib as L
        lib = L.load()
        requests = [(p, int(c)) for p, c in requests]
        results = [None] * len(requests)
        with concurrent.futures.ThreadPoolExecutor(max_workers=self.threads) as pool, torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)

            def plan(request):
                try:
                    return plan_file(*request)
                except ExrError as e:
                    return e
            plans = list(pool.map(plan, requests))
            for k, p in enumerate(plans):
                if isinstance(p, ExrError):
                    results[k] = p
            good = [k for k, p in enumerate(plans) if not isinstance(p, ExrError)]
            batches, room = [], 0
            for k in good:
                if not batches or room + plans[k].staged_bytes > self.max_staged_bytes:
                    batches.append([])
                    room = 0
                batches[-1].append(k)
                room += plans[k].staged_bytes
            planes, counted, checked = {}, [], []
            redo = [k for k in good if self.inflate == "device" and plans[k].source_layout()[4]]
            for b, batch in enumerate(batches):
                if self.inflate == "device":
                    done = self._inflate_batch(lib, L, pool, stream, b % self.RING, batch, plans, results, planes)
                    if done is not None:
                        counted.append(done[:2])
                        checked.append(done[2:])
                    continue
                # ---- layout of the batch's buffer: staged bytes | chunk table | file table
                bases, at = [], 0
                for k in batch:
                    bases.append(at)
                    at += plans[k].staged_bytes
                staged_bytes = max(at, _STAGE_ALIGN)
                n_chunks = sum(len(plans[k].chunks) for k in batch)
                chunks_at = _align(staged_bytes)
                files_at = _align(chunks_at + n_chunks * CHUNK_DTYPE.itemsize)
                total = files_at + len(batch) * FILE_DTYPE.itemsize
                entry = self._buffers(b % self.RING, total)
                host = entry[0].numpy()
                # ---- inflate, one job per file
                t0 = time.perf_counter()
                jobs = [pool.submit(plans[k].inflate, host[base:base + plans[k].staged_bytes]) for k, base in zip(batch, bases)]
                failed = set()
                for k, job in zip(batch, jobs):
                    try:
                        job.result()
                    except ExrError as e:
                        results[k] = e
                        failed.add(k)
                self.inflate_seconds += time.perf_counter() - t0
                # ---- the tables (a file that failed keeps its bytes in the buffer and gets neither a record nor a chunk)
                live = [(k, base) for k, base in zip(batch, bases) if k not in failed]
                chunk_table = host[chunks_at:chunks_at + n_chunks * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
                file_table = host[files_at:files_at + len(batch) * FILE_DTYPE.itemsize].view(FILE_DTYPE)
                file_table[:] = np.zeros((), dtype=FILE_DTYPE)
                n = 0
                for slot, (k, base) in enumerate(live):
                    p = plans[k]
                    planes[k] = torch.empty((p.height, p.width, p.channels), dtype=torch.float32, device=self.device)
                    row = file_table[slot]
                    row["dst"], row["H"], row["W"], row["C"], row["n_channels"] = planes[k].data_ptr(), p.height, p.width, p.channels, len(p.types)
                    row["type"][:len(p.types)] = p.types
                    row["dst_mask"][:len(p.types)] = p.dst_masks
                    part = chunk_table[n:n + len(p.chunks)]
                    part[:] = p.chunks
                    part["offset"] += base
                    part["file"] = slot
                    n += len(p.chunks)
                if n:
                    dev = self._staged[:total]
                    dev.copy_(entry[0][:total], non_blocking=True)
                    entry[1] = torch.cuda.Event()
                    entry[1].record(stream)
                    if self.time_launches:
                        self.events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                        self.events[-1][0].record(stream)
                    slot_counts = torch.zeros(len(live), dtype=torch.int64, device=self.device)
                    L.check(lib.dd_exr_reconstruct(host[chunks_at:].ctypes.data, dev.data_ptr() + chunks_at, n,
                                                   host[files_at:].ctypes.data, dev.data_ptr() + files_at, len(live),
                                                   dev.data_ptr(), staged_bytes, slot_counts.data_ptr(), stream.cuda_stream))
                    if self.time_launches:
                        self.events[-1][1].record(stream)
                    counted.append(([k for k, _ in live], slot_counts))
                    self.launches += 1
            if counted:
                n_counts = sum(len(batch) for batch, _ in counted)
                both = torch.cat([c for _, c in counted] + [s.to(torch.int64) for _, s in checked]).cpu().numpy()      # the one synchronisation
                order = [k for batch, _ in counted for k in batch]
                for k, count in zip(order, both[:n_counts].tolist()):
                    results[k] = (planes[k], int(count))
                owners = [k for batch_owners, _ in checked for k in batch_owners]
                redo += sorted({k for k, status in zip(owners, both[n_counts:].tolist()) if status != 0})
            for k in sorted(redo):                                  # inflate="device": a stream that is not OK, in input order
                self.host_fallbacks += 1
                try:
                    results[k] = self._on_host(lib, L, plans[k], stream)
                except ExrError as e:
                    results[k] = e
        if errors == "raise":
            for r in results:
                if isinstance(r, ExrError):
                    raise r
        return results


# ---------------------------------------------------------------------------------------------------- encode on the device
# The inverse of the above.  The host keeps the header, the offset table and the file; one dd_exr_pack launch (csrc/dd_exr_encode.hip) turns the
# fp32 planes of a whole batch of files into chunk bytes (samples, row and channel order, byte split, predictor), one dd_exr_deflate launch
# (csrc/dd_exr_deflate.hip) turns every chunk into a zlib stream.  plan_write and assemble need no device.
SOURCE_DTYPE = np.dtype([("src", "<u8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("n_channels", "<i4"), ("type", "<i4", (8,)),
                         ("src_channel", "<i4", (8,))])                                                                  # dd_exr_source
DEFLATE_STREAM_DTYPE = np.dtype([("src_offset", "<i8"), ("dst_offset", "<i8"), ("src_bytes", "<i4"), ("dst_capacity", "<i4")])      # dd_exr_deflate_stream
DEFLATE_OK, DEFLATE_RAW, DEFLATE_RECORD = 0, 1, 2               # DD_DEFLATE_*
HALF, FLOAT = 1, 2                                              # pixel types of a written channel
_TYPE_NAMES = {"half": HALF, "float": FLOAT, HALF: HALF, FLOAT: FLOAT}


def _pixel_type(value):
    if value not in _TYPE_NAMES:
        raise ValueError("pixel type %r (float or half)" % (value,))
    return _TYPE_NAMES[value]


class WritePlan:
    """What plan_write lays out for one file.  header: the bytes in front of the offset table; names / types / src_channels: the file's
    channels in name order; chunks: CHUNK_DTYPE records (`file` left 0) whose offset is the chunk's slot, relative to the file's slot bytes;
    raw_bytes: per chunk its n; slot_bytes: how many slot bytes the file has.  A slot is 16-byte aligned and _align(n) long: it takes the
    chunk's packed bytes in the pack buffer, and in the output buffer its zlib stream (at most dst_capacity = n - 1 bytes) or, stored raw,
    its n plain bytes.  coded: whether the chunks are predicted and deflated (ZIP, ZIPS) or plain (NONE)."""

    def __init__(self, path, height, width, names, types, src_channels, compression, header, chunks, raw_bytes, slot_bytes):
        self.path, self.height, self.width, self.names, self.types, self.src_channels = path, height, width, names, types, src_channels
        self.compression, self.header, self.chunks, self.raw_bytes, self.slot_bytes = compression, header, chunks, raw_bytes, slot_bytes
        self.coded = compression in (ZIP_COMPRESSION, ZIPS_COMPRESSION)

    def streams(self):
        """DEFLATE_STREAM_DTYPE records of the file's chunks, offsets relative to the file's slot bytes"""
        table = np.zeros(len(self.chunks), dtype=DEFLATE_STREAM_DTYPE)
        table["src_offset"] = table["dst_offset"] = self.chunks["offset"]
        table["src_bytes"] = self.raw_bytes
        table["dst_capacity"] = np.asarray(self.raw_bytes) - 1
        return table


def plan_write(path, height, width, names, types, compression=ZIP_COMPRESSION, src_channels=None):
    """The host half of a device encode, without a device: channel `names` (any order) with their pixel `types` (HALF / FLOAT, or "half" /
    "float") and the plane channel each is read from (default: its index in `names`) -> WritePlan.  The header is byte-identical to the
    one write_exr writes for the same channels."""
    if compression not in (NO_COMPRESSION, ZIPS_COMPRESSION, ZIP_COMPRESSION):
        raise ExrError("the device writes NONE, ZIPS and ZIP, not %s" % _CODEC_NAMES.get(compression, compression))
    if height < 1 or width < 1:
        raise ExrError("%s: empty image (%d x %d)" % (path, width, height))
    if not 1 <= len(names) <= MAX_FILE_CHANNELS or len(set(names)) != len(names):
        raise ExrError("%s: %d channels (1 .. %d distinct names)" % (path, len(names), MAX_FILE_CHANNELS))
    src_channels = list(range(len(names))) if src_channels is None else list(src_channels)
    order = sorted(range(len(names)), key=lambda k: names[k])
    names, types, src_channels = [names[k] for k in order], [_pixel_type(types[k]) for k in order], [int(src_channels[k]) for k in order]
    chlist = b"".join(n.encode("latin-1") + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in zip(names, types)) + b"\0"
    box = struct.pack("<4i", 0, 0, width - 1, height - 1)
    header = struct.pack("<ii", MAGIC, 2)
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([compression]))
    header += _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0")
    header += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0))
    header += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lines = _LINES[compression]
    row_bytes = sum(width * _PIXEL[t].itemsize for t in types)
    n_chunks = (height + lines - 1) // lines
    chunks, raw_bytes, at = np.zeros(n_chunks, dtype=CHUNK_DTYPE), [], 0
    coded = int(compression != NO_COMPRESSION)
    for k in range(n_chunks):
        row0 = k * lines
        rows = min(lines, height - row0)
        if rows * row_bytes > MAX_STREAM_BYTES:
            raise ExrError("%s: a chunk of %d bytes; the device takes at most %d" % (path, rows * row_bytes, MAX_STREAM_BYTES))
        chunks[k] = (at, 0, row0, rows, coded)
        raw_bytes.append(rows * row_bytes)
        at += _align(rows * row_bytes)
    return WritePlan(path, height, width, names, types, src_channels, compression, header, chunks, raw_bytes, at)


def assemble(plan, statuses, sizes, slots):
    """The file's bytes: header, offset table, then int32 y | int32 size | data per chunk.  statuses / sizes: what dd_exr_deflate gave for the
    file's chunks (ignored for NONE); slots: the file's slot bytes -- of a chunk whose status is OK its zlib stream, of one that is RAW
    (and of every chunk of a NONE file) its plain bytes."""
    slots = memoryview(slots)
    parts = []
    for k, (record, n) in enumerate(zip(plan.chunks, plan.raw_bytes)):
        at = int(record["offset"])
        size = n
        if plan.coded:
            status = int(statuses[k])
            if status == DEFLATE_OK:
                size = int(sizes[k])
                if not 1 <= size < n:
                    raise ExrError("%s: chunk %d: a stream of %d bytes for %d" % (plan.path, k, size, n))
            elif status != DEFLATE_RAW:
                raise ExrError("%s: chunk %d: deflate status %d" % (plan.path, k, status))
        parts.append((int(record["row0"]), slots[at:at + size]))
    pos = len(plan.header) + 8 * len(parts)
    table = []
    for _, data in parts:
        table.append(pos)
        pos += 8 + len(data)
    out = bytearray(plan.header) + struct.pack("<%dQ" % len(table), *table)
    for y, data in parts:
        out += struct.pack("<ii", y, len(data))
        out += data
    return bytes(out)


def _image_channels(shape):
    """write_image's channel naming: [H,W,3] is R, G, B; [H,W] is Y -> (names, plane channels)"""
    if len(shape) == 2:
        return ["Y"], 1
    if len(shape) != 3 or shape[2] != 3:
        raise ExrError("the writer takes [H,W,3] or [H,W], got %s" % (tuple(shape),))
    return ["R", "G", "B"], 3


class DeviceEncoder:
    """fp32 device planes to EXR files, all files of a call in one batch: one dd_exr_pack launch, one dd_exr_deflate launch, one
    synchronisation to read statuses and sizes, a second dd_exr_pack launch (coded = 0) for exactly the chunks that did not shrink, written
    straight into their slots, one download into a pinned buffer, and the files written on `threads` threads (at most 16).  The planes read
    back bit-identical through read_image (FLOAT) or as astype(float16) (HALF).  ZIP, ZIPS and NONE run on the device; RLE goes through the
    host writer.  The buffers grow to the largest batch seen, are reused across calls and given back by release()."""
    time_launches = False                                       # measurements: keep (start, end) events of the launches in pack_events / deflate_events

    def __init__(self, device, compression=ZIP_COMPRESSION, threads=4):
        import torch
        self.device = torch.device(device)
        if compression not in _LINES:
            raise ExrError("cannot write compression %s" % _CODEC_NAMES.get(compression, compression))
        if self.device.type != "cuda":
            raise ValueError("EXR files are encoded on a GPU: %s is none" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compression = compression
        self.threads = max(1, min(int(threads), 16))
        self._packed = self._out = self._workspace = self._tables = self._pinned = self._pinned_tables = None
        self.pack_launches = self.deflate_launches = self.raw_chunks = self.downloaded_bytes = 0
        self.host_seconds = 0.0                                 # wall time encode() spent assembling and writing the files
        self.pack_events, self.deflate_events = [], []

    def release(self):
        """Give the device and the pinned buffers back (the counters stay)."""
        import torch
        torch.cuda.synchronize(self.device)
        self._packed = self._out = self._workspace = self._tables = self._pinned = self._pinned_tables = None

    def _grow(self, name, nbytes, pinned=False):
        import torch
        have = getattr(self, name)
        if have is None or have.numel() < nbytes:
            have = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, name, have)
        return have

    def _timed(self, events, stream, launch):
        import torch
        if not self.time_launches:
            return launch()
        events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        events[-1][0].record(stream)
        launch()
        events[-1][1].record(stream)

    def encode(self, requests):
        """requests: [(path, fp32 tensor [H,W,3] (written as R, G, B) or [H,W] (as Y) on the device, "float" / "half"), ...] -> the paths."""
        import concurrent.futures
        import time

        import torch

        from . import _lib as L
        requests = [(path, image, _pixel_type(kind)) for path, image, kind in requests]
        if self.compression == RLE_COMPRESSION:                 # the run-length coder stays on the host
            for path, image, kind in requests:
                arr = image.detach().cpu().numpy().astype(np.float16 if kind == HALF else np.float32)
                names, _ = _image_channels(arr.shape)
                write_exr(path, {"Y": arr} if len(names) == 1 else {c: np.ascontiguousarray(arr[..., i]) for i, c in enumerate(names)}, RLE_COMPRESSION)
            return [path for path, _, _ in requests]
        if not requests:
            return []
        lib = L.load()
        planes, plans = [], []
        for path, image, kind in requests:
            if not torch.is_tensor(image) or image.device != self.device or image.dtype != torch.float32:
                raise ValueError("%s: the encoder takes fp32 tensors on %s" % (path, self.device))
            names, channels = _image_channels(image.shape)
            planes.append(image.detach().contiguous())
            plans.append(plan_write(path, image.shape[0], image.shape[1], names, [kind] * len(names), self.compression))
        # ---- layout: the slots of all files | per file a base; the tables: chunks | sources | streams | chunks of the second pack launch
        bases, at = [], 0
        for p in plans:
            bases.append(at)
            at += p.slot_bytes
        total = max(at, _STAGE_ALIGN)
        n_chunks = sum(len(p.chunks) for p in plans)
        coded = plans[0].coded
        sources_at = _align(n_chunks * CHUNK_DTYPE.itemsize)
        streams_at = _align(sources_at + len(plans) * SOURCE_DTYPE.itemsize)
        redo_at = _align(streams_at + n_chunks * DEFLATE_STREAM_DTYPE.itemsize)
        tables_bytes = redo_at + n_chunks * CHUNK_DTYPE.itemsize
        host = self._grow("_pinned_tables", tables_bytes, pinned=True).numpy()
        chunk_table = host[:n_chunks * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
        source_table = host[sources_at:sources_at + len(plans) * SOURCE_DTYPE.itemsize].view(SOURCE_DTYPE)
        stream_table = host[streams_at:streams_at + n_chunks * DEFLATE_STREAM_DTYPE.itemsize].view(DEFLATE_STREAM_DTYPE)
        source_table[:] = np.zeros((), dtype=SOURCE_DTYPE)
        n = 0
        for slot, (p, plane, base) in enumerate(zip(plans, planes, bases)):
            row = source_table[slot]
            row["src"], row["H"], row["W"], row["C"], row["n_channels"] = plane.data_ptr(), p.height, p.width, 1 if plane.dim() == 2 else plane.shape[2], len(p.names)
            row["type"][:len(p.types)] = p.types
            row["src_channel"][:len(p.types)] = p.src_channels
            part = chunk_table[n:n + len(p.chunks)]
            part[:] = p.chunks
            part["offset"] += base
            part["file"] = slot
            part = stream_table[n:n + len(p.chunks)]
            part[:] = p.streams()
            part["src_offset"] += base
            part["dst_offset"] += base
            n += len(p.chunks)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            out = self._grow("_out", total)
            tables = self._grow("_tables", tables_bytes)
            tables[:tables_bytes].copy_(self._pinned_tables[:tables_bytes], non_blocking=True)
            statuses = sizes = None
            if coded:
                packed = self._grow("_packed", total)
                workspace_bytes = int(lib.dd_exr_deflate_workspace(n_chunks))
                workspace = self._grow("_workspace", workspace_bytes)
                self._timed(self.pack_events, stream, lambda: L.check(lib.dd_exr_pack(
                    host.ctypes.data, tables.data_ptr(), n_chunks, host[sources_at:].ctypes.data, tables.data_ptr() + sources_at, len(plans),
                    packed.data_ptr(), total, stream.cuda_stream)))
                self.pack_launches += 1
                both = torch.empty(2 * n_chunks, dtype=torch.int32, device=self.device)
                self._timed(self.deflate_events, stream, lambda: L.check(lib.dd_exr_deflate(
                    host[streams_at:].ctypes.data, tables.data_ptr() + streams_at, n_chunks, packed.data_ptr(), total, out.data_ptr(), total,
                    workspace.data_ptr(), workspace_bytes, both.data_ptr(), both.data_ptr() + 4 * n_chunks, stream.cuda_stream)))
                self.deflate_launches += 1
                both = both.cpu().numpy()                           # the one synchronisation
                statuses, sizes = both[:n_chunks], both[n_chunks:]
                raw = np.flatnonzero(statuses == DEFLATE_RAW)
                if len(raw):
                    redo = host[redo_at:redo_at + len(raw) * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
                    redo[:] = chunk_table[raw]
                    redo["coded"] = 0
                    nbytes = len(raw) * CHUNK_DTYPE.itemsize
                    tables[redo_at:redo_at + nbytes].copy_(self._pinned_tables[redo_at:redo_at + nbytes], non_blocking=True)
                    self._timed(self.pack_events, stream, lambda: L.check(lib.dd_exr_pack(
                        host[redo_at:].ctypes.data, tables.data_ptr() + redo_at, len(raw), host[sources_at:].ctypes.data, tables.data_ptr() + sources_at,
                        len(plans), out.data_ptr(), total, stream.cuda_stream)))
                    self.pack_launches += 1
                    self.raw_chunks += len(raw)
            else:
                self._timed(self.pack_events, stream, lambda: L.check(lib.dd_exr_pack(
                    host.ctypes.data, tables.data_ptr(), n_chunks, host[sources_at:].ctypes.data, tables.data_ptr() + sources_at, len(plans),
                    out.data_ptr(), total, stream.cuda_stream)))
                self.pack_launches += 1
            pinned = self._grow("_pinned", total, pinned=True)
            pinned[:total].copy_(out[:total], non_blocking=True)
            stream.synchronize()
            self.downloaded_bytes += total
        t0 = time.perf_counter()
        slots = pinned.numpy()

        def write(k):
            p, first = plans[k], sum(len(q.chunks) for q in plans[:k])
            last = first + len(p.chunks)
            data = assemble(p, None if statuses is None else statuses[first:last], None if sizes is None else sizes[first:last],
                            slots[bases[k]:bases[k] + p.slot_bytes])
            with open(p.path, "wb") as f:
                f.write(data)
            return p.path
        with concurrent.futures.ThreadPoolExecutor(max_workers=self.threads) as pool:
            written = list(pool.map(write, range(len(plans))))
        self.host_seconds += time.perf_counter() - t0
        return written


def add_encode_arguments(p):
    """--exr_encode and --exr_type on a parser that has --exr: both only say how <Pass>.exr is written, so `device` (or `half`) without --exr
    is a usage error of the parser."""
    p.add_argument("--exr_encode", default="host", choices=["host", "device"],
                   help="with --exr, where <Pass>.exr is encoded: by the host writer, or on the device by one pack and one deflate launch for all "
                        "passes (the host writes headers, offset tables and the bytes it downloads).")
    p.add_argument("--exr_type", default="float", choices=["float", "half"], help="with --exr, the pixel type of the written channels")
    inner = p.parse_known_args

    def parse_known_args(args=None, namespace=None):
        parsed, rest = inner(args, namespace)
        if parsed.exr_encode == "device" and not parsed.exr:
            p.error("--exr_encode device needs --exr")
        if parsed.exr_type != "float" and not parsed.exr:
            p.error("--exr_type %s needs --exr" % parsed.exr_type)
        return parsed, rest
    p.parse_known_args = parse_known_args


def add_inflate_argument(p, what):
    """--exr_inflate on a parser that has --exr_decode: the device inflates only into the staged buffer of the device decoder, so `device`
    without --exr_decode device is a usage error of the parser."""
    p.add_argument("--exr_inflate", default="host", choices=["host", "device"],
                   help="%s: with --exr_decode device, where the zlib streams of ZIP / ZIPS chunks are inflated: on the host threads, or on the "
                        "device by one launch per batch (the host only reads the files)." % what)
    inner = p.parse_known_args

    def parse_known_args(args=None, namespace=None):
        parsed, rest = inner(args, namespace)
        if parsed.exr_inflate == "device" and parsed.exr_decode != "device":
            p.error("--exr_inflate device needs --exr_decode device")
        return parsed, rest
    p.parse_known_args = parse_known_args


# ---------------------------------------------------------------------------------------------------- a directory of render passes
class OpenEXRDirectory:
    """One rendered frame: a directory with one .exr per render pass, matched by '_<Pass>_' in the file name (the underscores keep
    'Normal' and 'Screen Space Normal' apart, OpenEXRDirectory.py:29-53); 1-channel passes keep channel 0 (:66-68).  A missing or
    ambiguous pass and non-finite samples raise ExrError (the reference logs and marks the directory invalid)."""

    def __init__(self, directory):
        self.directory = directory
        self.render_pass_to_image = {}

    def exr_files(self):
        return sorted(os.path.join(self.directory, n) for n in os.listdir(self.directory) if n.endswith(".exr"))

    def file_of(self, render_pass):
        hits = [p for p in self.exr_files() if "_" + render_pass + "_" in os.path.basename(p)]
        if not hits:
            raise ExrError("%s does not contain an exr file for %s" % (self.directory, render_pass))
        if len(hits) > 1:
            raise ExrError("more than one file in %s could be used for the %s pass" % (self.directory, render_pass))
        return hits[0]

    def load_images(self, render_passes, single_channel=()):
        for render_pass in render_passes:
            path = self.file_of(render_pass)
            image = read_image(path)
            if render_pass in single_channel:
                image = image[:, :, 0]
            if not np.isfinite(image).all():
                raise ExrError("there is at least one value in %s which is not finite" % path)
            self.render_pass_to_image[render_pass] = image
        return self.render_pass_to_image

    def size_of_loaded_images(self):
        for image in self.render_pass_to_image.values():
            return image.shape[0], image.shape[1]
        return 0, 0


# ---------------------------------------------------------------------------------------------------- a frame for the Predictor
def load_frame(directory, architecture, device=None, inflate="host"):
    """The feature dictionary Prediction.main builds from a directory of .exr files (Prediction.py:223-252): one [H,W,C] float32 array
    per required feature under 'source_image/0/<Pass>'.  Passes that are not loaded (`load_data` false) are constant 1.0 (colour) or
    0.5 (direct / indirect).  A pass's file is the one whose name contains '_<Pass>_'; the reference's looser rule -- the first
    listed file whose path contains the pass name -- is the fallback, made deterministic by taking the shortest such name.
    With a `device` every pass is a tensor on it: the files are decoded there by one DeviceDecoder.decode call (the same values);
    inflate="device" lets that decoder inflate on the device too."""
    if inflate not in ("host", "device"):
        raise ValueError("inflate=%r (host or device)" % (inflate,))
    if inflate == "device" and device is None:
        raise ValueError("inflate='device' needs a device to decode on")
    from .naming import Naming
    frame = OpenEXRDirectory(directory)
    files = frame.exr_files()
    features, size = {}, None
    required = list(architecture.auxiliary_features) + list(architecture.feature_predictions)
    loaded = [f for f in required if f.load_data]

    def file_of(f):
        try:
            return frame.file_of(f.name)
        except ExrError:
            loose = sorted((p for p in files if f.name in os.path.basename(p)), key=lambda p: (len(os.path.basename(p)), p))
            if not loose:
                raise ExrError("image for '%s' could not be loaded or does not exist in %s" % (f.name, directory))
            return loose[0]

    def on_host():
        for f in loaded:
            path = file_of(f)
            yield f, path, read_image(path)[..., :f.number_of_channels]

    def on_device():
        paths = [file_of(f) for f in loaded]
        decoded = DeviceDecoder(device, inflate=inflate).decode([(path, f.number_of_channels) for f, path in zip(loaded, paths)])
        for f, path, (image, _) in zip(loaded, paths, decoded):
            yield f, path, image
    for f, path, image in (on_host() if device is None else on_device()):
        if size is None:
            size = tuple(image.shape[:2])
        elif size != tuple(image.shape[:2]):
            raise ExrError("%s is %dx%d, the other passes are %dx%d" % (path, image.shape[1], image.shape[0], size[1], size[0]))
        features[Naming.source_feature_name(f.name, index=0)] = image
    if size is None:
        raise ExrError("no pass of the architecture is loaded from files")
    for f in required:
        if not f.load_data:
            value = 1.0 if f.feature_prediction_type == "COLOR" else 0.5        # Prediction.py:244-249
            shape = size + (f.number_of_channels,)
            if device is None:
                features[Naming.source_feature_name(f.name, index=0)] = np.full(shape, value, dtype=np.float32)
            else:
                import torch
                features[Naming.source_feature_name(f.name, index=0)] = torch.full(shape, value, dtype=torch.float32, device=device)
    return features


def save_predictions(directory, predictions, as_exr=False, encode="host", pixel_type="float"):
    """Prediction.py:483-510 stores every denoised pass and the combined image as <directory>/<Pass>.npy for the Blender side;
    as_exr additionally writes <Pass>.exr.  `predictions`: the dictionary Predictor.predict_frame returns.  encode="device": the .exr
    files of all passes are encoded by one DeviceEncoder.encode call from the tensors where they are (the same planes); pixel_type "half"
    writes HALF channels (the values rounded to nearest even, as numpy's astype(float16)), on either path."""
    if encode not in ("host", "device"):
        raise ValueError("encode=%r (host or device)" % (encode,))
    kind = _pixel_type(pixel_type)
    if not as_exr and (encode == "device" or kind != FLOAT):
        raise ValueError("encode=%r and pixel_type=%r say how the .exr files are written: they need as_exr" % (encode, pixel_type))
    written, requests = [], []
    for key, value in predictions.items():
        name = key.split("/", 1)[1] if key.startswith("prediction/") else key
        arr = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
        path = os.path.join(directory, name + ".npy")
        np.save(path, arr)
        written.append(path)
        if as_exr:
            exr = os.path.join(directory, name + ".exr")
            if encode == "device":
                if not hasattr(value, "detach"):
                    raise ValueError("encode='device' takes the predictions as device tensors; %s is none" % key)
                requests.append((exr, value if value.shape[-1] == 3 else value[..., 0], kind))
            elif kind == FLOAT:
                write_image(exr, arr if arr.shape[-1] == 3 else arr[..., 0])
            else:
                with np.errstate(over="ignore"):                # (a value past 65504 becomes an infinity: HALF's own rule)
                    image = np.asarray(arr if arr.shape[-1] == 3 else arr[..., 0], dtype=np.float32).astype(np.float16)
                write_exr(exr, {"Y": image} if image.ndim == 2 else {c: np.ascontiguousarray(image[..., i]) for i, c in enumerate("RGB")})
            written.append(exr)
    if requests:
        import torch
        encoder = DeviceEncoder(requests[0][1].device, threads=16)
        try:
            encoder.encode([(path, image.to(torch.float32), kind) for path, image, kind in requests])
        finally:
            encoder.release()
    return written
