"""Denoised passes as 8-bit sRGB PNGs (RFC 2083): the picture of a pass that an image viewer, a browser or a review tool opens.  Prediction.py:483-510
stores .npy only (its own PNG line is commented out).  Two paths write bit-identical pixel data:

  host    filtered_rows (numpy) -> zlib.compress -> the file                                                          (encode_host)
  device  one dd_png_pack launch (quantisation and row filters of all passes, csrc/dd_png_encode.hip), one dd_png_deflate launch (every
          segment of every pass, one wave each), one download; the host adds the chunk framing, the Adler-32 and the CRC  (DevicePngEncoder)

The picture.  A pass is fp32 [H, W, C]: 3 channels give an 8-bit RGB file (colour type 2), 1 channel an 8-bit gray file (colour type 0), not
interlaced.  The byte of a sample is the number of entries of metrics.preview_thresholds() that are <= sample * exposure (one fp32 multiply):
the sRGB transfer function with its clamp, owned by the host as a table; -inf, negatives and -0.0 give 0, +inf 255.  A NaN in any channel
makes an RGB pixel (255, 0, 255) as in the previews, a NaN gray sample 0.  Every row gets the one of PNG's five filters (None, Sub, Up,
Average, Paeth) with the smallest sum of |filtered byte as signed 8-bit|, ties to the lowest type; the row above the first is zeros.  The
file: signature, IHDR, sRGB (intent 0), ONE IDAT, IEND.

One zlib stream from independently coded segments.  The filtered rows are cut into segments of whole rows (default: the fewest rows that
reach 32 KiB, capped by what the pack kernel stages in LDS).  The IDAT payload is 78 01, the segments' raw-deflate bodies, and the Adler-32 of
all filtered bytes.  Every body but the last ends with a non-final block and an empty stored block (00 00 FF FF behind the padding: zlib's
Z_SYNC_FLUSH), so it ends on a byte border; the last body's last block is final.  The device returns each segment's Adler-32 and
adler_combine joins them; a segment that did not shrink (DEFLATE_RAW) is wrapped in stored blocks by the host.  plan_png and assemble_png
need no device."""
import os
import struct
import zlib

import numpy as np

from . import _lib as L
from .batch_encode import BatchEncoder, align16 as _align, slot_layout
from .metrics import preview_thresholds
from .summaries import PNG_SIGNATURE, _png_chunk

IMAGE_DTYPE = np.dtype(L.PngImage)                               # dd_png_image
SEGMENT_DTYPE = np.dtype(L.PngSegment)                           # dd_png_segment
STREAM_DTYPE = np.dtype(L.PngStream)                             # dd_png_stream
DEFLATE_OK, DEFLATE_RAW, DEFLATE_RECORD = L.DEFLATE_OK, L.DEFLATE_RAW, L.DEFLATE_RECORD
MAX_ROW_BYTES, STAGE_BYTES = L.PNG_MAX_ROW_BYTES, L.PNG_STAGE_BYTES
SEGMENT_TARGET_BYTES = 32768                                     # the default segment: the fewest rows whose filtered bytes reach this
STORED_BLOCK_BYTES = 65535
_ADLER = 65521


class PngError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------- the picture, in numpy
def _as_planes(image):
    a = np.asarray(image, dtype=np.float32)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise PngError("a pass of shape [H, W], [H, W, 1] or [H, W, 3] is expected, not %s" % (a.shape,))
    return a


def quantise(image, exposure=1.0):
    """The uint8 array [H, W, n] of an fp32 pass [H, W, n] (n = 1 or 3; [H, W] is n = 1)."""
    a = _as_planes(image)
    with np.errstate(over="ignore", invalid="ignore"):
        v = a * np.float32(exposure)
    nan = np.isnan(v)
    q = np.searchsorted(preview_thresholds(), np.where(nan, np.float32(0), v), side="right").astype(np.uint8)
    if a.shape[2] == 1:
        q[nan] = 0
    else:
        q[nan.any(axis=2)] = (255, 0, 255)
    return q


def filter_bytes(q):
    """The filtered rows, uint8 [H, 1 + W * n], of a uint8 picture [H, W, n]: vectorised over rows (every filter reads unfiltered bytes)."""
    H, W, n = q.shape
    x = q.reshape(H, W * n).astype(np.int16)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, n:] = x[:, :-n]
    b[1:] = x[:-1]
    c[1:, n:] = x[:-1, :-n]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    candidates = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255            # [5, H, W * n]
    cost = np.where(candidates < 128, candidates, 256 - candidates).sum(axis=2, dtype=np.int64)
    best = np.argmin(cost, axis=0)                                                           # (the first minimum: the lowest type)
    out = np.empty((H, 1 + W * n), dtype=np.uint8)
    out[:, 0] = best
    out[:, 1:] = candidates[best, np.arange(H)]
    return out


def filtered_rows(image, exposure=1.0):
    """The filtered rows of a pass, uint8 [H, 1 + W * n]: what both paths compress."""
    return filter_bytes(quantise(image, exposure))


def file_bytes(height, width, n_channels, idat):
    """signature, IHDR (8 bits, colour type 2 or 0, no interlace), sRGB with intent 0, one IDAT, IEND"""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2 if n_channels == 3 else 0, 0, 0, 0)
    return PNG_SIGNATURE + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"sRGB", b"\x00") + _png_chunk(b"IDAT", bytes(idat)) + _png_chunk(b"IEND", b"")


def encode_host(image, exposure=1.0):
    """The file bytes of a pass, compressed by zlib (level 6)."""
    a = _as_planes(image)
    return file_bytes(a.shape[0], a.shape[1], a.shape[2], zlib.compress(filtered_rows(a, exposure).tobytes(), 6))


# ---------------------------------------------------------------------------------------------------- segments
def adler_combine(adler1, adler2, len2):
    """The Adler-32 of two byte strings in a row from their Adler-32 values and the length of the second."""
    adler1, adler2, len2 = int(adler1), int(adler2), int(len2)      # (numpy's 32-bit scalars would wrap)
    a1, b1, a2, b2 = adler1 & 0xffff, adler1 >> 16, adler2 & 0xffff, adler2 >> 16
    a = (a1 + a2 - 1) % _ADLER
    b = (b1 + b2 + (len2 % _ADLER) * (a1 - 1)) % _ADLER
    return (b << 16) | a


def stored_blocks(data, final):
    """`data` as stored deflate blocks of at most 65535 bytes, the last one final if `final`.  They start and end on a byte border."""
    data = bytes(data)
    parts = []
    for at in range(0, max(len(data), 1), STORED_BLOCK_BYTES):
        piece = data[at:at + STORED_BLOCK_BYTES]
        is_last = at + STORED_BLOCK_BYTES >= len(data)
        parts.append(struct.pack("<BHH", 1 if (final and is_last) else 0, len(piece), len(piece) ^ 0xffff) + piece)
    return b"".join(parts)


class PngPlan:
    """What plan_png lays out for one file.  segments: [(y0, rows)]; raw_bytes: per segment its filtered bytes n; offsets: per segment its
    slot, relative to the file's slot bytes; slot_bytes: how many the file has.  A slot is 16-byte aligned and _align(n) long: it takes
    the segment's filtered rows in the pack buffer, and in the output buffer its deflate body (at most n - 1 bytes) or, when it did not
    shrink, its n filtered bytes."""

    def __init__(self, path, height, width, n_channels, segment_rows, segments, raw_bytes, offsets, slot_bytes):
        self.path, self.height, self.width, self.n_channels, self.segment_rows = path, height, width, n_channels, segment_rows
        self.segments, self.raw_bytes, self.offsets, self.slot_bytes = segments, raw_bytes, offsets, slot_bytes
        self.row_bytes = 1 + width * n_channels

    def segment_table(self, image=0, base=0):
        """SEGMENT_DTYPE records of the file's segments"""
        table = np.zeros(len(self.segments), dtype=SEGMENT_DTYPE)
        table["offset"] = np.asarray(self.offsets, dtype=np.int64) + base
        table["image"] = image
        table["y0"] = [y0 for y0, _ in self.segments]
        table["rows"] = [rows for _, rows in self.segments]
        return table

    def stream_table(self, base=0):
        """STREAM_DTYPE records of the file's segments: dst_capacity = n - 1, the last one marked"""
        table = np.zeros(len(self.segments), dtype=STREAM_DTYPE)
        table["src_offset"] = table["dst_offset"] = np.asarray(self.offsets, dtype=np.int64) + base
        table["src_bytes"] = self.raw_bytes
        table["dst_capacity"] = np.asarray(self.raw_bytes) - 1
        table["last"][-1] = 1
        return table


def default_segment_rows(width, n_channels):
    """the fewest rows whose filtered bytes reach SEGMENT_TARGET_BYTES, capped by what the pack kernel stages"""
    row_bytes = 1 + width * n_channels
    return max(1, min(-(-SEGMENT_TARGET_BYTES // row_bytes), STAGE_BYTES // row_bytes))


def plan_png(path, height, width, n_channels, segment_rows=None):
    """The host half of a device encode, without a device -> PngPlan."""
    if height < 1 or width < 1:
        raise PngError("%s: empty image (%d x %d)" % (path, width, height))
    if n_channels not in (1, 3):
        raise PngError("%s: %d channels (1 gray, 3 RGB)" % (path, n_channels))
    if width * n_channels > MAX_ROW_BYTES:
        raise PngError("%s: a row of %d bytes; the pack kernel holds %d" % (path, width * n_channels, MAX_ROW_BYTES))
    row_bytes = 1 + width * n_channels
    if segment_rows is None:
        segment_rows = default_segment_rows(width, n_channels)
    segment_rows = int(segment_rows)
    if not 1 <= segment_rows <= STAGE_BYTES // row_bytes:
        raise PngError("%s: segment_rows=%d (1 .. %d rows of %d bytes fit the pack kernel)" % (path, segment_rows, STAGE_BYTES // row_bytes, row_bytes))
    segments, raw_bytes, offsets, at = [], [], [], 0
    for y0 in range(0, height, segment_rows):
        rows = min(segment_rows, height - y0)
        segments.append((y0, rows))
        raw_bytes.append(rows * row_bytes)
        offsets.append(at)
        at += _align(rows * row_bytes)
    return PngPlan(path, height, width, n_channels, segment_rows, segments, raw_bytes, offsets, at)


def assemble_png(plan, statuses, sizes, adlers, slots, staged=None):
    """The file's bytes.  statuses / sizes / adlers: what dd_png_deflate gave for the file's segments; slots: the file's slot bytes of the
    output buffer (of a segment whose status is OK its deflate body); staged: the file's slot bytes of the pack buffer, read for the
    segments that are RAW (None: `slots` holds their filtered bytes too, as DevicePngEncoder arranges)."""
    slots = memoryview(slots)
    staged = slots if staged is None else memoryview(staged)
    parts, adler = [b"\x78\x01"], 1
    for k, (n, at) in enumerate(zip(plan.raw_bytes, plan.offsets)):
        status, last = int(statuses[k]), k == len(plan.segments) - 1
        if status == DEFLATE_OK:
            size = int(sizes[k])
            if not 1 <= size < n:
                raise PngError("%s: segment %d: a body of %d bytes for %d" % (plan.path, k, size, n))
            body = slots[at:at + size]
            if not last and bytes(body[-4:]) != b"\x00\x00\xff\xff":
                raise PngError("%s: segment %d does not end on a byte border" % (plan.path, k))
            parts.append(body)
        elif status == DEFLATE_RAW:
            parts.append(stored_blocks(staged[at:at + n], last))
        else:
            raise PngError("%s: segment %d: deflate status %d" % (plan.path, k, status))
        adler = adler_combine(adler, int(adlers[k]) & 0xffffffff, n)
    parts.append(struct.pack(">I", adler))
    return file_bytes(plan.height, plan.width, plan.n_channels, b"".join(parts))


# ---------------------------------------------------------------------------------------------------- the device
def _tables_layout(plans):
    """Where everything of a batch lies: the slot bytes of the files follow one another, so do their segments in the tables; the tables
    buffer holds segments | images | streams."""
    bases, first, total, n = slot_layout(plans, lambda p: len(p.segments))
    layout = {"bases": bases, "first": first, "total": total, "n_segments": n, "n_images": len(plans)}
    layout["images_at"] = _align(n * SEGMENT_DTYPE.itemsize)
    layout["streams_at"] = _align(layout["images_at"] + len(plans) * IMAGE_DTYPE.itemsize)
    layout["bytes"] = layout["streams_at"] + n * STREAM_DTYPE.itemsize
    return layout


def fill_tables(host, layout, plans, pointers, plane_channels, exposures, src_channels=None):
    """The segment, image and stream tables of _tables_layout written into the uint8 array `host`, offsets made absolute."""
    n = layout["n_segments"]
    segment_table = host[:n * SEGMENT_DTYPE.itemsize].view(SEGMENT_DTYPE)
    image_table = host[layout["images_at"]:layout["images_at"] + len(plans) * IMAGE_DTYPE.itemsize].view(IMAGE_DTYPE)
    stream_table = host[layout["streams_at"]:layout["streams_at"] + n * STREAM_DTYPE.itemsize].view(STREAM_DTYPE)
    for k, (p, base, first) in enumerate(zip(plans, layout["bases"], layout["first"])):
        image_table[k] = np.zeros((), dtype=IMAGE_DTYPE)
        row = image_table[k]
        row["src"], row["H"], row["W"], row["C"], row["n_channels"], row["exposure"] = pointers[k], p.height, p.width, plane_channels[k], p.n_channels, exposures[k]
        row["src_channel"][:p.n_channels] = list(range(p.n_channels)) if src_channels is None else src_channels[k]
        segment_table[first:first + len(p.segments)] = p.segment_table(image=k, base=base)
        stream_table[first:first + len(p.segments)] = p.stream_table(base=base)
    return segment_table, image_table, stream_table


class DevicePngEncoder(BatchEncoder):
    """fp32 device planes to PNG files, all files of a call in one batch (batch_encode.py: BatchEncoder): one upload of the tables, one
    dd_png_pack launch, one dd_png_deflate launch, one synchronisation to read statuses, sizes and Adler-32 values, the filtered bytes of the
    segments that did not shrink copied into their slots on the device, one download into a pinned buffer, and the files assembled and
    written on `threads` threads (at most 16)."""
    _files = "PNG"
    _buffers = BatchEncoder._buffers + ("_thresholds",)

    def __init__(self, device, threads=4, segment_rows=None):
        super().__init__(device, threads)
        self.segment_rows = segment_rows
        self.raw_segments = self.segments = 0
        self.staged_bytes = self.body_bytes = 0                 # what the last encode() gave deflate and what it kept of it

    def encode(self, requests):
        """requests: [(path, fp32 tensor [H, W, 3] (RGB), [H, W, 1] or [H, W] (gray) on the device, exposure), ...] -> the paths."""
        if not requests:
            return []
        planes, plans, exposures = [], [], []
        for path, image, exposure in requests:
            plane = self._plane(path, image)
            if image.dim() not in (2, 3) or (image.dim() == 3 and image.shape[2] not in (1, 3)):
                raise PngError("%s: a pass of shape [H, W], [H, W, 1] or [H, W, 3] is expected, not %s" % (path, tuple(image.shape)))
            planes.append(plane)
            n = 1 if image.dim() == 2 else image.shape[2]
            plans.append(plan_png(path, image.shape[0], image.shape[1], n, self.segment_rows))
            exposures.append(float(exposure))
        layout = _tables_layout(plans)
        host = self._grow("_pinned_tables", layout["bytes"], pinned=True).numpy()
        fill_tables(host, layout, plans, [p.data_ptr() for p in planes], [p.n_channels for p in plans], exposures)
        statuses, sizes, adlers = self._launches(layout, host)

        def assemble_one(k, slots):
            first, last = layout["first"][k], layout["first"][k] + len(plans[k].segments)
            return assemble_png(plans[k], statuses[first:last], sizes[first:last], adlers[first:last], slots)
        return self._write(plans, layout, assemble_one)

    def _launches(self, layout, host):
        """Everything on the device, for tables already filled in the pinned `host` -> (statuses, sizes, adlers) per segment; the slots are
        in _pinned afterwards."""
        import torch
        lib = L.load()
        total, n, images_at, streams_at = (layout[k] for k in ("total", "n_segments", "images_at", "streams_at"))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self._thresholds is None:
                self._thresholds = torch.from_numpy(preview_thresholds()).to(self.device)
            out, packed = self._grow("_out", total), self._grow("_packed", total)
            tables = self._grow("_tables", layout["bytes"])
            self._upload(0, layout["bytes"])
            workspace_bytes = int(lib.dd_png_deflate_workspace(n))
            workspace = self._grow("_workspace", workspace_bytes)
            self._pack(stream, lambda: lib.dd_png_pack(
                host.ctypes.data, tables.data_ptr(), n, host[images_at:].ctypes.data, tables.data_ptr() + images_at, layout["n_images"],
                self._thresholds.data_ptr(), packed.data_ptr(), total, stream.cuda_stream))
            statuses, sizes, adlers = self._deflate(stream, n, 3, lambda status_at, sizes_at, adler_at: lib.dd_png_deflate(
                host[streams_at:].ctypes.data, tables.data_ptr() + streams_at, n, packed.data_ptr(), total, out.data_ptr(), total,
                workspace.data_ptr(), workspace_bytes, status_at, sizes_at, adler_at, stream.cuda_stream))
            adlers = adlers.view(np.uint32)
            stream_table = host[streams_at:streams_at + n * STREAM_DTYPE.itemsize].view(STREAM_DTYPE)
            raw = np.flatnonzero(statuses == DEFLATE_RAW)
            k = 0
            while k < len(raw):                                     # runs of neighbouring RAW segments: one copy each (the slots are the same in both buffers)
                j = k
                while j + 1 < len(raw) and raw[j + 1] == raw[j] + 1:
                    j += 1
                start = int(stream_table["src_offset"][raw[k]])
                end = int(stream_table["src_offset"][raw[j]]) + _align(int(stream_table["src_bytes"][raw[j]]))
                out[start:end].copy_(packed[start:end], non_blocking=True)
                k = j + 1
            self._download(stream, total)
            self.raw_segments += len(raw)
            self.segments += n
            self.staged_bytes = int(stream_table["src_bytes"].sum())
            self.body_bytes = int(sizes.sum()) + int(stream_table["src_bytes"][raw].sum())
        return statuses, sizes, adlers


# ---------------------------------------------------------------------------------------------------- predictions and the command line
def save_pngs(directory, named, encode="host", exposure=1.0):
    """<directory>/<name>.png for every (name, pass) of `named` -> the paths.  encode="device": the passes are device tensors and all files
    are encoded by one DevicePngEncoder.encode call."""
    if encode not in ("host", "device"):
        raise ValueError("png_encode=%r (host or device)" % (encode,))
    paths = [os.path.join(directory, name + ".png") for name, _ in named]
    if encode == "host":
        for path, (_, value) in zip(paths, named):
            arr = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
            with open(path, "wb") as f:
                f.write(encode_host(arr, exposure))
        return paths
    if not named:
        return paths
    import torch
    for name, value in named:
        if not hasattr(value, "detach"):
            raise ValueError("png_encode='device' takes the predictions as device tensors; %s is none" % name)
    encoder = DevicePngEncoder(named[0][1].device, threads=16)
    try:
        encoder.encode([(path, value.to(torch.float32), exposure) for path, (_, value) in zip(paths, named)])
    finally:
        encoder.release()
    return paths


def add_png_arguments(p):
    """--png and --png_encode on a parser: --png_encode only says how <Pass>.png is written, so `device` without --png is a usage error."""
    from .openexr.frames import _add_rule
    p.add_argument("--png", action="store_true", help="also write <Pass>.png: the 8-bit sRGB picture of every pass (times --exposure), for viewers and review tools")
    p.add_argument("--png_encode", default="host", choices=["host", "device"],
                   help="with --png, where <Pass>.png is encoded: by numpy and zlib on the host, or on the device by one pack and one deflate launch "
                        "for all passes (the host adds the chunk framing and checksums to the bytes it downloads).")
    _add_rule(p, lambda parsed: "--png_encode device needs --png" if parsed.png_encode == "device" and not parsed.png else None)
