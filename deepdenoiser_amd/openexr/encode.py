"""Encode on the device: the inverse of decode.py.  The host keeps the header, the offset table and the file; one dd_exr_pack launch
(csrc/dd_exr_encode.hip) turns the fp32 planes of a whole batch of files into chunk bytes (samples, row and channel order, byte split,
predictor), one dd_exr_deflate launch (csrc/dd_exr_deflate.hip) turns every chunk into a zlib stream.  plan_write and assemble need no
device."""
import struct

import numpy as np

from .. import _lib as L
from ..batch_encode import BatchEncoder, slot_layout
from .codec import (_CODEC_NAMES, _LINES, _PIXEL, NO_COMPRESSION, RLE_COMPRESSION, ZIP_COMPRESSION, ZIPS_COMPRESSION, ExrError, _header,
                    _image_channels, _image_planes, write_exr)
from .records import (CHUNK_DTYPE, DEFLATE_OK, DEFLATE_RAW, DEFLATE_STREAM_DTYPE, MAX_FILE_CHANNELS, MAX_STREAM_BYTES, SOURCE_DTYPE,
                      _align, fill_row)

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
    "float") and the plane channel each is read from (default: its index in `names`) -> WritePlan.  The header is the one write_exr writes
    for the same channels."""
    if compression not in (NO_COMPRESSION, ZIPS_COMPRESSION, ZIP_COMPRESSION):
        raise ExrError("the device writes NONE, ZIPS and ZIP, not %s" % _CODEC_NAMES.get(compression, compression))
    if height < 1 or width < 1:
        raise ExrError("%s: empty image (%d x %d)" % (path, width, height))
    if not 1 <= len(names) <= MAX_FILE_CHANNELS or len(set(names)) != len(names):
        raise ExrError("%s: %d channels (1 .. %d distinct names)" % (path, len(names), MAX_FILE_CHANNELS))
    src_channels = list(range(len(names))) if src_channels is None else list(src_channels)
    order = sorted(range(len(names)), key=lambda k: names[k])
    names, types, src_channels = [names[k] for k in order], [_pixel_type(types[k]) for k in order], [int(src_channels[k]) for k in order]
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
    header = _header(names, types, compression, width, height)
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


def _tables_layout(plans):
    """Where everything of a batch lies.  The slot bytes of the files follow one another ("bases", "total" of them), so do their chunks in
    the tables ("first_chunk"); the tables buffer holds chunks | sources | streams | the chunks of the second pack launch."""
    bases, first_chunk, total, n_chunks = slot_layout(plans, lambda p: len(p.chunks))
    layout = {"bases": bases, "first_chunk": first_chunk, "total": total, "n_chunks": n_chunks, "n_files": len(plans)}
    layout["sources_at"] = _align(n_chunks * CHUNK_DTYPE.itemsize)
    layout["streams_at"] = _align(layout["sources_at"] + len(plans) * SOURCE_DTYPE.itemsize)
    layout["redo_at"] = _align(layout["streams_at"] + n_chunks * DEFLATE_STREAM_DTYPE.itemsize)
    layout["bytes"] = layout["redo_at"] + n_chunks * CHUNK_DTYPE.itemsize
    return layout


def _fill_tables(host, layout, plans, pointers, plane_channels):
    """The chunk, source and stream tables of _tables_layout written into `host`, offsets made absolute; pointers / plane_channels: per file
    the device address of its fp32 plane and how many channels that has.  -> the chunk table."""
    n_chunks = layout["n_chunks"]
    chunk_table = host[:n_chunks * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
    source_table = host[layout["sources_at"]:layout["sources_at"] + len(plans) * SOURCE_DTYPE.itemsize].view(SOURCE_DTYPE)
    stream_table = host[layout["streams_at"]:layout["streams_at"] + n_chunks * DEFLATE_STREAM_DTYPE.itemsize].view(DEFLATE_STREAM_DTYPE)
    for slot, (p, base, first) in enumerate(zip(plans, layout["bases"], layout["first_chunk"])):
        fill_row(source_table, slot, pointers[slot], p.height, p.width, plane_channels[slot], p.types, p.src_channels)
        part = chunk_table[first:first + len(p.chunks)]
        part[:] = p.chunks
        part["offset"] += base
        part["file"] = slot
        part = stream_table[first:first + len(p.chunks)]
        part[:] = p.streams()
        part["src_offset"] += base
        part["dst_offset"] += base
    return chunk_table


class DeviceEncoder(BatchEncoder):
    """fp32 device planes to EXR files, all files of a call in one batch (batch_encode.py: BatchEncoder): one dd_exr_pack launch, one
    dd_exr_deflate launch, one synchronisation to read statuses and sizes, a second dd_exr_pack launch (coded = 0) for exactly the chunks that
    did not shrink, written straight into their slots, one download into a pinned buffer, and the files written on `threads` threads (at
    most 16).  The planes read back bit-identical through read_image (FLOAT) or as astype(float16) (HALF).  ZIP, ZIPS and NONE run on the
    device; RLE goes through the host writer."""
    _files = "EXR"

    def __init__(self, device, compression=ZIP_COMPRESSION, threads=4):
        if compression not in _LINES:
            raise ExrError("cannot write compression %s" % _CODEC_NAMES.get(compression, compression))
        super().__init__(device, threads)
        self.compression = compression
        self.raw_chunks = 0

    def encode(self, requests):
        """requests: [(path, fp32 tensor [H,W,3] (written as R, G, B) or [H,W] (as Y) on the device, "float" / "half"), ...] -> the paths."""
        requests = [(path, image, _pixel_type(kind)) for path, image, kind in requests]
        if self.compression == RLE_COMPRESSION:                 # the run-length coder stays on the host
            for path, image, kind in requests:
                write_exr(path, _image_planes(image.detach().cpu().numpy().astype(np.float16 if kind == HALF else np.float32)), RLE_COMPRESSION)
            return [path for path, _, _ in requests]
        if not requests:
            return []
        planes, plans = [], []
        for path, image, kind in requests:
            planes.append(self._plane(path, image))
            names = _image_channels(image.shape)
            plans.append(plan_write(path, image.shape[0], image.shape[1], names, [kind] * len(names), self.compression))
        layout = _tables_layout(plans)
        host = self._grow("_pinned_tables", layout["bytes"], pinned=True).numpy()
        chunk_table = _fill_tables(host, layout, plans, [plane.data_ptr() for plane in planes], [1 if plane.dim() == 2 else plane.shape[2] for plane in planes])
        statuses, sizes = self._launches(layout, host, chunk_table, plans[0].coded)

        def assemble_one(k, slots):
            first, last = layout["first_chunk"][k], layout["first_chunk"][k] + len(plans[k].chunks)
            return assemble(plans[k], None if statuses is None else statuses[first:last], None if sizes is None else sizes[first:last], slots)
        return self._write(plans, layout, assemble_one)

    def _launches(self, layout, host, chunk_table, coded):
        """Everything on the device, for tables already filled in the pinned `host`: upload of the tables, pack, deflate, the one
        synchronisation, the second pack of the chunks that came back RAW, the download of the slots into _pinned
        -> (statuses, sizes) per chunk; (None, None) when the chunks are not coded (one pack launch straight into the slots)."""
        import torch
        lib = L.load()
        total, n_chunks, sources_at, streams_at, redo_at = (layout[k] for k in ("total", "n_chunks", "sources_at", "streams_at", "redo_at"))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            out = self._grow("_out", total)
            tables = self._grow("_tables", layout["bytes"])

            def pack(chunks_at, count, destination):
                self._pack(stream, lambda: lib.dd_exr_pack(
                    host[chunks_at:].ctypes.data, tables.data_ptr() + chunks_at, count, host[sources_at:].ctypes.data, tables.data_ptr() + sources_at,
                    layout["n_files"], destination.data_ptr(), total, stream.cuda_stream))
            self._upload(0, layout["bytes"])
            statuses = sizes = None
            if coded:
                packed = self._grow("_packed", total)
                workspace_bytes = int(lib.dd_exr_deflate_workspace(n_chunks))
                workspace = self._grow("_workspace", workspace_bytes)
                pack(0, n_chunks, packed)
                statuses, sizes = self._deflate(stream, n_chunks, 2, lambda status_at, sizes_at: lib.dd_exr_deflate(
                    host[streams_at:].ctypes.data, tables.data_ptr() + streams_at, n_chunks, packed.data_ptr(), total, out.data_ptr(), total,
                    workspace.data_ptr(), workspace_bytes, status_at, sizes_at, stream.cuda_stream))
                raw = np.flatnonzero(statuses == DEFLATE_RAW)
                if len(raw):
                    redo = host[redo_at:redo_at + len(raw) * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
                    redo[:] = chunk_table[raw]
                    redo["coded"] = 0
                    self._upload(redo_at, len(raw) * CHUNK_DTYPE.itemsize)
                    pack(redo_at, len(raw), out)
                    self.raw_chunks += len(raw)
            else:
                pack(0, n_chunks, out)
            self._download(stream, total)
        return statuses, sizes
