"""Decode on the device.  The host keeps the header, the offset table and inflate (zlib releases the GIL); the predictor, the byte split, the
row / channel split and the conversion to fp32 are one dd_exr_reconstruct launch over the staged bytes of many files
(csrc/dd_exr_decode.hip).  With inflate="device" the host keeps only the header, the offset table and the run-length decode: one
dd_exr_inflate launch per batch (csrc/dd_exr_inflate.hip) expands the zlib streams of the ZIP / ZIPS chunks into the staged buffer on the
device.  plan_file and pack_batch need no device."""
import zlib

import numpy as np

from .. import _lib as L
from .codec import NO_COMPRESSION, RLE_COMPRESSION, ZIP_COMPRESSION, ZIPS_COMPRESSION, ExrError, _rle_decode, _walk
from .records import CHUNK_DTYPE, FILE_DTYPE, MAX_FILE_CHANNELS, MAX_STREAM_BYTES, STREAM_DTYPE, _STAGE_ALIGN, _align, fill_row, timed


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

    def host_job(self, inflate):
        """What the host does with this file before a batch is uploaded -> (the bytes it writes, the method that writes them): the staged
        image itself (inflate="host"), or the source bytes the device makes it from (inflate="device")."""
        return (self.staged_bytes, self.inflate) if inflate == "host" else (self.source_layout()[0], self.fill_source)


def _batch_layout(plans, inflate="device"):
    """the arithmetic of pack_batch: where everything lies.  With inflate="host" the source bytes are the staged image: no stream, no run."""
    device = inflate == "device"
    source_bases, staged_bases, source_at, staged_at = [], [], 0, 0
    for p in plans:
        source_bases.append(source_at)
        staged_bases.append(staged_at)
        source_at = _align(source_at + p.host_job(inflate)[0])
        staged_at += p.staged_bytes
    n_streams = sum(len(p.source_layout()[1]) for p in plans) if device else 0
    n_chunks = sum(len(p.chunks) for p in plans)
    layout = {"inflate": inflate, "source_bases": source_bases, "staged_bases": staged_bases, "source_bytes": max(source_at, _STAGE_ALIGN),
              "staged_bytes": max(staged_at, _STAGE_ALIGN), "n_streams": n_streams, "n_chunks": n_chunks}
    layout["streams_at"] = _align(layout["source_bytes"])
    layout["chunks_at"] = _align(layout["streams_at"] + n_streams * STREAM_DTYPE.itemsize)
    layout["files_at"] = _align(layout["chunks_at"] + n_chunks * CHUNK_DTYPE.itemsize)
    layout["total"] = layout["files_at"] + len(plans) * FILE_DTYPE.itemsize
    layout["runs"], layout["owners"] = [], []
    if device:
        layout["runs"] = [(src + sb, dst + db, n) for p, sb, db in zip(plans, source_bases, staged_bases) for src, dst, n in p.source_layout()[2]]
        layout["owners"] = [k for k, p in enumerate(plans) for _ in range(len(p.source_layout()[1]))]
    return layout


def pack_batch(plans, inflate="device"):
    """The upload buffer of one batch, in plain numpy (DeviceDecoder lays its pinned buffer out the same way): source bytes of every
    file | stream table | chunk table.  -> (buffer uint8, layout) with layout = {"inflate", "source_bases", "staged_bases", "source_bytes",
    "staged_bytes", "streams_at", "n_streams", "chunks_at", "n_chunks", "files_at", "total", "runs": [(source offset, staged offset, bytes)]
    of the whole batch, "owners": per stream the index of its plan}.  The file table's place is reserved; its rows hold device pointers and
    are written by the decoder."""
    layout = _batch_layout(plans, inflate)
    buffer = np.zeros(layout["total"], dtype=np.uint8)
    fill_batch_tables(buffer, layout, plans)
    for p, base in zip(plans, layout["source_bases"]):
        nbytes, fill = p.host_job(inflate)
        fill(buffer[base:base + nbytes])
    return buffer, layout


def fill_batch_tables(buffer, layout, plans):
    """The stream and the chunk table of pack_batch's layout, written into `buffer`: offsets made absolute, a chunk's `file` the index of
    its plan."""
    streams = buffer[layout["streams_at"]:layout["streams_at"] + layout["n_streams"] * STREAM_DTYPE.itemsize].view(STREAM_DTYPE)
    chunks = buffer[layout["chunks_at"]:layout["chunks_at"] + layout["n_chunks"] * CHUNK_DTYPE.itemsize].view(CHUNK_DTYPE)
    ns = nc = 0
    for slot, (p, source_base, staged_base) in enumerate(zip(plans, layout["source_bases"], layout["staged_bases"])):
        if layout["inflate"] == "device":
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
    """The host half of a device decode of `path` into the plane read_image(path)[..., :channels]: the walk of read_exr over header, offset
    table and chunks (the same ExrErrors), no inflate yet and no device.  -> FilePlan."""
    if channels < 1:
        raise ValueError("channels=%d" % channels)
    channels = min(int(channels), 3)
    with open(path, "rb") as f:
        buf = f.read()
    walk = _walk(path, buf)
    head = next(walk)
    x0, y0, x1, y1 = head["data_window"]
    W, H = x1 - x0 + 1, y1 - y0 + 1
    if W < 1 or H < 1:
        raise ExrError("%s: empty data window (%d x %d)" % (path, W, H))
    chans = head["channels"]
    if len(chans) > MAX_FILE_CHANNELS:
        raise ExrError("%s: %d channels; the device decoder takes at most %d" % (path, len(chans), MAX_FILE_CHANNELS))
    compression = head["compression"]
    records, pieces, at = [], [], 0
    for r0, nl, data, expected in walk:
        coded = len(data) != expected                           # (as _decode_chunk: a chunk of the full size is stored raw)
        if coded and compression == NO_COMPRESSION:
            raise ExrError("chunk of %d bytes where %d are expected" % (len(data), expected))
        records.append((at, 0, r0, nl, int(coded)))
        pieces.append((data, coded, expected))
        at += _align(expected)
    masks = _destination_masks(path, [name for name, _ in chans], channels)
    return FilePlan(path, H, W, channels, [t for _, t in chans], masks, compression, np.array(records, dtype=CHUNK_DTYPE), at, pieces)


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
    the end; a file with a stream that is not OK is redone as a batch of its own with inflate="host" (`host_fallbacks` counts them), so a
    corrupt file raises what inflate="host" raises and a stream the device refused but zlib accepts still decodes."""
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
        self.uploaded_bytes = 0                                 # of every batch, in both modes
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

    def _batch(self, lib, pool, stream, slot, inflate, keys, plans, results, planes):
        """One batch, the files `keys` of `plans`, through ring slot `slot`: the host jobs (FilePlan.host_job) on the pool, one upload, with
        inflate="device" one dd_exr_inflate launch and the run copies, one dd_exr_reconstruct launch into fresh `planes`.  A file whose job
        raises an ExrError gets it into `results`, and the batch is laid out again without it.  -> (files in table order, their counts on
        the device, per stream the file it belongs to, the statuses on the device), or None when no file of the batch is left."""
        import time

        import torch
        t0 = time.perf_counter()
        live = list(keys)
        while live:
            batch = [plans[k] for k in live]
            layout = _batch_layout(batch, inflate)
            entry = self._buffers(slot, layout["total"], layout["staged_bytes"] if inflate == "device" else 0)
            host = entry[0].numpy()
            jobs = []
            for p, base in zip(batch, layout["source_bases"]):
                nbytes, fill = p.host_job(inflate)
                jobs.append(pool.submit(fill, host[base:base + nbytes]))
            bad = set()
            for k, job in zip(live, jobs):
                try:
                    job.result()
                except ExrError as e:
                    results[k] = e
                    bad.add(k)
            if not bad:
                break
            live = [k for k in live if k not in bad]
        self.inflate_seconds += time.perf_counter() - t0
        if not live:
            return None
        total, staged_bytes, n_streams = layout["total"], layout["staged_bytes"], layout["n_streams"]
        fill_batch_tables(host, layout, batch)
        file_table = host[layout["files_at"]:total].view(FILE_DTYPE)
        for row, (k, p) in enumerate(zip(live, batch)):
            planes[k] = torch.empty((p.height, p.width, p.channels), dtype=torch.float32, device=self.device)
            fill_row(file_table, row, planes[k].data_ptr(), p.height, p.width, p.channels, p.types, p.dst_masks)
        dev = self._staged[:total]
        image = self._image[:staged_bytes] if inflate == "device" else dev      # (inflate="host": the uploaded bytes are the staged image)
        dev.copy_(entry[0][:total], non_blocking=True)
        self.uploaded_bytes += total
        entry[1] = torch.cuda.Event()
        entry[1].record(stream)
        statuses = torch.empty(n_streams, dtype=torch.int32, device=self.device)
        if n_streams:
            timed(self.time_launches, self.inflate_events, stream, lambda: L.check(lib.dd_exr_inflate(
                host[layout["streams_at"]:].ctypes.data, dev.data_ptr() + layout["streams_at"], n_streams, dev.data_ptr(), layout["source_bytes"],
                image.data_ptr(), staged_bytes, statuses.data_ptr(), stream.cuda_stream)))
            self.inflate_launches += 1
        for src, dst, n in layout["runs"]:                          # raw and run-length decoded chunks: one device copy per run
            image[dst:dst + n].copy_(dev[src:src + n], non_blocking=True)
        counts = torch.zeros(len(live), dtype=torch.int64, device=self.device)
        timed(self.time_launches, self.events, stream, lambda: L.check(lib.dd_exr_reconstruct(
            host[layout["chunks_at"]:].ctypes.data, dev.data_ptr() + layout["chunks_at"], layout["n_chunks"],
            host[layout["files_at"]:].ctypes.data, dev.data_ptr() + layout["files_at"], len(live),
            image.data_ptr(), staged_bytes, counts.data_ptr(), stream.cuda_stream)))
        self.launches += 1
        return live, counts, [live[o] for o in layout["owners"]], statuses

    def decode(self, requests, errors="raise"):
        """requests: [(path, channels), ...] -> [(tensor [H, W, channels] fp32 on the device, non-finite count), ...] in input order; one
        synchronisation, at the end, to read the counts.  errors 'raise': the ExrError of the first file (in input order) that has one;
        'return': that file's place in the list holds its ExrError and the others are decoded."""
        import concurrent.futures

        import torch
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
            redo = [k for k in good if self.inflate == "device" and plans[k].source_layout()[4]]      # refused up front: redone with the failed
            for b, batch in enumerate(batches):
                done = self._batch(lib, pool, stream, b % self.RING, self.inflate, [k for k in batch if k not in redo], plans, results, planes)
                if done is not None:
                    counted.append(done[:2])
                    checked.append(done[2:])
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
                done = self._batch(lib, pool, stream, 0, "host", [k], plans, results, planes)      # (after the synchronisation: slot 0 is free)
                if done is not None:
                    results[k] = (planes[k], int(done[1].item()))
        if errors == "raise":
            for r in results:
                if isinstance(r, ExrError):
                    raise r
        return results
