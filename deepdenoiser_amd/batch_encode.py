"""What the device file writers (openexr/encode.py: DeviceEncoder, png.py: DevicePngEncoder) do alike.  Both turn the fp32 planes of a whole
batch of files into records of 16-byte aligned slots, upload the record tables, run one pack and one deflate launch over all records (the
launch side of the coder: csrc/dd_deflate_launch.h), read the results with one synchronisation, download the slots into a pinned buffer and
assemble and write the files on threads.  torch is imported where a device is needed."""
from . import _lib as L

ALIGN = 16                                                      # a record's offset in a staged buffer; it owns the bytes up to the next multiple


def align16(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def timed(keep, events, stream, launch):
    """Run `launch()`; with `keep` (a class's time_launches) between a (start, end) pair of timing events on `stream`, appended to `events`."""
    if not keep:
        return launch()
    import torch
    events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
    events[-1][0].record(stream)
    launch()
    events[-1][1].record(stream)


def slot_layout(plans, count):
    """The slot bytes of the files of a batch follow one another, so do their records in the tables: plans with .slot_bytes, count(plan)
    records each -> (per file the base of its slot bytes, per file the index of its first record, all slot bytes (at least one slot),
    all records)."""
    bases, first, at, n = [], [], 0, 0
    for p in plans:
        bases.append(at)
        first.append(n)
        at += p.slot_bytes
        n += count(p)
    return bases, first, max(at, ALIGN), n


class BatchEncoder:
    """The device, the buffers and the steps of an encode call that do not depend on the file format.  The buffers (_buffers) grow to the
    largest batch seen, are reused across calls and given back by release().  A subclass names its files (_files) and says in its encode()
    what is packed, what is deflated and what becomes of the records that did not shrink."""
    time_launches = False                                       # measurements: keep (start, end) events of the launches in pack_events / deflate_events
    _files = None                                               # "EXR", "PNG"
    _buffers = ("_packed", "_out", "_workspace", "_tables", "_pinned", "_pinned_tables")

    def __init__(self, device, threads):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("%s files are encoded on a GPU: %s is none" % (self._files, self.device))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.threads = max(1, min(int(threads), 16))
        for name in self._buffers:
            setattr(self, name, None)
        self.pack_launches = self.deflate_launches = self.downloaded_bytes = 0
        self.host_seconds = 0.0                                 # wall time encode() spent assembling and writing the files
        self.pack_events, self.deflate_events = [], []

    def release(self):
        """Give the device and the pinned buffers back (the counters stay)."""
        import torch
        torch.cuda.synchronize(self.device)
        for name in self._buffers:
            setattr(self, name, None)

    def _grow(self, name, nbytes, pinned=False):
        import torch
        have = getattr(self, name)
        if have is None or have.numel() < nbytes:
            have = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, name, have)
        return have

    def _plane(self, path, image):
        """the contiguous plane of a request"""
        import torch
        if not torch.is_tensor(image) or image.device != self.device or image.dtype != torch.float32:
            raise ValueError("%s: the encoder takes fp32 tensors on %s" % (path, self.device))
        return image.detach().contiguous()

    def _upload(self, at, nbytes):
        """bytes at .. at + nbytes of the pinned tables to the same place of the device tables"""
        self._tables[at:at + nbytes].copy_(self._pinned_tables[at:at + nbytes], non_blocking=True)

    def _pack(self, stream, launch):
        timed(self.time_launches, self.pack_events, stream, lambda: L.check(launch()))
        self.pack_launches += 1

    def _deflate(self, stream, n, k, launch):
        """launch(address of result array 0, .., of array k - 1), each of n int32, runs the deflate entry point -> the k arrays on the host,
        after the one synchronisation of an encode call"""
        import torch
        results = torch.empty(k * n, dtype=torch.int32, device=self.device)
        timed(self.time_launches, self.deflate_events, stream, lambda: L.check(launch(*(results.data_ptr() + 4 * n * j for j in range(k)))))
        self.deflate_launches += 1
        results = results.cpu().numpy()                         # the one synchronisation
        return [results[j * n:(j + 1) * n] for j in range(k)]

    def _download(self, stream, total):
        """the first `total` slot bytes of _out into _pinned; the stream is drained afterwards"""
        pinned = self._grow("_pinned", total, pinned=True)
        pinned[:total].copy_(self._out[:total], non_blocking=True)
        stream.synchronize()
        self.downloaded_bytes += total

    def _write(self, plans, layout, assemble_one):
        """assemble_one(k, the slot bytes of file k in _pinned) -> the bytes of plans[k].path; written on the threads -> the paths"""
        import concurrent.futures
        import time
        t0 = time.perf_counter()
        slots = self._pinned.numpy()

        def write(k):
            p, base = plans[k], layout["bases"][k]
            data = assemble_one(k, slots[base:base + p.slot_bytes])
            with open(p.path, "wb") as f:
                f.write(data)
            return p.path
        with concurrent.futures.ThreadPoolExecutor(max_workers=self.threads) as pool:
            written = list(pool.map(write, range(len(plans))))
        self.host_seconds += time.perf_counter() - t0
        return written
