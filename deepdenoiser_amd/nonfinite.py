"""NaN / Inf samples of render passes on the device: find them, report them, fill them in (csrc/dd_nonfinite.hip).

Path-traced frames regularly carry a few NaN / Inf samples; one of them turns a whole tile of every predicted pass into NaN.  The reference
ships a per-file host tool to look for them (TensorFlow/NaNHighlighter.py) and drops such frames from its data sets
(TensorFlow/OpenEXRDirectory.py:72-76); a frame that has to be delivered is scanned and repaired here, where it already sits in device memory.

    scanner = Scanner(device, [("source_image/0/Diffuse Color", (H, W, 3)), ("source_image/0/Depth", (H, W, 1)), ...])
    scanner.scan(tensors)            # one launch: mask planes + exact counts, no device-to-host copy
    scanner.repair(tensors)          # one launch, in place: masked values <- mean of the unmasked values of the window
    scanner.report()                 # synchronises: {name: {"values": int, "pixels": int}}
"""
import ctypes as C

import torch

from . import _lib as L


class Scanner:
    """The mask planes, the counts buffer and the plane table of one frame size ([H,W,ld] planes) or one batch shape ([N,H,W,ld] planes).

    names_and_shapes: a sequence of (name, shape) or (name, shape, channels).  `shape` is the tensor's shape; its last entry is the leading
    dimension in floats, `channels` (1 or 3, by default the last entry) the channels that are looked at: a pass whose frame is wider than the
    pass is scanned with the pass's channels."""

    def __init__(self, device, names_and_shapes):
        self.lib = L.load()
        self.device = torch.device(device)
        self.names, self.shapes, self.channels = [], [], []
        names_and_shapes = list(names_and_shapes)
        self._frames = all(len(entry[1]) == 3 for entry in names_and_shapes)      # masks() then hands back [H,W] planes
        for entry in names_and_shapes:
            name, shape = entry[0], tuple(int(v) for v in entry[1])
            if len(shape) == 3:
                shape = (1,) + shape
            if len(shape) != 4:
                raise ValueError("%s: an [H,W,ld] or [N,H,W,ld] shape is expected, not %s" % (name, tuple(entry[1])))
            ch = int(entry[2]) if len(entry) > 2 else shape[3]
            if ch not in (1, 3) or shape[3] < ch:
                raise ValueError("%s: 1 or 3 channels out of a leading dimension >= that are expected, not %d out of %d" % (name, ch, shape[3]))
            if self.shapes and shape[:3] != self.shapes[0][:3]:
                raise ValueError("%s: every plane shares N, H, W; got %s after %s" % (name, shape[:3], self.shapes[0][:3]))
            self.names.append(name)
            self.shapes.append(shape)
            self.channels.append(ch)
        if not 1 <= len(self.names) <= L.NONFINITE_MAX_PLANES:
            raise ValueError("1 .. %d planes are expected, not %d" % (L.NONFINITE_MAX_PLANES, len(self.names)))
        if len(set(self.names)) != len(self.names):
            raise ValueError("plane names must be distinct")
        self.N, self.H, self.W = self.shapes[0][:3]
        self._masks = torch.empty((len(self.names), self.N, self.H, self.W), dtype=torch.uint8, device=self.device)
        self._counts = torch.zeros((len(self.names), 2), dtype=torch.int64, device=self.device)
        self._desc = L.NonfiniteDesc()
        self._desc.n_planes = len(self.names)
        for i in range(len(self.names)):
            self._desc.plane[i].C, self._desc.plane[i].ld = self.channels[i], self.shapes[i][3]
            self._desc.plane[i].mask = self._masks[i].data_ptr()
        self._scanned = False

    def _bind(self, tensors):
        """Point the table at the tensors (a {name: tensor} mapping or a sequence in the order of the names)."""
        seq = [tensors[n] for n in self.names] if hasattr(tensors, "keys") else list(tensors)
        if len(seq) != len(self.names):
            raise ValueError("%d tensors for %d planes" % (len(seq), len(self.names)))
        for i, t in enumerate(seq):
            shape = tuple(t.shape) if t.dim() == 4 else (1,) + tuple(t.shape)
            if t.dtype != torch.float32 or t.device != self._masks.device or not t.is_contiguous() or shape != self.shapes[i]:
                raise ValueError("%s: a contiguous float32 %s tensor on %s is expected, not %s %s on %s"
                                 % (self.names[i], self.shapes[i], self._masks.device, t.dtype, tuple(t.shape), t.device))
            self._desc.plane[i].data = t.data_ptr()

    def scan(self, tensors):
        """Mask planes and counts of `tensors`, enqueued on the current stream; nothing is copied to the host."""
        self._bind(tensors)
        self._counts.zero_()
        L.check(self.lib.dd_nonfinite_scan(C.byref(self._desc), self.N, self.H, self.W, self._counts.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self._scanned = True

    def repair(self, tensors, radius=2):
        """In place, after scan() of the same tensors: every masked value becomes the mean of the unmasked values of its channel in the
        (2 radius + 1)^2 window (0 when there is none).  A plane without a non-finite value is left alone by the launch."""
        if not self._scanned:
            raise RuntimeError("repair() needs the masks of a scan() of the same tensors")
        self._bind(tensors)
        L.check(self.lib.dd_nonfinite_repair(C.byref(self._desc), self.N, self.H, self.W, int(radius), self._counts.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))

    def report(self):
        """{name: {"values": non-finite values, "pixels": pixels with at least one}} of the last scan (synchronises)."""
        if not self._scanned:
            raise RuntimeError("report() needs a scan()")
        counts = self._counts.cpu().tolist()
        return {n: {"values": int(v), "pixels": int(p)} for n, (v, p) in zip(self.names, counts)}

    def masks(self):
        """{name: uint8 [N,H,W] (or [H,W] for frames) device plane}: bit c is set where channel c was non-finite in the last scan."""
        return {n: (self._masks[i, 0] if self._frames else self._masks[i]) for i, n in enumerate(self.names)}


def mask_to_rgb(mask, channels):
    """uint8 mask plane [H,W] -> uint8 [H,W,3] picture: channel c is 255 where mask bit c is set; a 1-channel pass is replicated."""
    bits = [0, 0, 0] if channels == 1 else [0, 1, 2]
    return torch.stack([((mask >> b) & 1) * 255 for b in bits], dim=-1).to(torch.uint8)
