"""What the host classes of the frame-level launches share (quality.FrameQuality, temporal.TemporalStabilizer,
sequence_quality.SequenceQuality): the check of a frame tensor, the records and the scratch of a launch, the one copy that reads the records
back, and the motion scale of the two launches that follow the Motion Vector pass."""
import ctypes as C
import math

import torch

from . import _lib as L

MOTION_SCALE = (-1.0, 1.0)      # an unverified reading of Cycles' Vector pass (temporal.py)


def motion_scale(value=None):
    """(sx, sy) of previous position = (x + sx * motion channel 0, y + sy * motion channel 1) as two floats; None: MOTION_SCALE."""
    scale = tuple(float(v) for v in (MOTION_SCALE if value is None else value))
    if len(scale) != 2 or not all(math.isfinite(v) for v in scale):
        raise ValueError("motion_scale must be two finite numbers, not %r" % (value,))
    return scale


def check_frame(what, v, H, W, device, channels=None, least=1):
    """ValueError unless v is a float32 [H,W,C] tensor on `device`, dense or a [..., :C] view of a dense frame, with C in `channels` (when
    given) and C >= least."""
    if not torch.is_tensor(v) or v.dim() != 3 or tuple(v.shape[:2]) != (H, W) or v.dtype != torch.float32 or v.device != device:
        raise ValueError("%s must be a float32 [%d,%d,C] tensor on %s, not %s" % (what, H, W, device, (
            "%s %s on %s" % (v.dtype, tuple(v.shape), v.device)) if torch.is_tensor(v) else type(v).__name__))
    if v.stride(2) != 1 or v.stride(1) < v.shape[2] or v.stride(0) != W * v.stride(1):
        raise ValueError("%s must be a dense [H,W,ld] frame or a [..., :C] view of one" % what)
    if channels is not None and v.shape[2] not in channels:
        raise ValueError("%s: 1 or 3 channels are expected, not %d" % (what, v.shape[2]))
    if v.shape[2] < least:
        raise ValueError("%s: at least %d channels are expected, not %d" % (what, least, v.shape[2]))


def record_buffers(scratch_bytes, record_type, n, H, W, device):
    """scratch_bytes: the library's dd_*_scratch_bytes of the launch (a negative status raises its message).  -> (the n records as a uint8
    tensor of zeros, the 8-byte aligned scratch)."""
    nbytes = scratch_bytes(n, H, W)
    if nbytes < 0:
        L.check(int(nbytes))
    return (torch.zeros((n * C.sizeof(record_type),), dtype=torch.uint8, device=device),
            torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device))


def read_records(records, record_type, n):
    """ONE device-to-host copy (a synchronisation) -> the n ctypes records."""
    return (record_type * n).from_buffer_copy(records.cpu().numpy().tobytes())
