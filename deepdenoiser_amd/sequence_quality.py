"""Does a denoised sequence flicker against its ground truth?  The temporal error of every pass of a frame sequence against its target frames,
computed where the frames are (csrc/dd_sequence_quality.hip, include/dd_hip.h: dd_sequence_quality).

    scorer = SequenceQuality(device, exposure=1.0, motion_scale=(-1.0, 1.0))
    for frame in frames:                                             # in display order
        figures = scorer.measure(predictions, targets, frame.motion)     # None for the first frame: it becomes the history
    scorer.summary()                                                 # the same figures over all measured frames

With the error image E = P - T of a frame, the figure temporal_error is the mean of |E_t(x) - warp(E_t-1)(x)| over the valid values: the previous
frame is fetched along the current frame's motion vectors (bilinear), exactly as the stabiliser fetches its history (temporal.py).  A static
bias gives 0, error that changes from frame to frame (boiling) a large figure, and a filter that smears everything does NOT improve it: its
prediction follows the target's own change (change_target) less well.  change_prediction and change_target are the means of |P_t - warp(P_t-1)|
and |T_t - warp(T_t-1)|; with the wrong motion convention change_target explodes.  The ldr_ figures are the same on the 8-bit sRGB bytes of
`exposure * value` (metrics.preview_thresholds), divided by 255.  A pixel whose previous position lies outside the frame (offscreen) or that
reads a NaN / Inf in one of the four images (nonfinite) adds to nothing."""
import math

import numpy as np
import torch

from . import _lib as L
from . import frame_launch
from . import metrics as M

COUNTS = ("pixels_offscreen", "pixels_nonfinite", "pixels_valid")
SUMS = ("change_prediction", "change_target", "temporal_error")
LDR_SUMS = ("ldr_change_prediction", "ldr_change_target", "ldr_temporal_error")


class SequenceQuality:
    def __init__(self, device, exposure=1.0, motion_scale=None):
        """exposure: the factor in front of the 8-bit quantisation of the ldr_ figures.  motion_scale (sx, sy): previous position = (x + sx *
        motion channel 0, y + sy * motion channel 1); the default is the stabiliser's (frame_launch.MOTION_SCALE, temporal.py: an unverified reading of Cycles' Vector
        pass)."""
        self.exposure = float(exposure)
        if not math.isfinite(self.exposure):
            raise ValueError("exposure must be finite, not %r" % (exposure,))
        self.motion_scale = frame_launch.motion_scale(motion_scale)
        self.lib = L.load()
        self._thresholds = torch.from_numpy(M.preview_thresholds()).to(torch.device(device))
        self.device = self._thresholds.device      # (with its index: what the tensors of a frame are compared with)
        self.launches = 0
        self._totals = {}                          # name -> [channels, frames, {field: sum of the raw records}]
        self.reset()

    def reset(self):
        """Forget the history: the next frame is not measured and becomes the history.  summary() keeps what was measured."""
        self._signature, self._previous, self._records, self._scratch = None, None, None, None

    def measure(self, predictions, targets, motion):
        """predictions, targets: {name: float32 [H,W,C] device tensor, C 1 or 3}; every prediction is scored against the target of its name (a
        ValueError names the ones without).  motion: the [H,W,>=2] tensor of THIS frame.  ONE dd_sequence_quality call on the current stream,
        then the frame is copied into the object's own previous-frame buffers behind the launch, then ONE device-to-host copy (the records: the
        only synchronisation).  -> {name: figures}; None for the first frame, after reset() and after a changed frame size or key set: that
        frame becomes the history with no launch."""
        names = list(predictions)
        missing = [n for n in names if n not in targets]
        if missing:
            raise ValueError("no target for %s" % ", ".join(missing))
        if not 1 <= len(names) <= L.SEQQ_MAX_PAIRS:
            raise ValueError("1 .. %d passes are expected, not %d" % (L.SEQQ_MAX_PAIRS, len(names)))
        first = predictions[names[0]]
        if not torch.is_tensor(first) or first.dim() != 3:
            raise ValueError("%s must be a float32 [H,W,C] tensor" % names[0])
        H, W = int(first.shape[0]), int(first.shape[1])
        for n in names:
            frame_launch.check_frame(n, predictions[n], H, W, self.device, channels=(1, 3))
            frame_launch.check_frame("the target of %s" % n, targets[n], H, W, self.device, channels=(1, 3))
            if targets[n].shape[2] != predictions[n].shape[2]:
                raise ValueError("%s has %d channels, its target %d" % (n, predictions[n].shape[2], targets[n].shape[2]))
        frame_launch.check_frame("motion", motion, H, W, self.device, least=2)
        signature = (H, W, tuple((n, int(predictions[n].shape[2])) for n in names))
        if signature != self._signature:
            self._start(signature, names, predictions, targets)
            return None
        self._launch(names, predictions, targets, motion)
        for n in names:                               # (behind the launch on the same stream: it has read the previous frame)
            self._previous[n][0].copy_(predictions[n])
            self._previous[n][1].copy_(targets[n])
        recs = frame_launch.read_records(self._records, L.SequenceQualityRecord, len(names))
        out = {}
        for i, (n, channels) in enumerate(signature[2]):
            total = self._totals.setdefault(n, [channels, 0, {k: 0 for k in COUNTS + SUMS + LDR_SUMS}])
            if total[0] != channels:                  # (a name that comes back with another channel count starts again)
                total[:] = [channels, 0, {k: 0 for k in COUNTS + SUMS + LDR_SUMS}]
            total[1] += 1
            for k in COUNTS:
                total[2][k] += int(getattr(recs[i], k))
            for k in SUMS + LDR_SUMS:
                total[2][k] = float(np.float64(total[2][k]) + np.float64(getattr(recs[i], k)))
            out[n] = figures(recs[i], channels)
        return out

    def _launch(self, names, predictions, targets, motion):
        """The dd_sequence_quality call of a validated frame against the history, on the current stream: nothing else, no synchronisation."""
        H, W = self._signature[:2]
        table = (L.SequenceQualityPair * len(names))()
        for i, n in enumerate(names):
            p, t = predictions[n], targets[n]
            pp, tp = self._previous[n]
            table[i] = L.SequenceQualityPair(p.data_ptr(), pp.data_ptr(), t.data_ptr(), tp.data_ptr(), p.stride(1), pp.stride(1), t.stride(1), tp.stride(1),
                                             p.shape[2])
        L.check(self.lib.dd_sequence_quality(table, len(names), H, W, motion.data_ptr(), motion.stride(1), self.motion_scale[0], self.motion_scale[1],
                                             self._thresholds.data_ptr(), self.exposure, self._records.data_ptr(), self._scratch.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
        self.launches += 1

    def _start(self, signature, names, predictions, targets):
        """A new sequence: dense previous-frame buffers of the object's own (the predictor's and the stabiliser's outputs are reused by later
        frames), the records and the scratch; the frame becomes the history."""
        H, W = signature[:2]
        self._signature = signature
        self._previous = {n: (predictions[n].clone(memory_format=torch.contiguous_format), targets[n].clone(memory_format=torch.contiguous_format))
                          for n in names}
        self._records, self._scratch = frame_launch.record_buffers(self.lib.dd_sequence_quality_scratch_bytes, L.SequenceQualityRecord, len(names), H, W,
                                                                   self.device)

    def summary(self):
        """-> {name: the figures of measure() from the raw records of all measured frames added in float64 (frames weigh by their valid values),
        and "frames": how many were measured}.  Empty before the first measured frame."""
        return {n: dict(figures(sums, channels), frames=frames) for n, (channels, frames, sums) in self._totals.items()}


def figures(rec, channels):
    """A dd_seqq_record (or a dictionary of its fields) -> the dictionary of measure(): the three counts; the sums as means per valid value
    (pixels_valid * channels), the ldr_ ones divided by 255 as well; None instead of a mean when no pixel is valid."""
    get = rec.get if isinstance(rec, dict) else lambda k: getattr(rec, k)      # noqa: E731
    out = {k: int(get(k)) for k in COUNTS}
    values = float(out["pixels_valid"] * channels)
    for k in SUMS:
        out[k] = float(get(k)) / values if values else None
    for k in LDR_SUMS:
        out[k] = float(get(k)) / values / 255.0 if values else None
    return out


COLUMNS = SUMS + LDR_SUMS


def table_lines(result):
    """One line per pass: the six means and the pixels that were left out (offscreen + nonfinite)."""
    def cell(v):
        return "%21s" % "-" if v is None else "%21.6g" % v
    width = max([len(n) for n in result] + [4])
    lines = ["%-*s %s %10s" % (width, "pass", " ".join("%21s" % c for c in COLUMNS), "left out")]
    for name, r in result.items():
        lines.append("%-*s %s %10d" % (width, name, " ".join(cell(r[c]) for c in COLUMNS), r["pixels_offscreen"] + r["pixels_nonfinite"]))
    return lines
