"""Temporal stabilisation of a denoised frame sequence (csrc/dd_temporal.hip, include/dd_hip.h: dd_temporal_stabilize).

    stabilizer = TemporalStabilizer(device, guides=(("Normal", 0.25),))
    for frame in frames:                                             # in display order
        predictions = predictor.predict_frame(frame.features)       # without the recombined entries
        stable = stabilizer.stabilize(predictions, frame.motion, {"Normal": frame.normal})
        figures = stabilizer.report()                                # one copy of the records: the only synchronisation

Every frame is denoised on its own, so the filter kernels predicted for a pixel change with the noise from frame to frame and a denoised
animation flickers.  The stabiliser blends every pass of a frame with the stabilised previous frame, fetched along the motion vectors
(bilinear), after clamping that history to mean +- gamma * standard deviation of the current frame's 3 x 3 neighbourhood; pixels whose
previous position is outside the frame, whose guide passes (normal, depth, ...) changed by more than a tolerance, or that meet a NaN / Inf
keep the current value bit for bit.  One launch for all passes of a frame and no host synchronisation.  The reference has no such step.

alpha = 0.8 and gamma = 1.0 are choices, not measured optima.  The default motion_scale (-1, +1) encodes this reading of Cycles' Vector
pass: X, Y = current raster position minus previous raster position, in pixels, and raster y points up while rows count down.  It has not
been checked against a render (there is no Blender on the build machine); that is why it is an option."""
import math
import os
import re

import torch

from . import _lib as L
from . import frame_launch

COUNTS = ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended", "values_clamped")
SUMS = ("change", "flicker_before", "flicker_after")


def parse_guide(text):
    """'Pass:tolerance' of --temporal_guide -> (pass name, tolerance); ValueError for anything else."""
    name, colon, tolerance = str(text).rpartition(":")
    try:
        value = float(tolerance)
    except ValueError:
        value = math.nan
    if not colon or not name or not (math.isfinite(value) and value >= 0.0):
        raise ValueError("a guide is 'Pass:tolerance' with a finite tolerance >= 0, not %r" % (text,))
    return name, value


def frame_directories(parent):
    """--input_sequence: the sub-directories of `parent` that hold .exr files, ordered by the integers in their names, then by name
    (f2 before f10)."""
    found = []
    for name in os.listdir(parent):
        path = os.path.join(parent, name)
        if os.path.isdir(path) and any(n.endswith(".exr") for n in os.listdir(path)):
            found.append((tuple(int(d) for d in re.findall(r"\d+", name)), name, path))
    return [path for _, _, path in sorted(found)]


class TemporalStabilizer:
    def __init__(self, device, alpha=0.8, gamma=1.0, motion_scale=None, guides=()):
        """alpha: the weight of the (clamped) history in a blended pixel, 0 .. 1.  gamma >= 0: the clamp's half width in standard deviations of
        the 3 x 3 neighbourhood.  Both defaults are choices, not measured optima.  motion_scale (sx, sy): previous position = (x + sx * motion
        channel 0, y + sy * motion channel 1); the default, frame_launch.MOTION_SCALE = (-1, +1), is an unverified reading of Cycles' Vector pass (the module's docstring).  guides:
        a sequence of (pass name, tolerance), at most 4: a pixel whose guide pass differs from the previous frame's at the nearest previous
        pixel by more than the tolerance in any channel is not blended."""
        self.alpha, self.gamma = float(alpha), float(gamma)
        if not 0.0 <= self.alpha <= 1.0:
            raise ValueError("alpha must be 0 .. 1, not %r" % (alpha,))
        if not (self.gamma >= 0.0 and math.isfinite(self.gamma)):
            raise ValueError("gamma must be finite and >= 0, not %r" % (gamma,))
        self.motion_scale = frame_launch.motion_scale(motion_scale)
        self.guides = tuple((str(name), float(tolerance)) for name, tolerance in guides)
        if len(self.guides) > L.TEMPORAL_MAX_GUIDES:
            raise ValueError("at most %d guides are expected, not %d" % (L.TEMPORAL_MAX_GUIDES, len(self.guides)))
        for name, tolerance in self.guides:
            if not (tolerance >= 0.0 and math.isfinite(tolerance)):
                raise ValueError("guide %s: the tolerance must be finite and >= 0, not %r" % (name, tolerance))
        self.lib = L.load()
        self.device = torch.empty(0, device=torch.device(device)).device      # (with its index: what the tensors of a frame are compared with)
        self.launches = 0
        self.reset()

    def reset(self):
        """Forget the history: the next frame passes through unchanged and becomes the history."""
        self._signature, self._names = None, []
        self._sets, self._front, self._guide_previous, self._records, self._scratch = None, 0, {}, None, None

    def parameters(self):
        return {"alpha": self.alpha, "gamma": self.gamma, "motion_scale": list(self.motion_scale), "guides": [list(g) for g in self.guides]}

    def stabilize(self, predictions, motion, guide_frames=None):
        """predictions: {name: float32 [H,W,C] device tensor, C 1 or 3} (what Predictor.predict_frame returns, without the recombined entries);
        motion: the [H,W,>=2] tensor of the frame; guide_frames: {guide pass: [H,W,C] tensor} for every guide.  -> the same keys with the
        stabilised [H,W,C] tensors: the stabiliser's own buffers, valid until the call after the next one.  The first frame, a frame after
        reset(), a changed frame size or a changed key set passes through unchanged with no launch and becomes the history.  One
        dd_temporal_stabilize call on the current stream, no synchronisation."""
        names = list(predictions)
        if not 1 <= len(names) <= L.TEMPORAL_MAX_PASSES:
            raise ValueError("1 .. %d passes are expected, not %d" % (L.TEMPORAL_MAX_PASSES, len(names)))
        first = predictions[names[0]]
        if not torch.is_tensor(first) or first.dim() != 3:
            raise ValueError("%s must be a float32 [H,W,C] tensor" % names[0])
        H, W = int(first.shape[0]), int(first.shape[1])
        for n in names:
            frame_launch.check_frame(n, predictions[n], H, W, self.device, channels=(1, 3))
        frame_launch.check_frame("motion", motion, H, W, self.device, least=2)
        guide_frames = guide_frames or {}
        for g, _ in self.guides:
            if g not in guide_frames:
                raise ValueError("no frame for the guide pass %s" % g)
            frame_launch.check_frame("guide %s" % g, guide_frames[g], H, W, self.device, channels=(1, 3))
        signature = (H, W, tuple((n, int(predictions[n].shape[2])) for n in names), tuple(int(guide_frames[g].shape[2]) for g, _ in self.guides))
        if signature != self._signature:
            self._start(signature, names, predictions, guide_frames)
            return dict(self._sets[self._front])
        history, out = self._sets[self._front], self._sets[1 - self._front]
        table = (L.TemporalPass * len(names))()
        for i, n in enumerate(names):
            p, h, o = predictions[n], history[n], out[n]
            table[i] = L.TemporalPass(p.data_ptr(), h.data_ptr(), o.data_ptr(), p.stride(1), h.stride(1), o.stride(1), p.shape[2])
        guides = (L.TemporalGuide * max(len(self.guides), 1))()
        for i, (g, tolerance) in enumerate(self.guides):
            c, p = guide_frames[g], self._guide_previous[g]
            guides[i] = L.TemporalGuide(c.data_ptr(), p.data_ptr(), c.stride(1), p.stride(1), c.shape[2], tolerance)
        L.check(self.lib.dd_temporal_stabilize(table, len(names), guides, len(self.guides), H, W, motion.data_ptr(), motion.stride(1),
                                               self.motion_scale[0], self.motion_scale[1], self.alpha, self.gamma, self._records.data_ptr(),
                                               self._scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self.launches += 1
        for g, _ in self.guides:                      # (behind the launch on the same stream: it has read the previous frame's guides)
            self._guide_previous[g].copy_(guide_frames[g])
        self._front = 1 - self._front
        return dict(out)

    def _start(self, signature, names, predictions, guide_frames):
        """A new sequence: two sets of frame buffers, the records (zero: nothing was blended) and the scratch; the frame becomes the history."""
        H, W = signature[:2]
        self._signature, self._names, self._front = signature, names, 0
        self._sets = [{n: torch.empty((H, W, predictions[n].shape[2]), dtype=torch.float32, device=self.device) for n in names} for _ in range(2)]
        for n in names:
            self._sets[0][n].copy_(predictions[n])
        self._guide_previous = {g: guide_frames[g].clone(memory_format=torch.contiguous_format) for g, _ in self.guides}
        self._records, self._scratch = frame_launch.record_buffers(self.lib.dd_temporal_scratch_bytes, L.TemporalRecord, len(names), H, W, self.device)

    def report(self):
        """ONE device-to-host copy of the records of the last frame -> {name: {the five counts, "change", "flicker_before", "flicker_after"}}: the
        last three are means per blended value (pixels_blended * channels), None when nothing was blended (a frame that passed through)."""
        if self._records is None:
            raise RuntimeError("report() needs a frame: call stabilize() first")
        recs = frame_launch.read_records(self._records, L.TemporalRecord, len(self._names))
        return {n: figures(recs[i], channels) for i, (n, channels) in enumerate(self._signature[2])}


def figures(rec, channels):
    """A dd_temporal_record -> the dictionary of report()."""
    out = {k: int(getattr(rec, k)) for k in COUNTS}
    values = float(out["pixels_blended"] * channels)
    for k in SUMS:
        out[k] = float(getattr(rec, k)) / values if values else None
    return out
