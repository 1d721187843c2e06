"""dd_sequence_quality of include/dd_hip.h in numpy (TEST INFRASTRUCTURE ONLY), written from the definition: no tiles, no partial sums.

    rec = record(pred, pred_previous, target, target_previous, motion, sx, sy, thresholds, exposure)

The previous position and what follows from it alone (offscreen, the tap indices and weights) come from temporal_ref.positions, in float32 with
one rounding per operation as the header states them, and the bytes from quality_ref.quantise (an fp32 product against the fp32 table): those
decisions are the kernel's for ANY input.  Every term is float64.  -> the fields of a dd_seqq_record as Python numbers; "S": per sum the
magnitude its fp32 roundings scale with -- scene-referred the sum over valid pixels and channels of |p| + bil(|taps of pred_previous|) + |t| +
bil(|taps of target_previous|), for the ldr sums the same of the bytes; and the [H,W] masks "offscreen", "nonfinite", "valid"."""
import numpy as np

import quality_ref as Q
import temporal_ref as T

COUNTS = ("pixels_offscreen", "pixels_nonfinite", "pixels_valid")
SUMS = ("change_prediction", "change_target", "temporal_error")
LDR_SUMS = ("ldr_change_prediction", "ldr_change_target", "ldr_temporal_error")


def _taps(image, x0, y0):
    H, W = x0.shape
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    return image[y0, x0], image[y0, x1], image[y1, x0], image[y1, x1]


def _bilinear(taps, fx, fy):
    wx, wy = fx[..., None], fy[..., None]
    return (taps[0] * (1 - wx) + taps[1] * wx) * (1 - wy) + (taps[2] * (1 - wx) + taps[3] * wx) * wy


def record(pred, pred_previous, target, target_previous, motion, sx, sy, thresholds, exposure=1.0):
    images = [np.asarray(v) for v in (pred, pred_previous, target, target_previous)]
    assert all(v.dtype == np.float32 and v.shape == images[0].shape and v.ndim == 3 and v.shape[2] in (1, 3) for v in images)
    offscreen, x0, y0, fx, fy, _, _ = T.positions(motion, sx, sy)
    assert offscreen.shape == images[0].shape[:2]
    finite = np.ones(offscreen.shape, dtype=bool)
    for k, v in enumerate(images):
        ok = np.isfinite(v).all(axis=2)
        if k % 2 == 0:                                   # a current image: the pixel itself
            finite &= ok
        else:                                            # a previous image: all four taps, whatever their weights
            for tap in _taps(ok, x0, y0):
                finite &= tap
    nonfinite, valid = ~offscreen & ~finite, ~offscreen & finite
    v3 = np.broadcast_to(valid[..., None], images[0].shape)

    def terms(p, pp, t, tp):
        """[H,W,C] float64 images without non-finite values -> the three sums and S"""
        hp, ht = _bilinear(_taps(pp, x0, y0), fx, fy), _bilinear(_taps(tp, x0, y0), fx, fy)
        dp, dt = p - hp, t - ht
        size = np.abs(p) + _bilinear(_taps(np.abs(pp), x0, y0), fx, fy) + np.abs(t) + _bilinear(_taps(np.abs(tp), x0, y0), fx, fy)
        return [float(np.abs(v)[v3].sum()) for v in (dp, dt, dp - dt)], float(size[v3].sum())
    scene, s_scene = terms(*[np.where(np.isfinite(v), v, np.float32(0)).astype(np.float64) for v in images])
    ldr, s_ldr = terms(*[Q.quantise(v, thresholds, exposure).astype(np.float64) for v in images])
    out = {"pixels_offscreen": int(offscreen.sum()), "pixels_nonfinite": int(nonfinite.sum()), "pixels_valid": int(valid.sum()),
           "offscreen": offscreen, "nonfinite": nonfinite, "valid": valid, "S": {}}
    for names, values, size in ((SUMS, scene, s_scene), (LDR_SUMS, ldr, s_ldr)):
        for name, value in zip(names, values):
            out[name] = value
            out["S"][name] = size
    return out


def figures(rec, channels):
    """What sequence_quality.SequenceQuality.measure reports for one pass, from the record's fields."""
    out = {k: int(rec[k]) for k in COUNTS}
    values = float(out["pixels_valid"] * channels)
    for k in SUMS:
        out[k] = rec[k] / values if values else None
    for k in LDR_SUMS:
        out[k] = rec[k] / values / 255.0 if values else None
    return out


def add_records(records):
    """The fields of several records added (what SequenceQuality.summary() is taken from), S included."""
    out = {k: sum(r[k] for r in records) for k in COUNTS + SUMS + LDR_SUMS}
    out["S"] = {k: sum(r["S"][k] for r in records) for k in SUMS + LDR_SUMS}
    return out


# ---------------------------------------------------------------------------------------------------- the generator of the GPU tests
def make_case(H, W, channels, seed, sprinkle=False):
    """Per pair: target_previous = |N(0,1)|, target = target_previous + 0.2 N, pred_previous = target_previous + 0.1 N, pred = target + 0.1 N
    (bytes over the whole range at exposure 1, a few values below 0); motion on multiples of 1/8 pixel in [-3, 3] (positions, floor and
    weights are exact in fp32).  channels: the channel count of every pair.  sprinkle: NaN / Inf in the motion, in the first pair's pred and
    the last pair's target, in the last pair's pred_previous and the first pair's target_previous.
    -> (preds, pred_previouses, targets, target_previouses, motion [H,W,3])"""
    rng = np.random.default_rng(seed)
    target_previouses = [np.abs(rng.standard_normal((H, W, c))).astype(np.float32) for c in channels]
    targets = [(v + 0.2 * rng.standard_normal(v.shape)).astype(np.float32) for v in target_previouses]
    pred_previouses = [(v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32) for v in target_previouses]
    preds = [(v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32) for v in targets]
    motion = (rng.integers(-24, 25, size=(H, W, 3)) / 8.0).astype(np.float32)
    if H == 1:                                            # (a frame of one row or column: every second pixel stays on it)
        motion[:, ::2, 1] = 0
    if W == 1:
        motion[::2, :, 0] = 0
    if sprinkle and H * W >= 16:
        bad = (np.nan, np.inf, -np.inf)
        for k in range(max(H * W // 100, 3)):
            motion[rng.integers(H), rng.integers(W), rng.integers(2)] = bad[k % 3]
            for j, image in enumerate((preds[0], targets[-1], pred_previouses[-1], target_previouses[0])):
                image[rng.integers(H), rng.integers(W), rng.integers(image.shape[2])] = bad[(k + j + 1) % 3]
        preds[0].view(np.uint32)[rng.integers(H), rng.integers(W), 0] = 0x7fc12345      # a NaN with a payload of its own
    return preds, pred_previouses, targets, target_previouses, motion
