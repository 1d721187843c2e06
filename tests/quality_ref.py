"""Float64 / numpy restatement of dd_frame_quality (include/dd_hip.h) and of quality.FrameQuality.measure, for tests/test_quality_ref.py (CPU)
and tests/test_gpu_quality.py (-m gpu).  Written from the definitions, not from the kernel: no tiles, no separable filter (the 11 x 11
Gaussian is applied as 121 shifted additions of whole images), no partial sums.

    valid pixel   all channels of BOTH images finite; invalid pixels add to nothing
    valid window  all 121 pixels of an 11 x 11 window valid (VALID positions: (H - 10) x (W - 10) windows, none when H < 11 or W < 11)
    scene sums    se = sum (p-t)^2, ae = sum |p-t|, rse = sum (p-t)^2 / (t^2 + eps), smape = sum |p-t| / (|p| + |t| + eps) over valid pixels and
                  channels, in float64 from the fp32 inputs; max_abs = max |p-t|, rounded to fp32 (the record's field is a float; p - t of two
                  fp32 values is exact in float64 and rounding is monotonic, so this IS the maximum of the fp32 differences)
    bytes         the number of fp32 thresholds <= the fp32 product float32(exposure) * value
    ldr_sq_err    sum (b_p - b_t)^2 over valid pixels and channels, an integer
    SSIM          on byte / 255, per channel: Gaussian sigma 1.5, normalised, C1 = 0.01^2, C2 = 0.03^2,
                  (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)); map = mean over channels, NaN at invalid windows
"""
import math

import numpy as np

FILTER_SIZE, FILTER_SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
EPSILON = 1e-2


def gaussian():
    """[11,11] float64, normalised"""
    c = np.arange(FILTER_SIZE, dtype=np.float64) - (FILTER_SIZE - 1) / 2.0
    e = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2.0 * FILTER_SIGMA ** 2))
    return e / e.sum()


def _hwc(a):
    a = np.asarray(a)
    assert a.ndim == 3 and a.shape[2] in (1, 3), a.shape
    return a


def valid_pixels(pred, target):
    """bool [H,W]"""
    return np.isfinite(_hwc(pred)).all(axis=2) & np.isfinite(_hwc(target)).all(axis=2)


def quantise(values, thresholds, exposure=1.0):
    """int64, shape of values: entries of `thresholds` <= float32(exposure) * value, compared in fp32.  Non-finite values give 0 (their pixels
    are invalid and never looked at)."""
    thr = np.asarray(thresholds)
    assert thr.dtype == np.float32 and thr.shape == (255,) and (np.diff(thr) > 0).all()
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(all="ignore"):
        prod = np.where(np.isfinite(v), v, np.float32(0)) * np.float32(exposure)
    assert prod.dtype == np.float32
    return np.searchsorted(thr, prod, side="right").astype(np.int64)


def window_filter(a):
    """[H,W,...] float64 -> [(H-10),(W-10),...]: the normalised Gaussian at every VALID position"""
    g = gaussian()
    H, W = a.shape[:2]
    out = np.zeros((H - FILTER_SIZE + 1, W - FILTER_SIZE + 1) + a.shape[2:], dtype=np.float64)
    for i in range(FILTER_SIZE):
        for j in range(FILTER_SIZE):
            out += g[i, j] * a[i:i + out.shape[0], j:j + out.shape[1]]
    return out


def window_count(flags):
    """[H,W] bool -> [(H-10),(W-10)] int: how many of the window's 121 pixels are set"""
    H, W = flags.shape
    out = np.zeros((H - FILTER_SIZE + 1, W - FILTER_SIZE + 1), dtype=np.int64)
    for i in range(FILTER_SIZE):
        for j in range(FILTER_SIZE):
            out += flags[i:i + out.shape[0], j:j + out.shape[1]]
    return out


def ssim_channels(bp, bt):
    """bytes [H,W,C] -> SSIM of every window and channel [(H-10),(W-10),C], float64"""
    x, y = np.asarray(bp, dtype=np.float64) / 255.0, np.asarray(bt, dtype=np.float64) / 255.0
    c1, c2 = K1 ** 2, K2 ** 2
    mx, my = window_filter(x), window_filter(y)
    sxx, syy, sxy = window_filter(x * x) - mx * mx, window_filter(y * y) - my * my, window_filter(x * y) - mx * my
    return (2.0 * mx * my + c1) * (2.0 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))


def ssim_map(bp, bt, valid):
    """bytes [H,W,C], valid [H,W] -> [(H-10),(W-10)] float64 map (mean over channels), NaN at invalid windows; None without windows"""
    H, W = valid.shape
    if H < FILTER_SIZE or W < FILTER_SIZE:
        return None
    m = ssim_channels(bp, bt).mean(axis=2)
    m[window_count(~valid) > 0] = np.nan
    return m


def record(pred, target, thresholds, exposure=1.0, epsilon=EPSILON):
    """The fields of a dd_quality_record as Python numbers, plus "map" (the SSIM map or None)."""
    pred, target = _hwc(pred), _hwc(target)
    assert pred.shape == target.shape and pred.dtype == np.float32 and target.dtype == np.float32
    valid = valid_pixels(pred, target)
    p, t = pred.astype(np.float64)[valid], target.astype(np.float64)[valid]      # [n, C]
    d = p - t
    bp, bt = quantise(pred, thresholds, exposure), quantise(target, thresholds, exposure)
    m = ssim_map(bp, bt, valid)
    good = None if m is None else ~np.isnan(m)
    db = (bp - bt)[valid]
    return {
        "pixels_valid": int(valid.sum()),
        "windows_valid": 0 if m is None else int(good.sum()),
        "ldr_sq_err": int((db * db).sum()),
        "se": float((d * d).sum()),
        "ae": float(np.abs(d).sum()),
        "rse": float((d * d / (t * t + epsilon)).sum()),
        "smape": float((np.abs(d) / (np.abs(p) + np.abs(t) + epsilon)).sum()),
        "ssim_sum": 0.0 if m is None else float(m[good].sum()),
        "max_abs": float(np.float32(np.abs(d).max())) if d.size else 0.0,
        "map": m,
    }


def summary(rec, H, W, C):
    """What quality.FrameQuality.measure reports for one pair, from the record's fields."""
    n, nw = rec["pixels_valid"], rec["windows_valid"]
    terms = float(n * C)
    out = {"pixels": H * W, "valid_pixels": n, "windows": max(H - 10, 0) * max(W - 10, 0), "valid_windows": nw}
    for key, field in (("mse", "se"), ("mae", "ae"), ("rel_mse", "rse"), ("smape", "smape")):
        out[key] = rec[field] / terms if n else None
    out["max_abs"] = rec["max_abs"] if n else None
    if not n:
        out["psnr_8bit"] = None
    elif rec["ldr_sq_err"] == 0:
        out["psnr_8bit"] = math.inf
    else:
        out["psnr_8bit"] = 10.0 * math.log10(255.0 ** 2 * terms / rec["ldr_sq_err"])
    out["ssim"] = rec["ssim_sum"] / nw if nw else None
    return out


def measure(pred, target, thresholds, exposure=1.0, epsilon=EPSILON):
    pred = _hwc(pred)
    return summary(record(pred, target, thresholds, exposure, epsilon), pred.shape[0], pred.shape[1], pred.shape[2])


# ------------------------------------------------------------------------------------------------------------------ inputs
def radiance_pair(H, W, C, seed):
    """(prediction, target) fp32 [H,W,C] with a wide dynamic range: target = exp(1.5 N), a fifth of its pixels exactly 0 and a few per cent
    negative; prediction = target (1 + 0.2 N) + 0.05 N."""
    rng = np.random.default_rng(seed)
    t = np.exp(1.5 * rng.standard_normal((H, W, C)))
    t[rng.random((H, W)) < 0.2] = 0.0
    neg = rng.random((H, W, C)) < 0.03
    t[neg] = -0.1 * t[neg]
    p = t * (1.0 + 0.2 * rng.standard_normal((H, W, C))) + 0.05 * rng.standard_normal((H, W, C))
    return p.astype(np.float32), t.astype(np.float32)


def flat_bright_pair(H, W, C, seed, thresholds, level=0.9):
    """target: the constant `level`; prediction: values whose bytes are the target's byte -1, +0 or +1 (drawn per channel)"""
    thr = np.asarray(thresholds, dtype=np.float32)
    rng = np.random.default_rng(seed)
    t = np.full((H, W, C), level, dtype=np.float32)
    b = int(np.searchsorted(thr, np.float32(level), side="right"))
    assert 2 <= b <= 253
    mid = ((thr[b - 2:b + 1].astype(np.float64) + thr[b - 1:b + 2].astype(np.float64)) / 2).astype(np.float32)      # values of bytes b-1, b, b+1
    p = mid[rng.integers(0, 3, size=(H, W, C))]
    return p.astype(np.float32), t
