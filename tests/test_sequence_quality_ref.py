"""tests/sequence_quality_ref.py (the numpy definition of dd_sequence_quality) against closed forms.  The images hold multiples of 1/64 and the
motions whole pixels, so every expected figure is exact.  Every record also goes through the host's sequence_quality.figures, which must report
what the reference's figures() reports."""
import numpy as np

import sequence_quality_ref as R
from deepdenoiser_amd import metrics, sequence_quality

H, W = 12, 17
SX, SY = -1.0, 1.0


def _dyadic(rng, shape, scale=64.0):
    return (rng.integers(0, 256, size=shape) / scale).astype(np.float32)


def _record(*args):
    r = R.record(*args)
    for channels in (1, 3):
        assert sequence_quality.figures({k: r[k] for k in R.COUNTS + R.SUMS + R.LDR_SUMS}, channels) == R.figures(r, channels)
    return r


def _motion(dx, dy):
    """the motion pass that puts the previous position of every pixel at (x + dx, y + dy) under the scale (SX, SY)"""
    m = np.zeros((H, W, 3), dtype=np.float32)
    m[..., 0], m[..., 1] = dx / SX, dy / SY
    return m


def test_a_prediction_that_brightens_over_a_static_target():
    rng = np.random.default_rng(1)
    thr = metrics.preview_thresholds()
    for C, c in ((3, 0.25), (1, -0.5)):
        pp, t = _dyadic(rng, (H, W, C)), _dyadic(rng, (H, W, C))
        p = (pp + np.float32(c)).astype(np.float32)
        r = _record(p, pp, t, t, _motion(0, 0), SX, SY, thr)
        assert (r["pixels_offscreen"], r["pixels_nonfinite"], r["pixels_valid"]) == (0, 0, H * W)
        f = R.figures(r, C)
        assert f["change_prediction"] == abs(c) and f["temporal_error"] == abs(c) and f["change_target"] == 0.0
        assert f["ldr_change_target"] == 0.0 and f["ldr_change_prediction"] == f["ldr_temporal_error"]
        assert r["S"]["temporal_error"] == float((np.abs(p) + np.abs(pp) + 2 * np.abs(t)).astype(np.float64).sum())


def test_a_static_bias_has_no_temporal_error():
    rng = np.random.default_rng(2)
    thr = metrics.preview_thresholds()
    tp, t = _dyadic(rng, (H, W, 3)), _dyadic(rng, (H, W, 3))
    bias = np.float32(0.375)
    for dx, dy in ((0, 0), (2, -1), (-3, 2)):
        r = _record(t + bias, tp + bias, t, tp, _motion(dx, dy), SX, SY, thr)
        assert r["pixels_valid"] == (W - abs(dx)) * (H - abs(dy)) and r["pixels_nonfinite"] == 0
        assert r["temporal_error"] == 0.0 and r["change_prediction"] > 0.0 and r["change_prediction"] == r["change_target"]


def test_a_frame_that_only_moves_does_not_change():
    rng = np.random.default_rng(3)
    thr = metrics.preview_thresholds()
    for dx, dy in ((1, 0), (0, -2), (3, 2), (-2, -3)):
        pp, tp = _dyadic(rng, (H + 6, W + 6, 3)), _dyadic(rng, (H + 6, W + 6, 3))
        # current(x, y) = previous(x + dx, y + dy) wherever that is on the frame (the frames are windows of larger images)
        p, t = pp[3 + dy:3 + dy + H, 3 + dx:3 + dx + W], tp[3 + dy:3 + dy + H, 3 + dx:3 + dx + W]
        r = _record(np.ascontiguousarray(p), np.ascontiguousarray(pp[3:3 + H, 3:3 + W]), np.ascontiguousarray(t), np.ascontiguousarray(tp[3:3 + H, 3:3 + W]),
                     _motion(dx, dy), SX, SY, thr)
        assert r["pixels_offscreen"] == H * W - (W - abs(dx)) * (H - abs(dy)) and r["pixels_nonfinite"] == 0
        assert r["pixels_offscreen"] + r["pixels_valid"] == H * W
        for k in R.SUMS + R.LDR_SUMS:
            assert r[k] == 0.0, k
        assert r["S"]["temporal_error"] > 0.0 and r["S"]["ldr_temporal_error"] > 0.0


def test_a_nan_moves_exactly_the_pixels_that_read_it():
    rng = np.random.default_rng(4)
    thr = metrics.preview_thresholds()
    images = [_dyadic(rng, (H, W, 3)) for _ in range(4)]
    clean = _record(*images, _motion(1, 2), SX, SY, thr)
    assert clean["pixels_nonfinite"] == 0
    row, col = 6, 8
    for which, value in ((1, np.nan), (3, np.inf)):                                  # pred_previous, target_previous
        bad = [v.copy() for v in images]
        bad[which][row, col, 1] = value
        r = _record(*bad, _motion(1, 2), SX, SY, thr)
        # whole-pixel motion: the taps of pixel (x, y) are (x + 1 .. x + 2, y + 2 .. y + 3), the second ones with weight 0 -- they still count
        want = np.zeros((H, W), dtype=bool)
        want[row - 3:row - 1, col - 2:col] = True
        assert np.array_equal(r["nonfinite"], want) and r["pixels_nonfinite"] == 4
        assert r["pixels_offscreen"] == clean["pixels_offscreen"] and r["pixels_valid"] == clean["pixels_valid"] - 4
        assert np.isfinite([r[k] for k in R.SUMS + R.LDR_SUMS]).all()
    # half-pixel motion: all four taps carry weight
    half = _motion(0, 0)
    half[..., 0], half[..., 1] = 0.5 / SX, 0.5 / SY
    bad = [v.copy() for v in images]
    bad[1][row, col, 0] = -np.inf
    r = _record(*bad, half, SX, SY, thr)
    want = np.zeros((H, W), dtype=bool)
    want[row - 1:row + 1, col - 1:col + 1] = True
    assert np.array_equal(r["nonfinite"], want)
    # in a current image: the pixel alone; an offscreen pixel stays offscreen
    bad = [v.copy() for v in images]
    bad[0][row, col, 2] = np.nan
    bad[2][0, W - 1, 0] = np.nan                                                     # (its previous position x + 1 is outside)
    r = _record(*bad, _motion(1, 2), SX, SY, thr)
    want = np.zeros((H, W), dtype=bool)
    want[row, col] = True
    assert np.array_equal(r["nonfinite"], want) and r["pixels_offscreen"] == clean["pixels_offscreen"]
