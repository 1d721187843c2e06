"""tests/quality_ref.py (the float64 restatement dd_frame_quality is gated against) checked against independent facts: closed forms on flat
images, the quantiser of tests/preview_ref.py, the level-0 SSIM of tests/msssim_ref.py, and the counting of invalid pixels and windows."""
import math

import numpy as np
import torch

import msssim_ref
import preview_ref
import quality_ref as R
from deepdenoiser_amd import metrics as M

THR = M.preview_thresholds()


def _value_of_byte(b):
    """an fp32 value whose byte is b (1 <= b <= 254): the middle of its threshold interval"""
    return np.float32((float(THR[b - 1]) + float(THR[b])) / 2)


def test_flat_images_have_the_closed_form():
    H, W = 14, 19
    for C in (1, 3):
        for a, b in ((200, 190), (17, 17), (1, 254), (230, 231)):
            p = np.full((H, W, C), _value_of_byte(a), dtype=np.float32)
            t = np.full((H, W, C), _value_of_byte(b), dtype=np.float32)
            assert (R.quantise(p, THR) == a).all() and (R.quantise(t, THR) == b).all()
            rec = R.record(p, t, THR)
            c1 = 0.01 ** 2
            want = (2.0 * a * b / 255.0 ** 2 + c1) / ((a * a + b * b) / 255.0 ** 2 + c1)
            assert rec["map"].shape == (H - 10, W - 10)
            assert np.abs(rec["map"] - want).max() <= 1e-9          # (sigma_xy, sigma_x^2, sigma_y^2 vanish up to rounding against C2)
            assert rec["ldr_sq_err"] == (a - b) ** 2 * H * W * C
            assert rec["pixels_valid"] == H * W and rec["windows_valid"] == (H - 10) * (W - 10)
            d = float(p[0, 0, 0]) - float(t[0, 0, 0])
            assert math.isclose(rec["se"], d * d * H * W * C, rel_tol=1e-12) and rec["max_abs"] == float(np.float32(abs(d)))


def test_identical_images():
    p, _ = R.radiance_pair(20, 23, 3, 1)
    got = R.measure(p, p.copy(), THR)
    assert got["mse"] == 0.0 and got["mae"] == 0.0 and got["rel_mse"] == 0.0 and got["smape"] == 0.0 and got["max_abs"] == 0.0
    assert got["psnr_8bit"] == math.inf and abs(got["ssim"] - 1.0) <= 1e-12
    assert np.abs(R.record(p, p.copy(), THR)["map"] - 1.0).max() <= 1e-12


def test_bytes_are_those_of_the_preview_quantiser():
    rng = np.random.default_rng(3)
    v = np.concatenate([np.exp(2.0 * rng.standard_normal(4000)) * 0.2, -rng.random(50), [0.0, 1.0, 1e9, float(THR[0]), float(THR[254]), float(THR[100])],
                        np.nextafter(THR, np.float32(-1)), np.nextafter(THR, np.float32(2))]).astype(np.float32).reshape(-1, 1, 1)
    v = np.repeat(v, 3, axis=2)
    assert np.array_equal(R.quantise(v, THR), preview_ref.quantise(v.astype(np.float64), THR).astype(np.int64))
    # with an exposure the product is formed in fp32, as the device forms it
    e = np.float32(1.7)
    assert np.array_equal(R.quantise(v, THR, 1.7), preview_ref.quantise((v * e).astype(np.float64), THR).astype(np.int64))
    assert R.quantise(np.float32([[[np.inf]]]), THR)[0, 0, 0] == 0 and R.quantise(np.float32([[[np.nan]]]), THR)[0, 0, 0] == 0      # (invalid: never used)


def test_single_level_ssim_is_the_level_0_of_the_ms_ssim_reference():
    p, t = R.radiance_pair(24, 31, 3, 7)
    bp, bt = R.quantise(p, THR), R.quantise(t, THR)
    x = torch.from_numpy(bp.astype(np.float64) / 255.0)[None]
    y = torch.from_numpy(bt.astype(np.float64) / 255.0)[None]
    ssim, _ = msssim_ref.ssim_per_channel(x, y)                       # [1, 3]: the mean over the VALID positions, per channel
    ours = R.ssim_channels(bp, bt)
    assert ours.shape == (14, 21, 3)
    assert np.abs(ours.mean(axis=(0, 1)) - ssim[0].numpy()).max() <= 1e-12
    rec = R.record(p, t, THR)
    assert abs(rec["ssim_sum"] / rec["windows_valid"] - float(ssim.mean())) <= 1e-12
    assert np.abs(R.gaussian() - msssim_ref.fspecial_gauss().numpy()).max() <= 1e-15 and abs(R.gaussian().sum() - 1.0) <= 1e-15


def test_a_planted_nan_removes_one_pixel_and_its_windows():
    H, W, C = 30, 37, 3
    p, t = R.radiance_pair(H, W, C, 9)
    full = R.record(p, t, THR)
    assert full["pixels_valid"] == H * W and full["windows_valid"] == (H - 10) * (W - 10)
    for (y, x), windows_lost in (((15, 18), 121), ((0, 0), 1), ((H - 1, W - 1), 1), ((0, 18), 11), ((3, 2), 4 * 3)):
        for side in (0, 1):
            q = [p.copy(), t.copy()]
            q[side][y, x, 1] = np.nan if side == 0 else np.inf
            rec = R.record(q[0], q[1], THR)
            assert rec["pixels_valid"] == H * W - 1 and rec["windows_valid"] == (H - 10) * (W - 10) - windows_lost
            assert int(np.isnan(rec["map"]).sum()) == windows_lost
            # the sums are those of the clean pair without that pixel
            d = p[y, x].astype(np.float64) - t[y, x].astype(np.float64)
            assert math.isclose(rec["se"], full["se"] - float((d * d).sum()), rel_tol=1e-12)
            db = R.quantise(p[y, x][None, None], THR) - R.quantise(t[y, x][None, None], THR)
            assert rec["ldr_sq_err"] == full["ldr_sq_err"] - int((db * db).sum())
            keep = ~np.isnan(rec["map"])
            assert np.array_equal(rec["map"][keep], full["map"][keep])
    none = R.record(np.full((12, 12, 1), np.nan, dtype=np.float32), np.zeros((12, 12, 1), dtype=np.float32), THR)
    assert none["pixels_valid"] == 0 and none["windows_valid"] == 0 and none["se"] == 0.0 and none["ssim_sum"] == 0.0 and none["max_abs"] == 0.0
    s = R.summary(none, 12, 12, 1)
    assert s["ssim"] is None and s["mse"] is None and s["psnr_8bit"] is None and s["pixels"] == 144


def test_frames_without_a_window_and_the_inputs():
    p, t = R.radiance_pair(10, 64, 3, 2)
    got = R.measure(p, t, THR)
    assert got["windows"] == 0 and got["valid_windows"] == 0 and got["ssim"] is None and got["mse"] > 0
    zero = (t == 0).all(axis=2).mean()
    assert 0.1 < zero < 0.3 and (t < 0).any() and t.max() / np.abs(t[t != 0]).min() > 1e3
    fp, ft = R.flat_bright_pair(20, 20, 3, 1, THR)
    db = R.quantise(fp, THR) - R.quantise(ft, THR)
    assert set(np.unique(db)) == {-1, 0, 1} and (ft == np.float32(0.9)).all()
