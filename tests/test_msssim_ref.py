"""Pins the MS-SSIM reference of the tests (tests/msssim_ref.py) against itself and against closed forms, and the C-ABI of the new entries
without a GPU (argument validation only: nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import msssim_ref as R
from deepdenoiser_amd import _lib


def _pair(seed, B, H, W, sigma=0.2):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(B, H, W, 3, generator=g, dtype=torch.float64)
    x = y + sigma * torch.randn(B, H, W, 3, generator=g, dtype=torch.float64)
    return x, y


@pytest.mark.parametrize("seed,B,H,W", [(0, 2, 44, 44), (1, 1, 48, 52), (2, 1, 44, 60)])
def test_torch_version_equals_numpy_loops(seed, B, H, W):
    x, y = _pair(seed, B, H, W)
    got, want = R.ms_ssim(x, y).numpy(), R.ms_ssim_numpy(x.numpy(), y.numpy())
    assert np.abs(got - want).max() < 1e-12


def test_identical_tensors_give_one_and_a_zero_term():
    x, _ = _pair(3, 2, 48, 48)
    assert torch.allclose(R.ms_ssim(x, x), torch.ones(2, dtype=torch.float64), atol=1e-14, rtol=0)
    assert abs(float(R.ms_ssim_term(x, x, 0.7))) < 1e-14


def test_constant_images_closed_form():
    a, b = 0.3, 0.6
    x, y = torch.full((1, 48, 48, 3), a, dtype=torch.float64), torch.full((1, 48, 48, 3), b, dtype=torch.float64)
    c1 = 0.01 ** 2
    want = ((2 * a * b + c1) / (a * a + b * b + c1)) ** 0.3001      # cs_0 = cs_1 = 1; ssim_2 = the luminance term
    assert abs(want - 0.93524316714) < 1e-10
    assert abs(float(R.ms_ssim(x, y)[0]) - want) < 1e-12


def test_gaussian_sums_to_one_and_is_separable():
    g = R.fspecial_gauss()
    assert abs(float(g.sum()) - 1.0) < 1e-15
    m = g.sum(dim=1)
    m = m / m.sum()
    assert float((g - m.reshape(-1, 1) * m.reshape(1, -1)).abs().max()) < 1e-15


def checkerboard(H, W):
    s = ((torch.arange(H).reshape(-1, 1) + torch.arange(W).reshape(1, -1)) % 2).to(torch.float64) * 2 - 1
    s = s.reshape(1, H, W, 1).expand(1, H, W, 3)
    return 0.5 + 0.3 * s, 0.5 - 0.3 * s


def test_checkerboard_pair_is_clamped_at_level_0():
    x, y = checkerboard(48, 48)
    f = R.ms_ssim_factors(x, y)
    assert torch.equal(f[..., 0], torch.zeros(1, 3, dtype=torch.float64))      # anti-correlated: cs_0 < 0, relu -> 0
    assert float((f[..., 1:] - 1).abs().max()) < 1e-12                          # the 2x2 pool of a checkerboard is flat
    assert float(R.ms_ssim(x, y)[0]) == 0.0


def test_term_is_weight_times_one_minus_batch_mean():
    x, y = _pair(4, 3, 44, 44)
    assert abs(float(R.ms_ssim_term(x, y, 0.25)) - 0.25 * (1 - float(R.ms_ssim(x, y).mean()))) < 1e-15


# ---------------------------------------------------------------------------------------------------------------- C-ABI, no GPU
def test_msssim_symbols_exported(lib):
    for n in ("dd_loss_msssim_scratch_bytes", "dd_loss_msssim_fwd", "dd_loss_msssim_bwd"):
        assert hasattr(lib, n), n
        assert n in _lib.SYMBOLS


def test_msssim_scratch_size(lib):
    a, b = lib.dd_loss_msssim_scratch_bytes(1, 64, 64, 1), lib.dd_loss_msssim_scratch_bytes(4, 64, 64, 1)
    assert 0 < a < b
    assert lib.dd_loss_msssim_scratch_bytes(4, 64, 64, 3) > b
    assert lib.dd_loss_msssim_scratch_bytes(4, 64, 96, 1) > b
    for B, H, W, n in ((0, 64, 64, 1), (1, 0, 64, 1), (1, 64, -4, 1), (1, 66, 64, 1), (1, 64, 62, 1), (1, 40, 64, 1), (1, 64, 40, 1), (1, 64, 64, 0)):
        assert lib.dd_loss_msssim_scratch_bytes(B, H, W, n) == -1, (B, H, W, n)
        assert len(lib.dd_last_error()) > 0


def test_msssim_invalid_arguments_return_status(lib):
    scratch, loss = ctypes.c_void_p(256), ctypes.c_void_p(512)      # never dereferenced: validation fails first
    assert lib.dd_loss_msssim_fwd(None, 1, 64, 64, scratch, loss, None) == -1
    assert b"null" in lib.dd_last_error()
    assert lib.dd_loss_msssim_bwd(None, 1, 64, 64, scratch, 1.0, None) == -1
    d = _lib.MsSsimDesc()
    d.n_features = 1
    d.pred[0], d.target[0], d.dpred[0] = 1024, 2048, 4096
    d.pred_ld[0] = d.target_ld[0] = d.nch[0] = 3
    d.ssim_weight[0] = 1.0
    assert lib.dd_loss_msssim_fwd(ctypes.byref(d), 1, 64, 64, None, loss, None) == -1
    assert lib.dd_loss_msssim_fwd(ctypes.byref(d), 1, 64, 64, scratch, None, None) == -1
    for B, H, W, word in ((0, 64, 64, b"positive"), (1, 64, 66, b"multiples of 4"), (1, 40, 64, b"filter")):
        assert lib.dd_loss_msssim_fwd(ctypes.byref(d), B, H, W, scratch, loss, None) == -1
        assert word in lib.dd_last_error(), lib.dd_last_error()
        assert lib.dd_loss_msssim_bwd(ctypes.byref(d), B, H, W, scratch, 1.0, None) == -1
    d.nch[0] = 1      # a 1-channel pass (Alpha, Depth): Training.py:187-190 would make it an image 1 pixel high
    assert lib.dd_loss_msssim_fwd(ctypes.byref(d), 1, 64, 64, scratch, loss, None) == -1
    assert b"channels" in lib.dd_last_error()
    d.nch[0], d.ssim_weight[0] = 3, 0.0      # nothing to evaluate
    assert lib.dd_loss_msssim_fwd(ctypes.byref(d), 1, 64, 64, scratch, loss, None) == -1
    assert b"weight" in lib.dd_last_error()


def test_msssim_struct_size_matches_header(lib):
    import os, subprocess, tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = '#include <stdio.h>\n#include "dd_hip.h"\nint main(void){ printf("%zu\\n", sizeof(dd_loss_msssim_desc)); return 0; }\n'
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "t.c"), os.path.join(tmp, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe])) == ctypes.sizeof(_lib.MsSsimDesc)
