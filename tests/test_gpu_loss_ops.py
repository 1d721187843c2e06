"""-m gpu: the kernels that produce the training signal, op by op through the C-ABI, against the float64 reference of tests/loss_ref.py:
dd_loss_head (its three kernels: flat-stream, per-pixel, older), dd_loss_mask_sums, dd_invert_std_fwd / _bwd and dd_avgpool.

Every case of loss_ref.CASES x LossDifference kind pre-fills dpred and pred_inv with a sentinel, runs dd_loss_mask_sums where a masked weight is
set, then dd_loss_head, asserts WHICH kernel ran (dd_loss_head_path_count, expectation from the case and DD_LOSS_SIMPLE / DD_LOSS_GENERAL of this
process) and compares with the reference.  Gates (DESIGN.md "How the loss kernels are gated"):
    mask sums                    torch.equal with the integer counts (below 2^24: fp32 sums of 0 / 1 are exact)
    dpred, pred_inv, inversion,  gpu_util.ROUND["f32"] = 5e-6 rel-L2 per tensor.  The reference's own float32 evaluation differs from float64 by
    average pool                 <= 7.9e-7 (tests/test_loss_ref.py prints it per case and asserts <= 1.25e-6, so no case needs more)
    loss                         |loss - ref| / sum |w * term| <= 2e-5 (the loss gate of test_gpu_model.py; the normaliser is the sum of the
                                 ABSOLUTE per-element terms, because DIFFERENCE sums signed terms that cancel)
A feature nothing depends on must show the contract of include/dd_hip.h: dpred untouched by the flat-stream kernel, zeroed by the other two."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (the child process of the bit-identity test runs this file as a script)
    sys.path.insert(0, ROOT)

import loss_ref as R                              # noqa: E402
from deepdenoiser_amd import _lib as L            # noqa: E402
from gpu_util import ROUND, check, gate           # noqa: E402
from oracle import tf_ops as T                    # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
LOSS_GATE = 2e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _counts(lib):
    return [lib.dd_loss_head_path_count(p) for p in range(3)]


def _strided(values, ld, offset=0, junk=99.0):
    """[B,H,W,3] values -> (owner, data pointer) of a device block with pixel stride ld whose first element sits `offset` floats into the
    allocation; the unused channel holds junk."""
    n = values.shape[0] * values.shape[1] * values.shape[2]
    flat = torch.full((n * ld + 4,), junk, dtype=torch.float32, device="cuda")
    flat[offset:offset + n * ld].view(n, ld)[:, :3] = values.reshape(n, 3).float().cuda()
    return flat, flat.data_ptr() + 4 * offset


class Dev:
    """Device buffers and descriptor of one case."""

    def __init__(self, case, kind, x, t, grad_scale=None, fused=True, pred_override=None):
        self.case, self.lib = case, L.load()
        self.B, self.H, self.W = case["B"], case["H"], case["W"]
        self.grad_scale = case["grad_scale"] if grad_scale is None else grad_scale
        shape = (self.B, self.H, self.W, 3)
        self.keep, self.dpred, self.pred_inv = [], [], {}
        d = self.desc = L.LossDesc()
        d.n_features, d.kind, d.epsilon = len(case["features"]), R.KINDS[kind], R.EPSILON
        for f, ft in enumerate(case["features"]):
            xs = x[f] if pred_override is None else pred_override[f]
            if ft["fused"] is not None and fused:
                xb = xs.float().cuda().contiguous()
                nan = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")      # pred[f] must not be read
                inv = torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
                self.keep += [xb, nan]
                self.pred_inv[f] = inv
                d.pred_std[f], d.pred[f], d.pred_inv[f] = xb.data_ptr(), nan.data_ptr(), inv.data_ptr()
                d.inv_log1p[f], d.inv_mean[f], d.inv_std[f] = ft["fused"]
            else:
                owner, ptr = _strided(xs, ft["pred_ld"], case["pred_offset"])
                self.keep.append(owner)
                d.pred[f] = ptr
            d.pred_ld[f] = ft["pred_ld"]
            owner, ptr = _strided(t[f], ft["target_ld"])
            self.keep.append(owner)
            d.target[f], d.target_ld[f], d.nch[f] = ptr, ft["target_ld"], ft["nch"]
            g = torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
            self.dpred.append(g)
            d.dpred[f] = g.data_ptr()
            d.weight[f], d.var_weight[f], d.masked_weight[f], d.mask_feature[f] = ft["w"], ft["vw"], ft["mw"], ft["mask"]
        d.n_combined = len(case["combined"])
        for k, c in enumerate(case["combined"]):
            for j in range(3):
                d.comb[k][j] = c["triple"][j]
            d.comb_weight[k], d.comb_var_weight[k], d.comb_masked_weight[k], d.comb_mask_feature[k] = c["w"], c["vw"], c["mw"], c["mask"]
        img = case["image"]
        if img:
            d.n_image_combined, d.n_image_features = len(img["combined"]), len(img["features"])
            for j, k in enumerate(img["combined"]):
                d.image_combined[j] = k
            for j, f in enumerate(img["features"]):
                d.image_features[j] = f
            d.image_weight, d.image_var_weight = img["w"], img["vw"]
        self.masked = any(ft["mw"] != 0 and ft["mask"] >= 0 for ft in case["features"]) or any(c["mw"] != 0 and c["mask"] >= 0 for c in case["combined"])
        self.mask_sums = torch.full((R.MAX_FEATURES + R.MAX_COMBINED,), SENTINEL, dtype=torch.float32, device="cuda")
        d.mask_sums = self.mask_sums.data_ptr() if self.masked else None
        self.loss = torch.zeros(1, dtype=torch.float32, device="cuda")

    def run(self):
        """dd_loss_mask_sums where needed, then dd_loss_head; returns the index of the kernel that ran (exactly one launch)."""
        if self.masked:
            L.check(self.lib.dd_loss_mask_sums(C.byref(self.desc), self.B, self.H, self.W, self.mask_sums.data_ptr(), _stream()))
        before = _counts(self.lib)
        L.check(self.lib.dd_loss_head(C.byref(self.desc), self.B, self.H, self.W, self.loss.data_ptr(), self.grad_scale, _stream()))
        torch.cuda.synchronize()
        moved = [a - b for a, b in zip(_counts(self.lib), before)]
        assert sorted(moved) == [0, 0, 1], "dd_loss_head did not launch exactly one kernel: %s" % moved
        return moved.index(1)


def _compare(case, kind, dev, ref, path, tag):
    if dev.masked:
        assert torch.equal(dev.mask_sums.cpu().double(), ref["mask_sums"]), (dev.mask_sums.cpu(), ref["mask_sums"])
    loss = float(dev.loss)
    err = abs(loss - ref["loss"]) / ref["abs_sum"] if ref["abs_sum"] > 0 else abs(loss - ref["loss"])
    print("%s: kernel %d, loss %.8f (reference %.8f), error %.2e of sum|w term|" % (tag, path, loss, ref["loss"], err))
    gate("loss " + tag, err, LOSS_GATE)
    for f, want in enumerate(ref["dpred"]):
        got = dev.dpred[f].cpu()
        if want is None:      # nothing depends on this feature: include/dd_hip.h, dd_loss_desc.dpred
            if path == 0:
                assert bool((got == SENTINEL).all()), "feature %d: the flat-stream kernel touched the dpred of a feature without a weight" % f
            else:
                assert not got.any(), "feature %d: dpred of a feature without a weight is not zero after kernel %d" % (f, path)
            continue
        assert not bool((got == SENTINEL).any()), "feature %d: dpred was not overwritten completely" % f
        if float(want.norm()) == 0.0:
            assert not got.any(), f
        else:
            e = check("dpred[%d] %s" % (f, tag), got, want, ROUND["f32"])
            print("  dpred[%d] rel-L2 %.3e" % (f, e))
    for f, want in ref["pred_inv"].items():
        if f in dev.pred_inv:
            got = dev.pred_inv[f].cpu()
            assert not bool((got == SENTINEL).any()), "feature %d: pred_inv was not written completely" % f
            e = check("pred_inv[%d] %s" % (f, tag), got, want, ROUND["f32"])
            print("  pred_inv[%d] rel-L2 %.3e" % (f, e))


@pytest.mark.parametrize("name,kind", R.CASE_KINDS, ids=["%s-%s" % ck for ck in R.CASE_KINDS])
def test_loss_head_parity(name, kind):
    _need_gpu()
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    R.check_family(case, kind, x, t)
    ref = R.evaluate(case, kind, x, t)
    dev = Dev(case, kind, x, t)
    path = dev.run()
    assert path == R.expected_path(case, os.environ), "kernel %d ran, the case and the switches call for %d" % (path, R.expected_path(case, os.environ))
    _compare(case, kind, dev, ref, path, "%s %s" % (name, kind))


# ---------------------------------------------------------------------------------------------------------------- contracts
ONE_WORKGROUP = ["flat_2_features", "ragged_pixel_64px", "older_variation_with_mean"]      # one workgroup each: a single atomic into loss_out
PER_KERNEL = ["flat_17_features", "pixel_combined_image_features", "older_variation_with_masked"]


@pytest.mark.parametrize("name", ONE_WORKGROUP)
def test_loss_out_is_added_to(name):
    _need_gpu()
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    a, b = Dev(case, "SMAPE", x, t), Dev(case, "SMAPE", x, t)
    b.loss.fill_(3.0)
    a.run(), b.run()
    assert float(a.loss) != 0.0 and torch.equal(b.loss, a.loss + 3.0), (float(a.loss), float(b.loss))


@pytest.mark.parametrize("name", PER_KERNEL)
def test_grad_scale_4096_scales_dpred_exactly(name):
    _need_gpu()
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    for kind in R.ALL_KINDS:
        a, b = Dev(case, kind, x, t, grad_scale=1.0), Dev(case, kind, x, t, grad_scale=4096.0)
        assert a.run() == b.run()
        for f in range(len(a.dpred)):
            assert torch.equal(b.dpred[f], a.dpred[f] * 4096.0), (kind, f)


@pytest.mark.parametrize("name", PER_KERNEL + ["flat_fused_on_some_features", "pixel_fused_next_to_combined"])
def test_two_runs_give_the_same_bits(name):
    _need_gpu()
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    a, b = Dev(case, "SMAPE" if "SMAPE" in case["kinds"] else "SQUARED", x, t), Dev(case, "SMAPE" if "SMAPE" in case["kinds"] else "SQUARED", x, t)
    assert a.run() == b.run()
    for f in range(len(a.dpred)):
        assert torch.equal(a.dpred[f], b.dpred[f]), f
    for f in a.pred_inv:
        assert torch.equal(a.pred_inv[f], b.pred_inv[f]), f


def test_feature_without_a_weight_per_kernel():
    """include/dd_hip.h (dd_loss_desc.dpred): left untouched by the flat-stream kernel, zeroed by the other two."""
    _need_gpu()
    for name, f in (("flat_zero_weight_in_the_middle", 1), ("pixel_masked_all_black", 1)):
        case = R.BY_NAME[name]
        x, t = R.make_inputs(case)
        dev = Dev(case, "SMAPE", x, t)
        path = dev.run()
        assert path == R.expected_path(case, os.environ)
        got = dev.dpred[f].cpu()
        assert bool((got == SENTINEL).all()) if path == 0 else not got.any(), (name, path)
    # the older kernel: a feature next to a variation term
    case = R.case("weightless_older", "older", "dyadic", (2, 8, 10), [R.feat(vw=1.0), R.feat()], seed=61)
    x, t = R.make_inputs(case)
    dev = Dev(case, "SMAPE", x, t)
    assert dev.run() == 2 and not dev.dpred[1].any() and not bool((dev.dpred[0] == SENTINEL).any())


def test_rejected_descriptors_launch_nothing():
    _need_gpu()
    lib = L.load()
    case = R.BY_NAME["flat_fused_log1p"]
    x, t = R.make_inputs(case)

    def refused(dev):
        before = _counts(lib)
        rc = lib.dd_loss_head(C.byref(dev.desc), dev.B, dev.H, dev.W, dev.loss.data_ptr(), 1.0, _stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error(), rc
        assert _counts(lib) == before and float(dev.loss) == 0.0
        for g in dev.dpred + list(dev.pred_inv.values()):
            assert bool((g == SENTINEL).all())

    for kind in (0, 6):
        dev = Dev(case, "SMAPE", x, t)
        dev.desc.kind = kind
        refused(dev)
    dev = Dev(case, "SMAPE", x, t)
    dev.desc.pred_inv[1] = None
    refused(dev)
    for std in (0.0, -1.5):
        dev = Dev(case, "SMAPE", x, t)
        dev.desc.inv_std[0] = std
        refused(dev)
    dev = Dev(case, "SMAPE", x, t)
    dev.desc.var_weight[1] = 0.5
    refused(dev)


# ---------------------------------------------------------------------------------------------------------------- the code's own claims
def _invert_fwd(lib, xb, fused):
    y = torch.full_like(xb, SENTINEL)
    L.check(lib.dd_invert_std_fwd(xb.data_ptr(), y.data_ptr(), xb.numel(), int(fused[0]), fused[1], fused[2], _stream()))
    return y


@pytest.mark.parametrize("name", ["flat_fused_log1p", "flat_fused_linear", "flat_fused_z_exactly_0", "flat_fused_on_some_features",
                                  "pixel_fused_next_to_combined"])
def test_fused_inversion_stores_what_the_inversion_kernels_store(name):
    """csrc/dd_pointwise.hip: the fused launch stores "the expressions of invert_std_fwd_kernel / invert_std_bwd_kernel, element for element".
    pred_inv: bit-equal to dd_invert_std_fwd.  dpred: bit-equal to the unfused dd_loss_head on that pred_inv followed by dd_invert_std_bwd."""
    _need_gpu()
    lib = L.load()
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    for kind in case["kinds"]:
        fused = Dev(case, kind, x, t)
        fused.run()
        inv = {}
        for f, ft in enumerate(case["features"]):
            if ft["fused"] is not None:
                inv[f] = _invert_fwd(lib, x[f].float().cuda().contiguous(), ft["fused"])
                assert torch.equal(fused.pred_inv[f], inv[f]), "%s %s: pred_inv[%d] differs from dd_invert_std_fwd" % (name, kind, f)
        plain = Dev(case, kind, x, t, fused=False, pred_override=[inv[f].cpu().double() if f in inv else x[f] for f in range(len(x))])
        plain.run()
        for f, ft in enumerate(case["features"]):
            want = plain.dpred[f]
            if ft["fused"] is not None:
                xb = x[f].float().cuda().contiguous()
                L.check(lib.dd_invert_std_bwd(xb.data_ptr(), want.data_ptr(), want.data_ptr(), xb.numel(), int(ft["fused"][0]), ft["fused"][1],
                                              ft["fused"][2], _stream()))      # in place: dx == dy
                torch.cuda.synchronize()
            # measured bit-equal in all 61 comparisons of these cases, so that is what is asserted (the recorded figure is 0)
            check("fused dpred[%d] vs unfused + dd_invert_std_bwd, %s %s" % (f, name, kind), fused.dpred[f].cpu(), want.cpu(), 1e-6)
            assert torch.equal(fused.dpred[f], want), "%s %s: fused dpred[%d] differs from dd_loss_head + dd_invert_std_bwd" % (name, kind, f)


BIT_CASES = ["pixel_combined_image_features", "pixel_masked_partially_black", "pixel_32_features_8_triples"]


def _bit_case_dpred(name):
    case = R.BY_NAME[name]
    x, t = R.make_inputs(dict(case, family="continuous", seed=700 + len(name)))      # seeded randn: every rounding of the two kernels is exercised
    dev = Dev(case, "SMAPE", x, t)
    path = dev.run()
    return path, [g.cpu() for g in dev.dpred]


def test_per_pixel_kernel_is_bit_identical_to_the_older_kernel(tmp_path):
    """csrc/dd_pointwise.hip: loss_general_kernel's "dpred is bit-identical to loss_head_kernel's".  The switches are read once per process, so
    the older kernel runs in a child (DD_LOSS_SIMPLE=0 DD_LOSS_GENERAL=0) that leaves its dpred tensors in tmp_path."""
    _need_gpu()
    out = str(tmp_path / "older.pt")
    env = dict(os.environ, DD_LOSS_SIMPLE="0", DD_LOSS_GENERAL="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child failed\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:])
    older = torch.load(out)
    for name in BIT_CASES:
        path, dpred = _bit_case_dpred(name)
        assert path == 1 and older[name][0] == 2, (name, path, older[name][0])
        for f, (a, b) in enumerate(zip(dpred, older[name][1])):
            assert float(a.abs().max()) > 0 and torch.equal(a, b), "%s: dpred[%d] of the two kernels differs (max %.3e)" % (name, f, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- inversion and pooling alone
@pytest.mark.parametrize("log1p", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 70001])
def test_invert_std_alone(n, log1p):
    _need_gpu()
    lib = L.load()
    g = torch.Generator().manual_seed(n + log1p)
    mean, std = 0.25, 1.5
    z = torch.randn(n, generator=g, dtype=torch.float64) * 2
    x = ((z - mean) / std).float().double()                      # fp32 inputs
    special = torch.tensor([0.0, 1e-30, -1e-30, 1e-6, -1e-6, 5.0, -5.0], dtype=torch.float64)[:n]
    z[:len(special)] = special                                   # mean 0: x == 0 gives z == 0 exactly, x = +-tiny gives z = +-tiny
    dy = torch.randn(n, generator=g, dtype=torch.float32).double()
    for m, xs in ((mean, x), (0.0, (z / std).float().double())):
        xr = xs.clone().requires_grad_()
        want = R.invert(xr, (log1p, m, std))
        (want_dx,) = torch.autograd.grad(want, xr, dy)
        xb, dyb = xs.float().cuda(), dy.float().cuda()
        y = torch.full_like(xb, SENTINEL)
        dx = torch.full_like(xb, SENTINEL)
        L.check(lib.dd_invert_std_fwd(xb.data_ptr(), y.data_ptr(), n, log1p, m, std, _stream()))
        L.check(lib.dd_invert_std_bwd(xb.data_ptr(), dyb.data_ptr(), dx.data_ptr(), n, log1p, m, std, _stream()))
        torch.cuda.synchronize()
        check("invert_std_fwd n %d log1p %d mean %g" % (n, log1p, m), y.cpu(), want.detach(), ROUND["f32"])
        check("invert_std_bwd n %d log1p %d mean %g" % (n, log1p, m), dx.cpu(), want_dx, ROUND["f32"])
        if m == 0.0:
            zero = xs == 0
            assert bool(zero.any()) and not y.cpu()[zero].any()
            assert (not dx.cpu()[zero].any()) if log1p else bool((dx.cpu()[zero] == (dy[zero] * std).float()).all())
        # in place (y == x, dx == dy): the header allows it; same bits as out of place
        xi, dyi = xb.clone(), dyb.clone()
        L.check(lib.dd_invert_std_bwd(xb.data_ptr(), dyi.data_ptr(), dyi.data_ptr(), n, log1p, m, std, _stream()))
        L.check(lib.dd_invert_std_fwd(xi.data_ptr(), xi.data_ptr(), n, log1p, m, std, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(xi, y) and torch.equal(dyi, dx)
    assert lib.dd_invert_std_fwd(None, None, n, log1p, mean, std, _stream()) != 0


@pytest.mark.parametrize("f", [1, 2, 4])
@pytest.mark.parametrize("nch", [1, 3])
def test_avgpool_alone(nch, f):
    _need_gpu()
    lib = L.load()
    B, H, W, ldx, ldy, cx, cy = 2, 8, 12, 5, 6, 1, 2      # the pooled channels sit at channel 1 of x and channel 2 of y
    g = torch.Generator().manual_seed(10 * nch + f)
    x = torch.randn(B, H, W, ldx, generator=g, dtype=torch.float32)
    want = T.avg_pool_same(x.double()[..., cx:cx + nch], f)
    xb = x.cuda()
    y = torch.full((B, H // f, W // f, ldy), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(lib.dd_avgpool(xb.data_ptr() + 4 * cx, ldx, y.data_ptr() + 4 * cy, ldy, nch, B, H, W, f, _stream()))
    torch.cuda.synchronize()
    check("avgpool C %d f %d" % (nch, f), y.cpu()[..., cy:cy + nch], want, ROUND["f32"])
    untouched = torch.ones(ldy, dtype=torch.bool)
    untouched[cy:cy + nch] = False
    assert bool((y.cpu()[..., untouched] == SENTINEL).all()), "dd_avgpool wrote a neighbouring channel"
    assert torch.equal(xb.cpu(), x)
    if f > 1:
        assert lib.dd_avgpool(xb.data_ptr(), ldx, y.data_ptr(), ldy, nch, B, H + 1, W, f, _stream()) != 0      # H % f != 0: refused
        assert b"divisible" in lib.dd_last_error()


if __name__ == "__main__":      # the child of test_per_pixel_kernel_is_bit_identical_to_the_older_kernel
    torch.save({name: _bit_case_dpred(name) for name in BIT_CASES}, sys.argv[1])
