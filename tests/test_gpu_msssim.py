"""-m gpu: the MS-SSIM loss term (csrc/dd_loss_msssim.hip) against the float64 restatement of tf.image.ssim_multiscale in tests/msssim_ref.py:
the op through the C-ABI, and whole models against the oracle wrapped with the term (msssim_ref.wrap_oracle).

Gates: the loss contribution at the project's fp32 gate for a loss (1e-4 relative) and dpred at 1e-4 rel-L2.  For scale: the reference
algorithm itself evaluated in float32 on the CPU differs from float64 by 4e-6 ... 3.6e-5 rel-L2 in the gradient (worst at 48 x 48) and by less
than 1e-6 absolute in the loss on these inputs; every device figure is recorded through gpu_util.check / gate (parity_errors.txt).
Every op-level and model-level case first asserts, ON THE REFERENCE'S OWN VALUES, that every factor cs_0, cs_1, ssim_2 of every image and
channel is >= 0.05: no case sits near the relu clamp, where the gradient of x^0.0448 is steep or undefined."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import msssim_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs
from deepdenoiser_amd.naming import Naming
from gpu_util import check, gate, rel_l2
from oracle import training as OT
from oracle.model import OracleArchitecture

pytestmark = pytest.mark.gpu
MIN_FACTOR = 0.05


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- op level
IMAGE_COMBINED = 4
LAYOUTS = {
    # name: (number of features, combined triples, image members (combined, features), weights (feature list, combined list, image))
    "features_only": (2, [], ([], []), ([0.7, 1.3], [], 0.0)),
    "one_combined": (3, [(0, 1, 2)], ([], []), ([0.0, 0.0, 0.0], [0.9], 0.0)),
    "full_image": (16, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(IMAGE_COMBINED)], (list(range(IMAGE_COMBINED)), [12, 13, 14, 15]),
                   ([0.0] * 16, [0.0] * 4, 1.1)),
    "all_levels": (16, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(IMAGE_COMBINED)], (list(range(IMAGE_COMBINED)), [12, 13, 14, 15]),
                   ([0.3] * 16, [0.5] * 4, 1.1)),
}


def _op_inputs(n_features, B, H, W, sigma, seed):
    """targets uniform in [0, 1] per pixel and channel, predictions = target + sigma * normal noise"""
    g = torch.Generator().manual_seed(seed)
    tgt = [torch.rand(B, H, W, 3, generator=g, dtype=torch.float64) for _ in range(n_features)]
    pred = [t + sigma * torch.randn(B, H, W, 3, generator=g, dtype=torch.float64) for t in tgt]
    return pred, tgt


def _sources(layout, pred, tgt):
    """[(name, weight, x, y)] of every source with a positive weight, formed as the oracle forms them (oracle/training.py)."""
    n, combs, (img_c, img_f), (wf, wc, wi) = LAYOUTS[layout]
    cx = [pred[c] * (pred[d] + pred[i]) for (c, d, i) in combs]
    cy = [tgt[c] * (tgt[d] + tgt[i]) for (c, d, i) in combs]
    out = [("feature %d" % f, wf[f], pred[f], tgt[f]) for f in range(n) if wf[f] > 0]
    out += [("combined %d" % k, wc[k], cx[k], cy[k]) for k in range(len(combs)) if wc[k] > 0]
    if wi > 0:
        out.append(("image", wi, sum([cx[k] for k in img_c] + [pred[f] for f in img_f]), sum([cy[k] for k in img_c] + [tgt[f] for f in img_f])))
    return out


def _reference(layout, pred, tgt):
    pred = [p.clone().requires_grad_() for p in pred]
    loss = 0.0
    for name, w, x, y in _sources(layout, pred, tgt):
        f = R.ms_ssim_factors(x, y)
        assert float(f.min()) >= MIN_FACTOR, "%s: factor %.3f is too close to the clamp for a gradient comparison" % (name, float(f.min()))
        loss = loss + R.ms_ssim_term(x, y, w)
    grads = torch.autograd.grad(loss, pred, allow_unused=True)
    return float(loss), [torch.zeros_like(p) if g is None else g for p, g in zip(pred, grads)]


class _Op:
    """Device buffers + descriptor of one layout; feature 1 is stored with a pixel stride of 4 (a source echoed next to the prediction)."""

    def __init__(self, layout, pred, tgt, B, H, W):
        n, combs, (img_c, img_f), (wf, wc, wi) = LAYOUTS[layout]
        self.B, self.H, self.W, self.n = B, H, W, n
        self.pred, self.tgt, self.dpred = [], [], []
        d = self.desc = L.MsSsimDesc()
        d.n_features = n
        for f in range(n):
            ld = 4 if f == 1 else 3
            p = torch.zeros(B, H, W, ld, dtype=torch.float32, device="cuda")
            p[..., :3] = pred[f].float().cuda()
            self.pred.append(p)
            self.tgt.append(tgt[f].float().cuda().contiguous())
            self.dpred.append(torch.zeros(B, H, W, 3, dtype=torch.float32, device="cuda"))
            d.pred[f], d.target[f], d.dpred[f] = p.data_ptr(), self.tgt[f].data_ptr(), self.dpred[f].data_ptr()
            d.pred_ld[f], d.target_ld[f], d.nch[f], d.ssim_weight[f] = ld, 3, 3, wf[f]
        d.n_combined = len(combs)
        for k, triple in enumerate(combs):
            for c in range(3):
                d.comb[k][c] = triple[c]
            d.comb_ssim_weight[k] = wc[k]
        d.n_image_combined, d.n_image_features = len(img_c), len(img_f)
        for i, k in enumerate(img_c):
            d.image_combined[i] = k
        for i, f in enumerate(img_f):
            d.image_features[i] = f
        d.image_ssim_weight = wi
        n_sources = sum(w > 0 for w in wf) + sum(w > 0 for w in wc) + (wi > 0)
        nbytes = L.load().dd_loss_msssim_scratch_bytes(B, H, W, n_sources)
        assert nbytes > 0
        self.scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        self.loss = torch.zeros(1, dtype=torch.float32, device="cuda")

    def forward(self):
        L.check(L.load().dd_loss_msssim_fwd(C.byref(self.desc), self.B, self.H, self.W, self.scratch.data_ptr(), self.loss.data_ptr(), _stream()))

    def backward(self, grad_scale=1.0):
        L.check(L.load().dd_loss_msssim_bwd(C.byref(self.desc), self.B, self.H, self.W, self.scratch.data_ptr(), grad_scale, _stream()))


SIZES = [(128, 128), (64, 64), (48, 48), (64, 96)]
# every size x sigma for the three layouts; the 21-source layout (whose float64 reference takes seconds per case on the CPU) at three of them
OP_CASES = ([(layout, size, sigma) for layout in ("features_only", "one_combined", "full_image") for size in SIZES for sigma in (0.1, 0.3)]
            + [("all_levels", (48, 48), 0.1), ("all_levels", (48, 48), 0.3), ("all_levels", (64, 64), 0.1)])


@pytest.mark.parametrize("layout,size,sigma", OP_CASES)
def test_op_parity(layout, size, sigma):
    _need_gpu()
    (H, W), B = size, 4
    pred, tgt = _op_inputs(LAYOUTS[layout][0], B, H, W, sigma, seed=H + W + int(10 * sigma))
    loss_ref, grads_ref = _reference(layout, pred, tgt)
    op = _Op(layout, pred, tgt, B, H, W)
    op.forward()
    op.backward()
    torch.cuda.synchronize()
    loss = float(op.loss)
    print("%s %dx%d sigma %.1f: loss %.8f (reference %.8f)" % (layout, H, W, sigma, loss, loss_ref))
    gate("loss contribution %s %dx%d s%.1f" % (layout, H, W, sigma), abs(loss - loss_ref) / abs(loss_ref), 1e-4)
    for f in range(op.n):
        if float(grads_ref[f].abs().max()) == 0.0:
            assert float(op.dpred[f].abs().max()) == 0.0, f
        else:
            e = check("dpred[%d] %s %dx%d s%.1f" % (f, layout, H, W, sigma), op.dpred[f].cpu(), grads_ref[f], 1e-4)
            print("  dpred[%d] rel-L2 %.3e" % (f, e))


def test_grad_scale_multiplies_the_gradient():
    _need_gpu()
    B, H, W = 2, 48, 48
    pred, tgt = _op_inputs(2, B, H, W, 0.1, seed=5)
    a, b = _Op("features_only", pred, tgt, B, H, W), _Op("features_only", pred, tgt, B, H, W)
    a.forward(), a.backward(1.0), b.forward(), b.backward(4096.0)
    torch.cuda.synchronize()
    for f in range(2):
        check("dpred[%d] at grad_scale 4096" % f, b.dpred[f].cpu() / 4096.0, a.dpred[f].cpu(), 1e-6)


def test_backward_adds_to_what_the_loss_head_wrote():
    """dd_loss_head OVERWRITES dpred, dd_loss_msssim_bwd ADDS to it: head, then the term == the sum of the two gradients, to the bit (one fp32
    addition per value on either side)."""
    _need_gpu()
    B, H, W = 2, 48, 64
    pred, tgt = _op_inputs(2, B, H, W, 0.1, seed=7)
    lib = L.load()

    def head(op):
        d = L.LossDesc()
        d.n_features, d.kind, d.epsilon = op.n, 5, 1e-2      # SMAPE
        for f in range(op.n):
            d.pred[f], d.target[f], d.dpred[f] = op.pred[f].data_ptr(), op.tgt[f].data_ptr(), op.dpred[f].data_ptr()
            d.pred_ld[f], d.target_ld[f], d.nch[f], d.weight[f], d.mask_feature[f] = op.desc.pred_ld[f], 3, 3, 1.0 + f, -1
        loss = torch.zeros(1, dtype=torch.float32, device="cuda")
        L.check(lib.dd_loss_head(C.byref(d), B, H, W, loss.data_ptr(), 1.0, _stream()))

    only_head, only_term, both = (_Op("features_only", pred, tgt, B, H, W) for _ in range(3))
    head(only_head)
    only_term.forward(), only_term.backward()
    for t in both.dpred:
        t.fill_(123.0)      # the head must overwrite this
    head(both)
    both.forward(), both.backward()
    torch.cuda.synchronize()
    for f in range(2):
        assert float(only_head.dpred[f].abs().max()) > 0 and float(only_term.dpred[f].abs().max()) > 0
        assert torch.equal(both.dpred[f], only_head.dpred[f] + only_term.dpred[f]), f


def test_two_runs_are_bit_identical():
    _need_gpu()
    B, H, W = 4, 64, 96
    pred, tgt = _op_inputs(16, B, H, W, 0.3, seed=11)
    runs = []
    for _ in range(2):
        op = _Op("all_levels", pred, tgt, B, H, W)
        op.forward(), op.backward()
        torch.cuda.synchronize()
        runs.append(op)
    assert torch.equal(runs[0].loss, runs[1].loss)
    for a, b in zip(runs[0].dpred, runs[1].dpred):
        assert torch.equal(a, b)


def test_checkerboard_pair_is_clamped_with_a_zero_gradient():
    """x = 0.5 + 0.3 s, y = 0.5 - 0.3 s (s a +-1 checkerboard): cs_0 < 0, relu clamps, MS = 0 as in TF; the term of that image is the weight
    itself and its gradient is DEFINED as 0 (TF's is 0 * inf)."""
    _need_gpu()
    H, W, w = 48, 48, LAYOUTS["features_only"][3][0][0]
    s = ((torch.arange(H).reshape(-1, 1) + torch.arange(W).reshape(1, -1)) % 2).double() * 2 - 1
    s = s.reshape(1, H, W, 1).expand(1, H, W, 3)
    assert float(R.ms_ssim(0.5 + 0.3 * s, 0.5 - 0.3 * s)[0]) == 0.0
    # one image, feature 0 alone (the weight of feature 1 is set to 0 below): loss contribution == the weight exactly
    pred, tgt = [0.5 + 0.3 * s, 0.25 + 0 * s], [0.5 - 0.3 * s, 0.25 + 0 * s]
    op = _Op("features_only", pred, tgt, 1, H, W)
    op.desc.ssim_weight[1] = 0.0
    op.scratch = torch.zeros(L.load().dd_loss_msssim_scratch_bytes(1, H, W, 1) // 4, dtype=torch.float32, device="cuda")
    op.forward(), op.backward()
    torch.cuda.synchronize()
    assert float(op.loss) == float(torch.tensor(w, dtype=torch.float32))
    assert float(op.dpred[0].abs().max()) == 0.0
    # two images, the second an ordinary noisy pair: image 0 clamped (gradient 0), image 1 with the gradient of the reference
    g = torch.Generator().manual_seed(3)
    t1 = torch.rand(1, H, W, 3, generator=g, dtype=torch.float64)
    p1 = t1 + 0.1 * torch.randn(1, H, W, 3, generator=g, dtype=torch.float64)
    pred, tgt = [torch.cat([0.5 + 0.3 * s, p1]), torch.cat([p1, p1])], [torch.cat([0.5 - 0.3 * s, t1]), torch.cat([t1, t1])]
    op = _Op("features_only", pred, tgt, 2, H, W)
    op.forward(), op.backward()
    torch.cuda.synchronize()
    for t in op.dpred:
        assert torch.isfinite(t).all()
    assert float(op.dpred[0][0].abs().max()) == 0.0
    x = p1.clone().requires_grad_()
    want = torch.autograd.grad(w * (1.0 - (0.0 + R.ms_ssim(x, t1)[0]) / 2.0), x)[0]
    check("dpred of the unclamped image", op.dpred[0][1:].cpu(), want, 1e-4)


# ---------------------------------------------------------------------------------------------------------------- whole model
NO_ALPHA = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
MODELS = {
    # cfg-2 (one SINGLE tuple: Emission): the features level is the only one that exists
    "cfg2_features_next_to_mean": (lambda: configs.cfg2_unet_kpcn(), dict(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0)), "f32"),
    "cfg2_ms_ssim_only": (lambda: configs.cfg2_unet_kpcn(), dict(feature_mean=0.0, combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0)), "f32"),
    "cfg2_bf16": (lambda: configs.cfg2_unet_kpcn(), dict(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0)), "bf16"),
    # the 17-tuple example network: its loaded 1-channel Alpha pass rules a features-level weight out (Training.py:187-190), as in the reference
    "example_combined_and_image": (lambda: configs.architecture(filters=(16, 16), convs=1, flag_mode="NONE"), dict(ms_ssim=(0.0, 2.0, 4.0)), "f32"),
    # the same network without the Alpha pass: all three levels next to the mean weights
    "all_three_levels": (lambda: configs.architecture(filters=(16, 16), convs=1, flag_mode="NONE", combined=NO_ALPHA), dict(ms_ssim=(0.6, 2.0, 4.0)), "f32"),
    # invert_standardization_after_multiscale_predictions: the inversion must NOT be fused into dd_loss_head when the term is on
    "invert_after_multiscale": (lambda: configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), dict(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0)), "f32"),
    "invert_before_multiscale": (lambda: configs.architecture(filters=(16, 16), convs=1, flag_mode="NONE", invert_after_multiscale=False,
                                                              combined={"Emission": {"Color": "Emission", "Direct": "", "Indirect": ""}}),
                                 dict(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0)), "f32"),
}


def _smooth(g, B, H, W, channels):
    """an 8x8 uniform random grid bilinearly enlarged to the tile, mapped to [0.1, 1]"""
    grid = torch.rand(B, channels, 8, 8, generator=g)
    return (0.1 + 0.9 * F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)).permute(0, 2, 3, 1).contiguous()


def _model_inputs(oracle, B, H, W, seed=0):
    """labels = smooth random fields, sources = label + 0.05 * normal noise; generated passes constant (Training.py:531-538).  An untrained
    kernel-predicting network returns a blurred source, which correlates with such a label."""
    g = torch.Generator().manual_seed(seed)
    feats, labels = {}, {}
    for f in oracle.features:
        t = _smooth(g, B, H, W, f.channels)
        v = t + 0.05 * torch.randn(B, H, W, f.channels, generator=g)
        if not f.load_data:
            t = torch.full((B, H, W, f.channels), 1.0 if f.ftype == "COLOR" else 0.5)
            v = t.clone()
        labels[Naming.target_feature_name(f.name)] = t
        feats[Naming.source_feature_name(f.name, index=0)] = v
    for f in oracle.auxiliary:
        feats[Naming.source_feature_name(f.name, index=0)] = _smooth(g, B, H, W, f.channels) + 0.05 * torch.randn(B, H, W, f.channels, generator=g)
    return feats, labels


def _model(case, monkeypatch, record=None):
    from deepdenoiser_amd.architecture import Architecture
    make, knobs, dtype = MODELS[case]
    aj, tj = make(), configs.training(**knobs)
    R.wrap_oracle(monkeypatch, record)
    B, H, W = 2, 64, 64
    oracle = OracleArchitecture(aj, dtype=torch.float64, seed=2)
    feats, labels = _model_inputs(oracle, B, H, W)
    preds_o = oracle.predict(feats)
    arch = Architecture(aj, device="cuda", dtype=dtype)
    prog = arch.program(B, H, W, training_json=tj)
    assert [p.name for p in arch.params.params] == list(oracle.vs.vars.keys())
    arch.params.load_list(list(oracle.vs.vars.values()))
    dev = {k: v.cuda() for k, v in feats.items()}
    devl = {k: v.cuda() for k, v in labels.items()}
    return aj, tj, oracle, arch, prog, feats, labels, dev, devl, preds_o


def _assert_factors(record, expected_terms):
    assert len(record) == expected_terms, [n for n, _ in record]
    for name, f in record:
        assert float(f.min()) >= MIN_FACTOR, "%s: factor %.3f is too close to the clamp" % (name, float(f.min()))
    print("ms_ssim factors of the oracle: %.3f ... %.3f over %d terms" % (min(float(f.min()) for _, f in record), max(float(f.max()) for _, f in record), len(record)))


EXPECTED_TERMS = {"cfg2_features_next_to_mean": 1, "cfg2_ms_ssim_only": 1, "cfg2_bf16": 1, "invert_after_multiscale": 1,
                  "example_combined_and_image": 4 + 1, "all_three_levels": 16 + 4 + 1, "invert_before_multiscale": 1}


@pytest.mark.parametrize("case", ["cfg2_features_next_to_mean", "cfg2_ms_ssim_only", "example_combined_and_image", "all_three_levels",
                                  "invert_after_multiscale", "invert_before_multiscale"])
def test_model_step_parity_f32(case, monkeypatch):
    """predictions, loss and every weight gradient against the wrapped oracle, at the step-1 gates of test_gpu_model.test_training_step_parity_f32"""
    _need_gpu()
    record = []
    aj, tj, oracle, arch, prog, feats, labels, dev, devl, preds_o = _model(case, monkeypatch, record)
    if case == "invert_after_multiscale":
        assert aj["architecture"]["multiscale_prediction"]["invert_standardization_after_multiscale_predictions"]
    start = [v.detach().clone() for v in oracle.vs.vars.values()]
    loss_o, grads_o = OT.train_step(oracle, aj, tj, feats, labels, ([], []), 1)
    _assert_factors(record, EXPECTED_TERMS[case])
    # the term must actually contribute
    tj0 = configs.training(**dict(MODELS[case][1], ms_ssim=(0.0, 0.0, 0.0)))
    assert abs(float(OT.model_loss(oracle, aj, tj0, preds_o, labels)) - float(loss_o)) > 1e-2 * abs(float(loss_o))
    preds = arch.predict(dev)
    for s, (dp, do) in enumerate(zip(preds, preds_o)):
        for k in do:
            check("scale %d %s" % (s, k), dp[k].cpu(), do[k], 1e-4)
    loss = prog.train_step(dev, devl)
    torch.cuda.synchronize()
    gate("loss %s" % case, abs(float(loss) - float(loss_o)) / abs(float(loss_o)), 2e-5)
    errs = []
    for p, n, go in zip(arch.params.params, list(oracle.vs.vars.keys()), grads_o):
        if float(go.abs().max()) == 0.0:
            assert float(arch.params.grad(p).abs().max()) < 1e-6, n
        else:
            errs.append(check("grad " + n, arch.params.grad(p).cpu(), go, 5e-4))
    print("%s: gradient rel-L2 median %.2e max %.2e" % (case, sorted(errs)[len(errs) // 2], max(errs)))
    if case == "cfg2_ms_ssim_only":
        # dd_loss_head writes no dpred for a source without a mean weight and the term's backward ADDS: a second step from the same weights
        # must give the same gradients again, not twice the gradients
        arch.params.load_list(start)
        loss2 = prog.train_step(dev, devl)
        torch.cuda.synchronize()
        assert float(loss2) == float(loss)
        for p, go in zip(arch.params.params, grads_o):
            if float(go.abs().max()) > 0:
                check("grad (second step) " + p.name, arch.params.grad(p).cpu(), go, 5e-4)


def test_model_step_bf16(monkeypatch):
    """bf16 storage at the half-precision gates of test_gpu_model.test_bf16_path_reports_its_tolerance (loss 3e-2, median gradient 0.14)"""
    _need_gpu()
    record = []
    aj, tj, oracle, arch, prog, feats, labels, dev, devl, preds_o = _model("cfg2_bf16", monkeypatch, record)
    loss_o, grads_o = OT.train_step(oracle, aj, tj, feats, labels, ([], []), 1)
    _assert_factors(record, 1)
    loss = prog.train_step(dev, devl)
    torch.cuda.synchronize()
    gate("bf16 loss", abs(float(loss) - float(loss_o)) / abs(float(loss_o)), 3e-2)
    errs = sorted(rel_l2(arch.params.grad(p).cpu(), go) for p, go in zip(arch.params.params, grads_o) if float(go.norm()) > 0)
    gate("bf16 median gradient rel-L2", errs[len(errs) // 2], 0.14)


def test_program_build_rules():
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    tj = configs.training(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0))
    with pytest.raises(ValueError, match="multiples of 4 and at least 44"):
        Architecture(configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), device="cuda", dtype="f32").program(1, 40, 40, training_json=tj)
    with pytest.raises(ValueError, match="multiples of 4 and at least 44"):
        Architecture(configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), device="cuda", dtype="f32").program(1, 64, 50, training_json=tj)
    with pytest.raises(ValueError, match="1-channel target pass 'Alpha'"):
        Architecture(configs.architecture(filters=(16, 16), convs=1, flag_mode="NONE"), device="cuda", dtype="f32").program(
            1, 64, 64, training_json=configs.training(ms_ssim=(0.6, 0.0, 0.0)))
    masked = configs.training(ms_ssim=(0.0, 0.0, 0.0))
    masked["features_training_settings"]["loss_weights_masked"]["ms_ssim"] = 0.5
    with pytest.raises(NotImplementedError, match="Training.py:206-207"):
        Architecture(configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), device="cuda", dtype="f32").program(1, 64, 64, training_json=masked)
    # track_ms_ssim selects nothing (summaries are out of scope): with every weight 0 no launch is added
    tracked = configs.training(combined_mean=0.0, image_mean=0.0)
    tracked["features_training_settings"]["statistics"]["track_ms_ssim"] = True
    prog = Architecture(configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), device="cuda", dtype="f32").program(1, 64, 64, training_json=tracked)
    assert not hasattr(prog, "ms_ssim_desc")


def test_three_adam_steps_follow_the_oracle(monkeypatch):
    """three Adam steps against oracle.training.train_step under the same wrapper: the loss and displacement gates of
    test_gpu_model.test_training_step_parity_f32 (2e-5 on the loss of step 1, 1e-3 on steps 2 and 3)"""
    _need_gpu()
    aj, tj, oracle, arch, prog, feats, labels, dev, devl, _ = _model("cfg2_features_next_to_mean", monkeypatch)
    state = ([], [])
    start = [p.detach().clone() for p in oracle.parameters()]
    for step in range(1, 4):
        loss_o, _ = OT.train_step(oracle, aj, tj, feats, labels, state, step)
        loss = prog.train_step(dev, devl)
        torch.cuda.synchronize()
        gate("loss of step %d" % step, abs(float(loss) - float(loss_o)) / abs(float(loss_o)), 2e-5 if step == 1 else 1e-3)
    lr = tj["learning_rate"]
    for p, po, p0 in zip(arch.params.params, oracle.parameters(), start):
        d, do = arch.params.value(p).double().cpu() - p0, po.detach() - p0
        assert float((d - do).abs().max()) <= 2.0 * 3 * lr + 1e-9, p.name
        if float(do.norm()) > 0:
            assert rel_l2(d, do) < 0.2, (p.name, rel_l2(d, do))
            assert int(((d - do).abs() > 0.5 * lr).sum()) <= max(0.15 * d.numel(), 4), p.name


@pytest.mark.parametrize("use_graph", [False, True])
def test_captured_graph_step_equals_plain_step(use_graph):
    """as test_gpu_model.test_segmented_trainer_matches_plain_step, with the term on: every new launch is captured in the step's hipGraph"""
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.training import Trainer
    aj, B, H, W = configs.cfg2_unet_kpcn(filters=(16, 16), convs=1), 2, 64, 64
    tj = configs.training(combined_mean=0.0, image_mean=0.0, ms_ssim=(0.6, 0.0, 0.0))
    ref = Architecture(aj, device="cuda", dtype="f32", seed=2)
    prog = ref.program(B, H, W, training_json=tj)
    seg = Architecture(aj, device="cuda", dtype="f32", seed=2)
    trainer = Trainer(seg, tj, B, H, W, world_size=1, use_graph=use_graph, n_buckets=3, force_segments=True)
    assert hasattr(prog, "ms_ssim_desc") and hasattr(trainer.program, "ms_ssim_desc")
    oracle = OracleArchitecture(aj, dtype=torch.float64, seed=2)
    feats, labels = _model_inputs(oracle, B, H, W)
    dev = {k: v.cuda() for k, v in feats.items()}
    devl = {k: v.cuda() for k, v in labels.items()}
    trainer.program.set_inputs(dev, devl)
    for step in range(4):                      # graphs are captured after two eager steps
        loss_ref = float(prog.train_step(dev, devl))
        loss_seg = float(trainer.step())
        assert abs(loss_ref - loss_seg) <= 1e-5 * abs(loss_ref), (step, loss_ref, loss_seg)
    assert (trainer._graphs is not None) == use_graph
    lr = tj["learning_rate"]
    d = (ref.params.values - seg.params.values).abs()
    assert float(d.max()) <= 2 * 4 * lr
    assert float((d > 0.5 * lr).float().mean()) < 0.02
