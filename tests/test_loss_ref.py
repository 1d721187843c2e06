"""CPU: tests/loss_ref.py, the float64 reference of the op-level loss tests (tests/test_gpu_loss_ops.py), anchored and characterised.

* anchored: descriptors run through oracle.training._FT objects built the way model_loss builds them (what tests/test_wiring_golden.py pins
  against the reference's executed graph) must give loss_ref's loss and gradients, at that file's gates (1e-12 / 1e-9);
* every case of the table satisfies its input family's condition (dyadic: every source value bit-equal in fp32 and f64; continuous: the
  margin), names the kernel it is aimed at, and has its float32-vs-float64 floor printed: the numbers the device gates are read against."""
import pytest
import torch

import loss_ref as R
from oracle import training as OT


def _rel(a, b):
    den = float(b.abs().max())
    return float((a - b).abs().max()) / den if den > 0 else float((a - b).abs().max())


ANCHORS = ["pixel_combined_image_features", "pixel_masked_partially_black", "older_variation_with_mean", "older_variation_with_masked",
           "pixel_1_channel_colour_and_image_member", "flat_2_features", "older_H_1"]


@pytest.mark.parametrize("kind", R.ALL_KINDS)
@pytest.mark.parametrize("name", ANCHORS)
def test_reference_agrees_with_the_oracle_training_objects(name, kind):
    case = R.BY_NAME[name]
    x, t = R.make_inputs(case)
    p = [xi[..., :ft["nch"]].clone().requires_grad_() for xi, ft in zip(x, case["features"])]
    tt = [ti[..., :ft["nch"]] for ti, ft in zip(t, case["features"])]
    mask = lambda f: OT.non_zero_mask(tt[f])      # noqa: E731
    fts = []
    for f, ft in enumerate(case["features"]):     # FeatureTraining.initialize
        o = OT._FT("feature %d" % f, kind, (ft["w"], ft["vw"], 0.0), (ft["mw"] if ft["mask"] >= 0 else 0.0, 0.0, 0.0))
        o.predicted, o.target = [p[f]], [tt[f]]
        if ft["mask"] >= 0:
            o.mask = [mask(ft["mask"])]
        fts.append(o)
    cfts = []
    for k, c in enumerate(case["combined"]):      # CombinedFeatureTraining.initialize
        fc, fd, fi = c["triple"]
        o = OT._FT("combined %d" % k, kind, (c["w"], c["vw"], 0.0), (c["mw"] if c["mask"] >= 0 else 0.0, 0.0, 0.0))
        o.predicted, o.target = [p[fc] * (p[fd] + p[fi])], [tt[fc] * (tt[fd] + tt[fi])]
        if c["mask"] >= 0:
            o.mask = [mask(c["mask"])]
        cfts.append(o)
    loss = sum(o.loss(False) for o in fts + cfts)
    img = case["image"]
    if img:                                       # CombinedImageFeatureTraining.initialize
        parts = [cfts[k] for k in img["combined"]] + [fts[f] for f in img["features"]]
        o = OT._FT("Combined", kind, (img["w"], img["vw"], 0.0), (0.0, 0.0, 0.0))
        o.predicted, o.target = [sum(q.predicted[0] for q in parts)], [sum(q.target[0] for q in parts)]
        loss = loss + o.loss(False)
    grads = torch.autograd.grad(loss, p, allow_unused=True)
    ref = R.evaluate(case, kind, x, t)
    assert abs(ref["loss"] - float(loss)) <= 1e-12 * max(abs(float(loss)), ref["abs_sum"]), (ref["loss"], float(loss))
    for f, (g, ft) in enumerate(zip(grads, case["features"])):
        if g is None:
            assert ref["dpred"][f] is None, f
            continue
        assert _rel(ref["dpred"][f][..., :ft["nch"]], g) < 1e-9, (f, _rel(ref["dpred"][f][..., :ft["nch"]], g))
        assert not ref["dpred"][f][..., ft["nch"]:].any(), "a channel the feature does not have carries a gradient"


def test_masked_mean_with_an_empty_mask_is_zero_and_counts_are_integers():
    case = R.BY_NAME["pixel_masked_all_black"]
    x, t = R.make_inputs(case)
    ref = R.evaluate(case, "SMAPE", x, t)
    assert not ref["mask_sums"].any()
    assert ref["dpred"][1] is None                # feature 1 has a masked weight only: nothing depends on it
    case = R.BY_NAME["pixel_masked_partially_black"]
    x, t = R.make_inputs(case)
    ms = R.evaluate(case, "SMAPE", x, t)["mask_sums"]
    n = case["B"] * case["H"] * case["W"]
    assert 0 < ms[0] < n and ms[0] == ms[1] == ms[2] == ms[R.MAX_FEATURES] and ms[0] == ms[0].round() and not ms[3]
    case = R.BY_NAME["pixel_masked_all_ones"]
    x, t = R.make_inputs(case)
    assert R.evaluate(case, "SMAPE", x, t)["mask_sums"][0] == case["B"] * case["H"] * case["W"]


def test_fused_inversion_of_the_reference():
    """z == 0 exactly is planted and gives p == 0 with gradient 0 (log1p) or std (linear); z < 0 occurs."""
    case = R.BY_NAME["flat_fused_z_exactly_0"]
    x, t = R.make_inputs(case)
    ref = R.evaluate(case, "SQUARED", x, t)
    zero = x[0] == 0
    assert int(zero.sum()) > 10 and not ref["pred_inv"][0][zero].any() and not ref["dpred"][0][zero].any()
    assert (x[0] * 1.5 < 0).any()
    zero = x[1] == 0
    assert int(zero.sum()) > 10 and ref["dpred"][1][zero].abs().min() > 0


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_case_inputs_kernel_and_float32_floor(case):
    assert case["kernel"] in R.PATHS and R.expected_path(case, {}) == R.PATHS[case["kernel"]], "the case does not reach the kernel it names"
    if all(ft["fused"] is None for ft in case["features"]):
        assert R.expected_path(case, {"DD_LOSS_SIMPLE": "0", "DD_LOSS_GENERAL": "0"}) == 2
    assert case["family"] in ("dyadic", "continuous") and set(case["kinds"]) <= set(R.KINDS)
    assert len(case["features"]) <= R.MAX_FEATURES and len(case["combined"]) <= R.MAX_COMBINED
    x, t = R.make_inputs(case)
    for xi in x + t:
        assert torch.equal(xi.float().double(), xi), "inputs must be fp32 values"
    for kind in case["kinds"]:
        note = R.check_family(case, kind, x, t)
        r64, r32 = R.evaluate(case, kind, x, t), R.evaluate(case, kind, x, t, torch.float32)
        worst = 0.0
        for g64, g32 in zip(r64["dpred"], r32["dpred"]):
            assert (g64 is None) == (g32 is None)
            if g64 is not None and float(g64.norm()) > 0:
                worst = max(worst, float((g32.double() - g64).norm() / g64.norm()))
        loss_err = abs(r32["loss"] - r64["loss"]) / r64["abs_sum"] if r64["abs_sum"] > 0 else abs(r32["loss"] - r64["loss"])
        print("%s %s: %s | float32 reference vs float64: loss %.2e of sum|w term|, worst dpred rel-L2 %.2e" % (case["name"], kind, note, loss_err, worst))
        # the float32 evaluation of the reference itself stays far below the device gates (5e-6 dpred, 2e-5 loss): the gates have room
        assert worst <= 1.25e-6 and loss_err <= 5e-6, (case["name"], kind, worst, loss_err)
