"""Float64 restatement of ONE dd_loss_desc (include/dd_hip.h) for the op-level tests of the loss kernels: tests/test_loss_ref.py (CPU) and
tests/test_gpu_loss_ops.py (-m gpu).  Written with oracle/tf_ops.py (loss_difference, signed_expm1) and the formulas of
oracle/training.py::_FT (mean, masked mean with the batch-global count, variation over the concatenated horizontal and vertical pairs,
combined = colour x (direct + indirect) with 1-channel passes broadcast, image = sum of its members); gradients come from torch.autograd.
Nothing here looks at the kernels: no grid, no dispatch, no per-pixel loop.

A CASE is a plain dict:
    name, kernel ("flat" / "pixel" / "older": the kernel the case is aimed at with the library's default switches), family ("dyadic" /
    "continuous"), B, H, W, seed, kinds (names of LossDifference kinds), grad_scale,
    features: [{nch, pred_ld, target_ld, w, vw, mw, mask, fused}]   w / vw / mw: mean, variation, masked-mean weight; mask: the feature whose
                                                                    target defines the mask (-1: none); fused: None or (log1p, mean, std)
    combined: [{triple: (colour, direct, indirect), w, vw, mw, mask}]
    image: {combined: [indices into combined], features: [feature indices], w, vw}
    pred_offset: floats by which the device test shifts every prediction pointer (0 or 1)
    black: None, or (feature, "all" / "part" / "none"): how much of that feature's TARGET is exactly zero (the mask source)
    zero_x: plant exact zeros in the fused inputs (z == 0 exactly with mean 0)
The tensors that go with it: x[f] and t[f], [B, H, W, 3] each; a feature uses the first nch channels (x is the prediction, or the STANDARDIZED
prediction of a fused feature, whose 3 channels are all inverted and stored as the kernels do).

Input families
    dyadic      every value is k / 16, integer k in [-32, 32]: all derived source values (products of combined features, sums of up to 8 image
                members, neighbour differences) are exact in fp32, so every sign, mask and tie (p == t, p == 0, |p - t| == 1) is the same on
                the device and here, and torch's conventions at the kinks (abs'(0) = 0, where(a < 1, ...)) are the expected values.
    continuous  randn rounded to fp32 (fused inversion leaves the dyadic grid).  With ABSOLUTE / SMAPE every |p - t| of every source must be
                >= MARGIN (|p| + |t|), with SMAPE every |p| too: a condition on the inputs (the seed is chosen for it), never an exclusion."""
import torch

from oracle import tf_ops as T

MAX_FEATURES, MAX_COMBINED = 32, 8
KINDS = {"DIFFERENCE": 1, "ABSOLUTE": 2, "SMOOTH_ABSOLUTE": 3, "SQUARED": 4, "SMAPE": 5}
ALL_KINDS = tuple(KINDS)
SMOOTH_KINDS = ("DIFFERENCE", "SMOOTH_ABSOLUTE", "SQUARED")      # kinds without a kink condition on continuous inputs
EPSILON = 1e-2
MARGIN = 1e-4
PATHS = {"flat": 0, "pixel": 1, "older": 2}                      # dd_loss_head_path_count index of each kernel


# ------------------------------------------------------------------------------------------------------------------ the reference
def invert(x, fused):
    """FeatureStandardization.invert_standardization with the descriptor's (log1p, mean, std)."""
    log1p, mean, std = fused
    z = x * std + mean
    return T.signed_expm1(z) if log1p else z


def _variation_pairs(v):
    """x[., j+1] - x[., j] and x[i+1, .] - x[i, .], each flattened per image (oracle/training.py::_FT.variation_mean)."""
    return v[:, :, 1:, :] - v[:, :, :-1, :], v[:, 1:, :, :] - v[:, :-1, :, :]


def _source_terms(p, t, mask, w, vw, mw, kind):
    """[(weight, per-element values that are SUMMED into the term)] of one source; p, t [B,H,W,C], mask [B,H,W] or None."""
    out = []
    b = p.shape[0]
    if w != 0:
        d = T.loss_difference(p, t, kind, EPSILON)
        out.append((w, d / d.numel()))                                           # mean over B*H*W of the channel sum
    if vw != 0:
        (hp, vp), (ht, vt) = _variation_pairs(p), _variation_pairs(t)
        d = torch.cat([T.loss_difference(hp, ht, kind, EPSILON).reshape(b, -1), T.loss_difference(vp, vt, kind, EPSILON).reshape(b, -1)], dim=1)
        out.append((vw, d / d.numel()))
    if mw != 0 and mask is not None:
        msum = mask.sum()
        if float(msum) > 0:                                                      # count 0: the masked mean is 0
            out.append((mw, T.loss_difference(p, t, kind, EPSILON) * mask / msum))
    return out


def _broadcast3(v):
    return v.expand(-1, -1, -1, 3)


def sources(case, p, t):
    """[(name, prediction, target, mask feature or -1, weights (w, vw, mw))] of every source of the case from the per-feature values
    p[f], t[f] ([B,H,W,nch])."""
    out = []
    for f, ft in enumerate(case["features"]):
        out.append(("feature %d" % f, p[f], t[f], ft["mask"], (ft["w"], ft["vw"], ft["mw"])))
    comb = []
    for k, c in enumerate(case["combined"]):
        fc, fd, fi = c["triple"]
        cp, ct = _broadcast3(p[fc] * (p[fd] + p[fi])), _broadcast3(t[fc] * (t[fd] + t[fi]))
        comb.append((cp, ct))
        out.append(("combined %d" % k, cp, ct, c["mask"], (c["w"], c["vw"], c["mw"])))
    img = case.get("image")
    if img and (img["w"] != 0 or img["vw"] != 0) and (img["combined"] or img["features"]):
        members = [comb[k] for k in img["combined"]] + [(_broadcast3(p[f]), _broadcast3(t[f])) for f in img["features"]]
        out.append(("image", sum(m[0] for m in members), sum(m[1] for m in members), -1, (img["w"], img["vw"], 0.0)))
    return out


def feature_values(case, x, t, dtype):
    """x, t -> leaves (what the gradient is taken against), per-feature prediction and target [B,H,W,nch], inverted predictions {f: [B,H,W,3]}"""
    leaves = [xi.to(dtype).clone().requires_grad_() for xi in x]
    p, tt, pred_inv = [], [], {}
    for f, ft in enumerate(case["features"]):
        v = leaves[f]
        if ft["fused"] is not None:
            v = pred_inv[f] = invert(v, ft["fused"])
        p.append(v[..., :ft["nch"]])
        tt.append(t[f].to(dtype)[..., :ft["nch"]])
    return leaves, p, tt, pred_inv


def mask_of(case, tt, f):
    """Conv2dUtilities.non_zero_mask of feature f's target: sign(sum_c |t_c|), [B,H,W]"""
    return torch.sign(torch.abs(tt[f]).sum(dim=3))


def evaluate(case, kind, x, t, dtype=torch.float64):
    """-> dict(loss, abs_sum, dpred [per feature, [B,H,W,3], None for a feature nothing depends on], pred_inv {f: tensor}, mask_sums [40])."""
    leaves, p, tt, pred_inv = feature_values(case, x, t, dtype)
    loss = torch.zeros((), dtype=dtype)
    abs_sum = 0.0
    mask_sums = torch.zeros(MAX_FEATURES + MAX_COMBINED, dtype=torch.float64)
    for name, sp, st, mf, (w, vw, mw) in sources(case, p, tt):
        mask = mask_of(case, tt, mf) if mf >= 0 else None
        if mw != 0 and mask is not None and not name.startswith("image"):
            slot = int(name.split()[1]) + (MAX_FEATURES if name.startswith("combined") else 0)
            mask_sums[slot] = float(mask.sum())
        for weight, values in _source_terms(sp, st, mask, w, vw, mw, kind):
            loss = loss + weight * values.sum()
            abs_sum += abs(weight) * float(values.detach().abs().sum())
    grads = [None] * len(leaves)
    if loss.requires_grad:
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    gs = case.get("grad_scale", 1.0)
    return {"loss": float(loss.detach()), "abs_sum": abs_sum, "dpred": [None if g is None else (g * gs).detach() for g in grads],
            "pred_inv": {f: v.detach() for f, v in pred_inv.items()}, "mask_sums": mask_sums}


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(case):
    """Seeded x[f], t[f] ([B,H,W,3], float64 holding fp32-representable values) of the case's family."""
    g = torch.Generator().manual_seed(case["seed"])
    shape = (case["B"], case["H"], case["W"], 3)
    x, t = [], []
    for f, ft in enumerate(case["features"]):
        if case["family"] == "dyadic":
            assert ft["fused"] is None, "expm1 leaves the dyadic grid"
            xi = torch.randint(-32, 33, shape, generator=g).double() / 16
            ti = torch.randint(-32, 33, shape, generator=g).double() / 16
        else:
            xi = torch.randn(shape, generator=g, dtype=torch.float32).double()
            ti = torch.randn(shape, generator=g, dtype=torch.float32).double()
        x.append(xi)
        t.append(ti)
    if case.get("black"):
        f, how = case["black"]
        if how == "all":
            t[f].zero_()
        elif how == "part":                      # whole pixels black: rows of the upper third and a scatter of single pixels
            t[f][:, :max(1, case["H"] // 3)] = 0
            t[f][torch.rand(shape[:3], generator=g) < 0.1] = 0
        else:                                    # no black pixel at all
            dark = torch.abs(t[f]).sum(dim=3) == 0
            t[f][dark] = 1.0 / 16
    if case.get("zero_x"):
        for f, ft in enumerate(case["features"]):
            if ft["fused"] is not None:
                x[f][torch.rand(shape, generator=g) < 0.05] = 0
    return x, t


def all_source_values(case, x, t, dtype, variation=True):
    """[(name, p, t)] of every value a loss term of the case is evaluated on: the sources and, with a variation weight, their neighbour
    differences."""
    _, p, tt, _ = feature_values(case, x, t, dtype)
    out = []
    for name, sp, st, _, (w, vw, mw) in sources(case, p, tt):
        sp, st = sp.detach(), st.detach()
        out.append((name, sp, st))
        if variation and vw != 0:
            (hp, vp), (ht, vt) = _variation_pairs(sp), _variation_pairs(st)
            out += [(name + " horizontal pairs", hp, ht), (name + " vertical pairs", vp, vt)]
    return out


def check_family(case, kind, x, t):
    """Asserts the family's condition on the inputs; returns a one-line description for the test's output."""
    if case["family"] == "dyadic":
        ties = total = 0
        for (name, p64, t64), (_, p32, t32) in zip(all_source_values(case, x, t, torch.float64), all_source_values(case, x, t, torch.float32)):
            assert torch.equal(p32.double(), p64) and torch.equal(t32.double(), t64), "%s: %s is not exact in fp32" % (case["name"], name)
            d = (p64 - t64).abs()
            ties += int((d == 0).sum()) + int((d == 1).sum()) + int((p64 == 0).sum())
            total += d.numel()
        return "dyadic: every source value bit-equal in fp32 and f64; %d ties (p == t, |p - t| == 1, p == 0) in %d elements" % (ties, total)
    worst_d = worst_p = float("inf")
    for name, p, tt in all_source_values(case, x, t, torch.float64):
        scale = (p.abs() + tt.abs()).clamp_min(1e-300)
        worst_d = min(worst_d, float(((p - tt).abs() / scale).min()))
        worst_p = min(worst_p, float((p.abs() / scale).min()))
    if kind in ("ABSOLUTE", "SMAPE"):
        assert worst_d >= MARGIN, "%s %s: some |p - t| is %.2e (|p| + |t|): choose another seed" % (case["name"], kind, worst_d)
    if kind == "SMAPE":
        assert worst_p >= MARGIN, "%s %s: some |p| is %.2e (|p| + |t|): choose another seed" % (case["name"], kind, worst_p)
    return "continuous: min |p - t| / (|p| + |t|) = %.2e, min |p| / (|p| + |t|) = %.2e" % (worst_d, worst_p)


# ------------------------------------------------------------------------------------------------------------------ which kernel
def expected_path(case, env):
    """dd_loss_head_path_count index the case must move, from the case and the library's switches in `env` (include/dd_hip.h: features-only
    descriptors whose blocks are flat 16-byte-aligned float4 streams -> flat-stream kernel; no variation term -> per-pixel kernel; else the
    older kernel; a fused inversion exists only in the first two, whatever the switches say)."""
    def on(name):
        return not env.get(name, "1").startswith("0")
    feats, img = case["features"], case.get("image")
    fused_any = any(ft["fused"] is not None for ft in feats)
    use_image = bool(img) and (img["w"] != 0 or img["vw"] != 0) and bool(img["combined"] or img["features"])
    variation = any(ft["vw"] != 0 for ft in feats) or any(c["vw"] != 0 for c in case["combined"]) or bool(img and img["vw"] != 0)
    masked = any(ft["mw"] != 0 and ft["mask"] >= 0 for ft in feats)
    flat = not case["combined"] and not use_image and not variation and not masked and (case["B"] * case["H"] * case["W"] * 3) % 4 == 0
    for ft in feats:
        if ft["w"] != 0 or ft["fused"] is not None:
            flat = flat and ft["pred_ld"] == 3 and ft["target_ld"] == 3 and ft["nch"] in (1, 3) and case.get("pred_offset", 0) == 0
    if flat and (on("DD_LOSS_SIMPLE") or fused_any):
        return 0
    if not variation and (on("DD_LOSS_GENERAL") or fused_any):
        return 1
    return 2


# ------------------------------------------------------------------------------------------------------------------ the case table
def feat(w=0.0, vw=0.0, mw=0.0, mask=-1, nch=3, fused=None, pred_ld=3, target_ld=3):
    return {"nch": nch, "pred_ld": pred_ld, "target_ld": target_ld, "w": w, "vw": vw, "mw": mw, "mask": mask, "fused": fused}


def comb(triple, w=0.0, vw=0.0, mw=0.0, mask=-1):
    return {"triple": tuple(triple), "w": w, "vw": vw, "mw": mw, "mask": mask}


def case(name, kernel, family, shape, features, combined=(), image=None, kinds=ALL_KINDS, seed=1, **extra):
    c = {"name": name, "kernel": kernel, "family": family, "B": shape[0], "H": shape[1], "W": shape[2], "features": list(features),
         "combined": list(combined), "image": image, "kinds": tuple(kinds), "seed": seed, "grad_scale": 1.0, "pred_offset": 0,
         "black": None, "zero_x": False}
    c.update(extra)
    return c


LOG1P, LINEAR = (1, 0.25, 1.5), (0, 0.5, 0.75)      # (log1p, mean, std) of a fused inversion; all fp32-representable
# all weights are multiples of 1/8: exact in fp32
_W4 = [feat(w=1.0), feat(w=0.75), feat(w=1.25), feat(w=0.5)]
_TRIPLE = [comb((0, 1, 2), w=0.875)]
_IMAGE = {"combined": [0], "features": [3], "w": 1.5, "vw": 0.0}


def _pixel_count_cases():
    out = []
    for shape in ((1, 5, 7), (1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 1, 257)):
        n = shape[0] * shape[1] * shape[2]
        out.append(case("ragged_pixel_%dpx" % n, "pixel", "dyadic", shape, _W4, _TRIPLE, dict(_IMAGE), seed=n))
        out.append(case("ragged_older_%dpx" % n, "older", "dyadic", shape, [feat(w=1.0, vw=0.5), feat(w=0.75), feat(vw=1.25), feat(w=0.5)],
                        [comb((0, 1, 2), w=0.875, vw=0.25)], dict(_IMAGE, vw=0.75), seed=n + 1))
    return out


WRAP_SHAPE, WRAP_SHAPE_3 = (5, 400, 400), (6, 512, 512)      # 800 000 and 1 572 864 pixels: every kernel's grid-stride loop wraps
CASES = [
    # ---- flat-stream kernel: features only
    case("flat_1_feature", "flat", "dyadic", (2, 8, 10), [feat(w=1.0)], seed=11),
    case("flat_2_features", "flat", "dyadic", (2, 8, 10), [feat(w=1.0), feat(w=0.625)], seed=12),
    case("flat_17_features", "flat", "dyadic", (2, 6, 8), [feat(w=0.125 * (1 + f % 7)) for f in range(17)], seed=13),
    case("flat_zero_weight_in_the_middle", "flat", "dyadic", (2, 8, 10), [feat(w=1.0), feat(w=0.0), feat(w=0.75)], seed=14),
    case("flat_1_channel_feature", "flat", "dyadic", (2, 8, 10), [feat(w=1.0), feat(w=0.75, nch=1)], seed=15),
    case("flat_fused_log1p", "flat", "continuous", (2, 6, 8), [feat(w=1.0, fused=LOG1P), feat(w=0.75, fused=LOG1P)], seed=101),
    case("flat_fused_linear", "flat", "continuous", (2, 6, 8), [feat(w=1.0, fused=LINEAR), feat(w=0.75, fused=LINEAR)], seed=100),
    case("flat_fused_z_exactly_0", "flat", "continuous", (2, 8, 10), [feat(w=1.0, fused=(1, 0.0, 1.5)), feat(w=0.75, fused=(0, 0.0, 0.75))],
         kinds=SMOOTH_KINDS, seed=100, zero_x=True),
    case("flat_fused_on_some_features", "flat", "continuous", (2, 6, 8), [feat(w=1.0, fused=LOG1P), feat(w=0.75), feat(w=0.5, fused=LINEAR, nch=1)],
         seed=101),
    # ---- per-pixel kernel
    case("pixel_combined_only", "pixel", "dyadic", (2, 8, 10), [feat(), feat(), feat()], _TRIPLE, seed=21),
    case("pixel_image_only", "pixel", "dyadic", (2, 8, 10), [feat(), feat(), feat(), feat()], [comb((0, 1, 2))], dict(_IMAGE), seed=22),
    case("pixel_combined_image_features", "pixel", "dyadic", (2, 8, 10), _W4, _TRIPLE, dict(_IMAGE), seed=23),
    case("pixel_masked_partially_black", "pixel", "dyadic", (2, 9, 10), [feat(w=1.0, mw=0.5, mask=0), feat(mw=0.75, mask=0), feat(w=0.25, mw=1.0, mask=0),
                                                                        feat(w=0.5)],
         [comb((0, 1, 2), w=0.875, mw=0.625, mask=0)], dict(_IMAGE), seed=24, black=(0, "part")),
    case("pixel_masked_all_black", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0, mw=0.5, mask=0), feat(mw=0.75, mask=0), feat(w=0.25, mw=1.0, mask=0)],
         [comb((0, 1, 2), mw=0.625, mask=0)], seed=25, black=(0, "all")),
    case("pixel_masked_all_ones", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0, mw=0.5, mask=0), feat(mw=0.75, mask=0), feat(w=0.25, mw=1.0, mask=0)],
         [comb((0, 1, 2), w=0.5, mw=0.625, mask=0)], seed=26, black=(0, "none")),
    case("pixel_1_channel_colour_and_image_member", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0, nch=1), feat(w=0.75), feat(w=1.25), feat(w=0.5, nch=1)],
         _TRIPLE, dict(_IMAGE), seed=27),
    case("pixel_32_features_8_triples", "pixel", "dyadic", (1, 9, 15), [feat(w=0.125 * (1 + f % 5), nch=1 if f == 30 else 3) for f in range(32)],
         [comb((3 * k, 3 * k + 1, 3 * k + 2), w=0.25 * (1 + k % 3)) for k in range(8)],
         {"combined": list(range(8)), "features": [24, 25, 26, 27, 28, 29, 30, 31], "w": 1.5, "vw": 0.0}, seed=28),
    case("pixel_fused_next_to_combined", "pixel", "continuous", (1, 5, 8), [feat(w=1.0, fused=LOG1P), feat(w=0.75, fused=LINEAR), feat(w=1.25, fused=LOG1P),
                                                                            feat(w=0.5, fused=LINEAR, nch=1)],
         _TRIPLE, dict(_IMAGE), seed=103),
    case("pixel_2_channel_feature", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0), feat(w=0.75, nch=2)], seed=30),
    # ---- older kernel: variation terms
    case("older_variation_alone", "older", "dyadic", (2, 8, 10), [feat(vw=1.0), feat(vw=0.75, nch=1), feat(vw=0.5)], [comb((0, 1, 2), vw=0.875)],
         {"combined": [0], "features": [1], "w": 0.0, "vw": 1.5}, seed=31),
    case("older_variation_with_mean", "older", "dyadic", (2, 8, 10), [feat(w=1.0, vw=0.5), feat(w=0.75, vw=0.25), feat(w=1.25), feat(vw=0.5)],
         [comb((0, 1, 2), w=0.875, vw=0.375)], dict(_IMAGE, vw=0.75), seed=32),
    case("older_variation_with_masked", "older", "dyadic", (2, 9, 10), [feat(w=1.0, vw=0.5, mw=0.5, mask=0), feat(vw=0.25, mw=0.75, mask=0), feat(w=1.25),
                                                                       feat(vw=0.5)],
         [comb((0, 1, 2), vw=0.375, mw=0.625, mask=0)], dict(_IMAGE, vw=0.75), seed=33, black=(0, "part")),
    case("older_variation_continuous", "older", "continuous", (1, 5, 8), [feat(w=1.0, vw=0.5), feat(w=0.75), feat(vw=1.25)], [comb((0, 1, 2), w=0.875, vw=0.375)],
         {"combined": [0], "features": [], "w": 1.5, "vw": 0.75}, kinds=SMOOTH_KINDS, seed=100),
    case("older_H_1", "older", "dyadic", (2, 1, 16), [feat(w=1.0, vw=0.5), feat(vw=0.75), feat(w=0.5)], [comb((0, 1, 2), w=0.875, vw=0.375)], seed=35),
    case("older_W_1", "older", "dyadic", (2, 16, 1), [feat(w=1.0, vw=0.5), feat(vw=0.75), feat(w=0.5)], [comb((0, 1, 2), w=0.875, vw=0.375)], seed=36),
    case("older_2x2", "older", "dyadic", (3, 2, 2), [feat(w=1.0, vw=0.5), feat(vw=0.75), feat(w=0.5)], [comb((0, 1, 2), w=0.875, vw=0.375)], seed=37),
    # ---- dispatch edges: features-only descriptors that must leave the flat-stream kernel and still be right
    case("edge_1x5x7", "pixel", "dyadic", (1, 5, 7), [feat(w=1.0), feat(w=0.75, nch=1)], seed=41),
    case("edge_pred_offset_by_one_float", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0), feat(w=0.75, nch=1)], seed=42, pred_offset=1),
    case("edge_pred_ld_4_target_ld_4", "pixel", "dyadic", (2, 8, 10), [feat(w=1.0, pred_ld=4, target_ld=4), feat(w=0.75, nch=1, pred_ld=4, target_ld=4)], seed=43),
    case("flat_continuous_features", "flat", "continuous", (2, 6, 8), [feat(w=1.0), feat(w=0.75, nch=1)], seed=100),
] + _pixel_count_cases() + [
    # ---- sizes at which the grid-stride loops wrap (dyadic: exact)
    case("wrap_flat_800k", "flat", "dyadic", WRAP_SHAPE, [feat(w=1.0), feat(w=0.75, nch=1)], seed=51),
    case("wrap_flat_1572k", "flat", "dyadic", WRAP_SHAPE_3, [feat(w=1.0)], seed=52),
    case("wrap_pixel_800k", "pixel", "dyadic", WRAP_SHAPE, [feat(w=1.0, mw=0.5, mask=0), feat(w=0.75), feat(w=1.25), feat(w=0.5)], _TRIPLE, dict(_IMAGE), seed=53,
         black=(0, "part")),
    case("wrap_older_800k", "older", "dyadic", WRAP_SHAPE, [feat(w=1.0, vw=0.5), feat(vw=0.75, nch=1)], seed=54),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_KINDS = [(c["name"], k) for c in CASES for k in c["kinds"]]
