"""Float64 / numpy restatement of dd_loss_previews (include/dd_hip.h) for tests/test_previews.py (CPU) and tests/test_gpu_previews.py (-m gpu),
written with the conventions of tests/loss_ref.py: a 1-channel pass is broadcast to 3 channels, combined = colour x (direct + indirect),
image = sum of its members.  Nothing here looks at the kernel: no grid, no packing, no per-pixel loop.

A CASE is a plain dict:
    B, H, W, nch: [channels of feature f, 1 or 3], combined: [(colour, direct, indirect)], image: {"combined": [...], "features": [...]} or None
The tensors that go with it are SIDES: {"source" | "prediction" | "target": [array [B, H, W, nch[f]] per feature]}, float64 arrays that hold
fp32-representable values.

Arithmetic.  The value of a source / prediction / target panel is formed in float64 and multiplied by the exposure; for a FEATURE slot the
device's only operation is that one fp32 multiply, which is repeated here in np.float32 (IEEE: the same bits on any machine).  The
difference panel is |channel-summed LossDifference| * error_gain, restated in np.float32 operation by operation in the order include/dd_hip.h
documents (d = p - t; the term; the channels added in order from 0; abs; times gain): SMAPE divides by |p| + |t| + 0.01, which is not
exact in fp32 for any inputs, so a float64 value could sit on the other side of a threshold without either being wrong.  Its operands (the
slot's prediction and target) come from the float64 values and must be fp32-exact, which the dyadic family guarantees.

Bytes are np.searchsorted(thresholds, v, side="right"); a pixel with a NaN channel is (255, 0, 255)."""
import numpy as np

MAX_FEATURES, MAX_COMBINED = 32, 8
IMAGE_SLOT = MAX_FEATURES + MAX_COMBINED
PANELS = ("source", "prediction", "target", "difference")
KINDS = {"DIFFERENCE": 1, "ABSOLUTE": 2, "SMOOTH_ABSOLUTE": 3, "SQUARED": 4, "SMAPE": 5}
EPSILON = 1e-2
MAGENTA = (255, 0, 255)


def slots_of(case):
    """every slot the case has: features, combined features, the image"""
    out = list(range(len(case["nch"]))) + [MAX_FEATURES + k for k in range(len(case["combined"]))]
    if case.get("image") and (case["image"]["combined"] or case["image"]["features"]):
        out.append(IMAGE_SLOT)
    return out


def _broadcast3(v):
    return np.broadcast_to(v, v.shape[:3] + (3,)) if v.shape[3] == 1 else v[..., :3]


def slot_value(case, feats, slot):
    """[B, H, W, 3] float64: the slot's value formed from one side's per-feature arrays"""
    feats = [np.asarray(f, dtype=np.float64) for f in feats]

    def combined(k):
        c, d, i = case["combined"][k]
        return _broadcast3(feats[c] * (feats[d] + feats[i]))
    if slot < MAX_FEATURES:
        return _broadcast3(feats[slot])
    if slot < IMAGE_SLOT:
        return combined(slot - MAX_FEATURES)
    total = np.zeros(feats[0].shape[:3] + (3,), dtype=np.float64)
    for k in case["image"]["combined"]:
        total = total + combined(k)
    for f in case["image"]["features"]:
        total = total + _broadcast3(feats[f])
    return total


def _exact32(v, what):
    v32 = v.astype(np.float32)
    ok = (v32.astype(np.float64) == v) | np.isnan(v)
    assert ok.all(), "%s is not exact in fp32: the difference panel's restatement needs fp32 operands" % what
    return v32


def difference_value(p, t, nch, kind, error_gain):
    """[B, H, W] float32: |sum over the first nch channels of LossDifference(p, t)| * error_gain, every operation in np.float32"""
    p, t = _exact32(p, "prediction"), _exact32(t, "target")
    eps, half, one = np.float32(EPSILON), np.float32(0.5), np.float32(1.0)
    s = np.zeros(p.shape[:3], dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(nch):
            pc, tc = p[..., c], t[..., c]
            d = pc - tc
            a = np.abs(d)
            if kind == "DIFFERENCE":
                term = d
            elif kind == "ABSOLUTE":
                term = a
            elif kind == "SMOOTH_ABSOLUTE":
                term = np.where(a < one, half * a * a, a - half)
            elif kind == "SQUARED":
                term = d * d
            else:
                assert kind == "SMAPE"
                term = a / (np.abs(pc) + np.abs(tc) + eps)
            s = s + term
        out = np.abs(s) * np.float32(error_gain)
    assert out.dtype == np.float32
    return out


def panel_values(case, sides, slot, panel, images, kind="ABSOLUTE", exposure=1.0, error_gain=1.0):
    """[len(images) * H, W, 3] float64: the values the bytes of one panel of one slot's mosaic are taken from"""
    idx = np.asarray(images, dtype=np.int64)
    e32 = np.float32(exposure)
    with np.errstate(all="ignore"):
        if panel == "difference":
            nch = 1 if (slot < MAX_FEATURES and case["nch"][slot] == 1) else 3
            g = difference_value(slot_value(case, sides["prediction"], slot)[idx], slot_value(case, sides["target"], slot)[idx], nch, kind, error_gain)
            v = np.repeat(g.astype(np.float64)[..., None], 3, axis=3)
        else:
            v = slot_value(case, sides[panel], slot)[idx]
            if slot < MAX_FEATURES:      # the device's one operation, repeated in fp32
                v = (_exact32(v, "a feature") * e32).astype(np.float64)
            else:
                v = v * np.float64(e32)
    return v.reshape(len(idx) * v.shape[1], v.shape[2], 3)


def quantise(v, thresholds):
    """uint8 of the same shape [..., 3]: the number of thresholds <= v; a pixel with a NaN channel is magenta"""
    thresholds = np.asarray(thresholds)
    assert thresholds.shape == (255,) and (np.diff(thresholds) > 0).all()
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v).any(axis=-1)
    out = np.searchsorted(thresholds.astype(np.float64), np.where(np.isnan(v), 0.0, v), side="right").astype(np.uint8)
    out[nan] = MAGENTA
    return out


def panel_names(mask):
    return [p for bit, p in enumerate(PANELS) if mask & (1 << bit)]


def mosaic_values(case, sides, slot, mask, images, **kw):
    """[len(images) * H, P * W, 3] float64: the panels of `mask` left to right in bit order, image row r = batch image images[r]"""
    return np.concatenate([panel_values(case, sides, slot, p, images, **kw) for p in panel_names(mask)], axis=1)


def mosaics(case, sides, slots, mask, images, thresholds, **kw):
    """uint8 [len(slots), len(images) * H, P * W, 3]: what dd_loss_previews writes"""
    return np.stack([quantise(mosaic_values(case, sides, s, mask, images, **kw), thresholds) for s in slots])


def near_threshold(v, thresholds, rel):
    """bool, shape of v: the value lies within a relative `rel` of a threshold"""
    t = np.asarray(thresholds, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    j = np.clip(np.searchsorted(t, v), 1, len(t) - 1)
    near = np.minimum(np.abs(v - t[j - 1]) / t[j - 1], np.abs(v - t[j]) / t[j])
    return near <= rel


# ------------------------------------------------------------------------------------------------------------------ inputs
def dyadic_sides(case, seed):
    """every raw, prediction and target value is k / 16 with |k| <= 32: products and sums of up to 8 members are exact in fp32"""
    rng = np.random.default_rng(seed)
    shape = (case["B"], case["H"], case["W"])
    return {side: [rng.integers(-32, 33, shape + (n,)).astype(np.float64) / 16 for n in case["nch"]] for side in PANELS[:3]}


def radiance_sides(case, seed):
    """non-negative fp32 radiances, most of them inside the display range: the image sum has no cancellation"""
    rng = np.random.default_rng(seed)
    shape = (case["B"], case["H"], case["W"])
    scale = 1.0 / max(1, len(case["combined"]) + 1)
    return {side: [(rng.random(shape + (n,)) * scale).astype(np.float32).astype(np.float64) for n in case["nch"]] for side in PANELS[:3]}


# a colour / direct / indirect triple, one more 3-channel pass and a 1-channel pass; the image sums the triple and the two passes
SMALL = {"nch": [3, 3, 3, 3, 1], "combined": [(0, 1, 2)], "image": {"combined": [0], "features": [3, 4]}}
# the 1-channel pass as the colour of a second triple
TWO_TRIPLES = {"nch": [3, 3, 3, 1, 3, 3], "combined": [(0, 1, 2), (3, 4, 5)], "image": {"combined": [0, 1], "features": [3]}}


def case(base, B, H, W):
    return dict(base, B=B, H=H, W=W)
