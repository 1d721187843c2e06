"""Float64 reference of the input assembly (standardise -> local variance -> pixel record -> network input) with a running error budget,
the input families and the case tables that tests/test_input_ref.py (CPU) and tests/test_gpu_input_ops.py (-m gpu) share.

The reference is plain torch float64 on whole images: no tiles, mirroring by index arithmetic (mirror_index), one code path.  The same code path
evaluated in torch.float32 (dtype=, form="div" | "rcp") is the f32 EMULATION, and evaluated with a `mut` dictionary it is a MUTANT (MUTANTS).

THE BUDGET.  Next to every value v the functions return e >= 0, a first-order bound on |fl(v) - v| for ANY float32 evaluation of the same
formulas, carried in float64 from the reference's own intermediates (never from device output) under the standard model fl(a op b) =
(a op b)(1 + d), |d| <= u:
    U = 2^-24          unit roundoff of float32 (round to nearest): an add, a subtraction, a multiplication or a division adds U*|result|;
                       one ulp of a float32 x is at most 2*U*|x| (ULP)
    LOG1P_ULPS = 2     log1pf: 2 ulp, the OpenCL C accuracy table ("log1p <= 2 ulp") that the ROCm device library is written to; the HIP
                       math API table documents 1 ulp, so 2 is the larger of the two published figures           -> 4*U*|log1p|
    RCP_ULPS = 1       v_rcp_f32: 1 ulp (CDNA instruction set reference, V_RCP_F32)                               -> 2*U*|1/d|
    a sum of n terms   (n-1)*U*sum|terms| in any order (Higham, Accuracy and Stability of Numerical Algorithms, (4.4), to first order)
    * (1/n)            2*U*|result|: the constant 1/9, 0.2 or 1/3 rounded to float32 (U) and the multiplication (U); it covers "/ n" (U) too
    var * rcp(d)       3*U*|result|: the reciprocal (2U) and the multiplication (U); it covers the division form (U) too
    max(m, eps)        the budget of m where m + e_m >= eps, else 0 (the clamp is exact)
    inputs             a budget e_x of an operand enters through the derivative: e(x^2) = 2|x|e_x, e(a/d) = e_a/d + |a|e_d/d^2, ...
A fused multiply-add (meansq - mean*mean contracts to one) rounds once where the model charges twice: the bound holds for it too.  mean,
inv_std and epsilon are taken as the float32 values the kernel is handed, the pixel values are float32-representable: no budget of their own.

THE GATE (tests/test_gpu_input_ops.py, mirrored here by worst_ratio): every written element has |got - ref| <= 2*e + r_T(ref), r_T = half an
ulp of the storage type at |ref| (0 for float32).  A float32 value within e of ref, rounded to nearest in T, is within 2e + r_T of ref: the
representable neighbour R of ref has |R - ref| <= r_T, and the rounded value is at least as close to the float32 value as R is."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
ULP = 2.0 * U
LOG1P_ULPS = 2.0
RCP_ULPS = 1.0
F64 = torch.float64


def f32(x):
    """The float32 value the kernel is handed for a Python float."""
    return float(np.float32(x))


def params(use_log1p=0, mean=0.0, inv_std=1.0, use_variance=1, variance_before=0, mode_neighbor=0, relative=1, compress=1, epsilon=1e-4):
    """dd_feature_params as a dictionary (defaults: FeatureEngineering's uniform / relative / compressed / after standardisation)."""
    return dict(use_log1p=int(use_log1p), mean=f32(mean), inv_std=f32(inv_std), use_variance=int(use_variance), variance_before=int(variance_before),
                mode_neighbor=int(mode_neighbor), relative=int(relative), compress=int(compress), epsilon=f32(epsilon))


IDENTITY = dict(use_log1p=0, mean=0.0, inv_std=1.0, use_variance=0)
# VARIANCE_BRANCHES of tests/test_gpu_round2.py in dd_feature_params terms, plus the default, use_variance = 0 and the identity
BRANCHES = {
    "default": dict(),
    "neighbor_relative_compressed": dict(mode_neighbor=1),
    "uniform_absolute": dict(relative=0),
    "neighbor_absolute_per_channel": dict(mode_neighbor=1, relative=0, compress=0),
    "uniform_relative_per_channel": dict(compress=0),
    "before_standardization": dict(variance_before=1),
    "before_standardization_neighbor_per_channel": dict(variance_before=1, mode_neighbor=1, compress=0),
    "no_variance": dict(use_variance=0),
    "identity": IDENTITY,
}
NO_MUTATION = dict(border="symmetric", uniform_count=9.0, diagonal=False, swap_source=False, epsilon=None, compress_sum=False, swap_ch12=False,
                   dst_shift=0)
# "clamp" is EQUIVALENT to the symmetric mirror for a halo of one pixel (-1 -> 0 and n -> n-1 under both): it cannot break any gate and
# test_input_ref.py asserts that it changes nothing; "reflect" (-1 -> 1, n -> n-2) and "zero" are the border mistakes that a 3x3 window can show.
MUTANTS = {
    "clamp_to_edge": dict(border="clamp"),
    "reflect_border": dict(border="reflect"),
    "zero_border": dict(border="zero"),
    "eighth_for_ninth": dict(uniform_count=8.0),
    "neighbor_with_diagonal": dict(diagonal=True),
    "variance_source_swapped": dict(swap_source=True),
    "epsilon_1e-3": dict(epsilon=1e-3),
    "compress_by_sum": dict(compress_sum=True),
    "channels_1_2_swapped": dict(swap_ch12=True),
    "dst_ch_off_by_one": dict(dst_shift=1),
}
EQUIVALENT_MUTANTS = ("clamp_to_edge",)


def mutation(name):
    return dict(NO_MUTATION, **MUTANTS[name]) if name else NO_MUTATION


# ---------------------------------------------------------------------------------------------------------------- the operations
def mirror_index(i, n, border="symmetric"):
    """Source index along an axis of n samples for the coordinates i (LongTensor, may be < 0 or >= n)."""
    if border == "symmetric":
        return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))
    if border == "reflect":
        return torch.where(i < 0, -i, torch.where(i >= n, 2 * n - 2 - i, i)).clamp(0, n - 1)
    return i.clamp(0, n - 1)      # "clamp", and "zero" (masked by shifted())


def shifted(x, dy, dx, border="symmetric"):
    """x[b, y + dy, x + dx, c] over the whole image [B,H,W,C], the border resolved by mirror_index."""
    H, W = x.shape[1], x.shape[2]
    cy, cx = torch.arange(H) + dy, torch.arange(W) + dx
    y = x[:, mirror_index(cy, H, border)][:, :, mirror_index(cx, W, border)]
    if border == "zero":
        inside = ((cy >= 0) & (cy < H))[:, None] & ((cx >= 0) & (cx < W))[None, :]
        y = y * inside[None, :, :, None].to(y.dtype)
    return y


def standardize(v, fp, dtype=F64):
    """sign(v) log1p|v| if use_log1p, then (x - mean) * inv_std.  -> (value, budget)"""
    x = v.to(dtype)
    e = torch.zeros_like(v, dtype=F64)
    if fp["use_log1p"]:
        x = torch.sign(x) * torch.log1p(x.abs())
        e = LOG1P_ULPS * ULP * x.double().abs()
    d = x - fp["mean"]
    e = e + U * d.double().abs()
    s = d * fp["inv_std"]
    e = abs(fp["inv_std"]) * e + U * s.double().abs()
    return s, e


def _sum(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _scale(x, e, n, dtype, form):
    """x / n, or x * fl(1/n)"""
    y = x * torch.tensor(1.0 / n, dtype=dtype) if form == "rcp" else x / n
    return y, e / n + 2 * U * y.double().abs()


def taps(fp, mut=NO_MUTATION):
    if not fp["mode_neighbor"]:
        return [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    return [(0, 0), (-1, -1) if mut["diagonal"] else (-1, 0), (1, 0), (0, -1), (0, 1)]


def local_variance(x, ex, fp, dtype=F64, form="div", mut=NO_MUTATION):
    """E[x^2] - E[x]^2 over the 3x3 ("uniform") or plus-shaped ("neighbor") window, optionally / max(E[x]^2, eps), optionally the mean over the
    channels.  x [B,H,W,C] in dtype with the budget ex (float64).  -> (value [B,H,W,C or 1], budget)"""
    tp = taps(fp, mut)
    n = len(tp)
    xs = [shifted(x, a, b, mut["border"]) for a, b in tp]
    es = [shifted(ex, a, b, mut["border"]) for a, b in tp]
    s = _sum(xs)
    e_s = _sum(es) + (n - 1) * U * _sum([t.double().abs() for t in xs])
    sq = [t * t for t in xs]
    e_sq = [2 * t.double().abs() * et + U * q.double() for t, et, q in zip(xs, es, sq)]
    ss = _sum(sq)
    e_ss = _sum(e_sq) + (n - 1) * U * _sum([q.double() for q in sq])
    cnt = n if fp["mode_neighbor"] else mut["uniform_count"]
    mean, e_mean = _scale(s, e_s, cnt, dtype, form)
    msq, e_msq = _scale(ss, e_ss, cnt, dtype, form)
    m2 = mean * mean
    e_m2 = 2 * mean.double().abs() * e_mean + U * m2.double()
    var = msq - m2
    e_var = e_msq + e_m2 + U * var.double().abs()
    if fp["relative"]:
        eps = f32(mut["epsilon"]) if mut["epsilon"] is not None else fp["epsilon"]
        d = m2.clamp_min(eps)
        e_d = torch.where(m2.double() + e_m2 >= eps, e_m2, torch.zeros_like(e_m2))
        r = var * (1.0 / d) if form == "rcp" else var / d
        dd = d.double()
        e_var = e_var / dd + var.double().abs() / (dd * dd) * e_d + (1 + RCP_ULPS * 2) * U * r.double().abs()
        var = r
    C = x.shape[3]
    if fp["compress"] and C > 1:
        ch = [var[..., c:c + 1] for c in range(C)]
        acc = _sum(ch)
        e_acc = e_var.sum(dim=3, keepdim=True) + (C - 1) * U * _sum([c.double().abs() for c in ch])
        if mut["compress_sum"]:
            var, e_var = acc, e_acc
        else:
            var, e_var = _scale(acc, e_acc, C, dtype, form)
    elif fp["compress"] and mut["compress_sum"]:
        pass      # one channel: the sum is the mean
    return var, e_var


def pixel_record(v, fp, dtype=F64, form="div", mut=NO_MUTATION):
    """The 3 + nv channels of one pass.  v [B,H,W,cs] float64 holding float32 values, cs in {1, 3}.  -> (value float64, budget)"""
    cs = v.shape[3]
    s, e = standardize(v, fp, dtype)
    rec, erec = (s, e) if cs == 3 else (s.expand(-1, -1, -1, 3), e.expand(-1, -1, -1, 3))
    if mut["swap_ch12"]:
        rec, erec = rec[..., [0, 2, 1]], erec[..., [0, 2, 1]]
    if fp["use_variance"]:
        raw = bool(fp["variance_before"]) != bool(mut["swap_source"])
        src, esrc = (v.to(dtype), torch.zeros_like(e)) if raw else (s, e)
        var, evar = local_variance(src, esrc, fp, dtype, form, mut)
        rec, erec = torch.cat([rec, var], dim=3), torch.cat([erec, evar], dim=3)
    return rec.double(), erec


def n_variance_channels(fp, cs):
    return (1 if fp["compress"] else cs) if fp["use_variance"] else 0


def network_input(entries, B, H, W, c_pad, dtype=F64, form="div", mut=NO_MUTATION):
    """entries: dictionaries with kind 0 (a pass: src [B,H,W,cs], fp), 1 (src [nch], broadcast) or 2 (src [B,H,W,nch], copied), nch and dst_ch;
    nch == 0 entries are skipped.  -> (value [B,H,W,c_pad], budget, records): zeros up to c_pad, records[i] = pixel_record of entry i (or None)."""
    out = torch.zeros(B, H, W, c_pad, dtype=F64)
    err = torch.zeros(B, H, W, c_pad, dtype=F64)
    records = []
    for en in entries:
        records.append(None)
        if en["nch"] <= 0:
            continue
        d = en["dst_ch"]
        if en["kind"] == 0:
            rec, erec = pixel_record(en["src"], en["fp"], dtype, form, mut)
            records[-1] = (rec, erec)
            d += mut["dst_shift"]
            n = min(en["nch"], rec.shape[3], c_pad - d)
            out[..., d:d + n], err[..., d:d + n] = rec[..., :n], erec[..., :n]
        elif en["kind"] == 1:
            out[..., d:d + en["nch"]] = en["src"].view(1, 1, 1, -1)
        else:
            out[..., d:d + en["nch"]] = en["src"]
    return out, err, records


# ---------------------------------------------------------------------------------------------------------------- the gate
STORAGE = {"f32": (torch.float32, None, None), "bf16": (torch.bfloat16, 8, -126), "f16": (torch.float16, 11, -14)}


def storage_rounding(ref, dtype):
    """r_T: half an ulp of the storage type at |ref| (subnormal spacing below the smallest normal); 0 for float32."""
    _, p, emin = STORAGE[dtype]
    if p is None:
        return torch.zeros_like(ref)
    _, ex = torch.frexp(ref.abs())                       # |ref| = m * 2^ex, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(ex, emin), (ex - 1).clamp_min(emin)).double()
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=F64), e - (p - 1))


def to_storage(x, dtype):
    """x rounded to the storage type (as the kernel's store does), back in float64."""
    return x.to(torch.float32).to(STORAGE[dtype][0]).double()


def ratio(got, ref, err, dtype="f32"):
    """|got - ref| / (2 err + r_T) per element; an element with a zero bound must be exact (ratio 0 or inf)."""
    diff = (got.double() - ref).abs()
    bound = 2 * err + storage_rounding(ref, dtype)
    return torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))


def worst_ratio(got, ref, err, dtype="f32"):
    return float(ratio(got, ref, err, dtype).max()) if ref.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- input families
SHAPES = [(1, 1, 1), (2, 1, 5), (1, 2, 2), (1, 16, 16), (1, 15, 31), (2, 17, 33), (3, 24, 40), (1, 5, 50)]
# the standardisation each family runs with (dyadic mean / inv_std for "dyadic"; non-zero mean and variance 4 for "signed"; flat_half sits
# where mean^2 of the standardised plane is below epsilon: log1p(0.5) - 0.4 = 0.0055)
FAMILY_FP = {
    "dyadic": dict(use_log1p=0, mean=0.25, inv_std=0.5),
    "radiance": dict(use_log1p=1, mean=0.7, inv_std=1.0 / 1.3),
    "signed": dict(use_log1p=0, mean=0.3, inv_std=0.5),
    "signed_log1p": dict(use_log1p=1, mean=0.3, inv_std=0.5),
    "flat_one": dict(use_log1p=0, mean=0.25, inv_std=2.0),
    "flat_half": dict(use_log1p=1, mean=0.4, inv_std=1.7),
}
FAMILIES = list(FAMILY_FP)
FLAT = ("flat_one", "flat_half")


def make_values(family, B, H, W, cs, seed):
    """[B,H,W,cs] float64 holding float32-representable values, seeded, built on the CPU."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, H, W, cs)
    if family == "dyadic":
        return torch.randint(-32, 33, shape, generator=g).double() / 16
    if family == "flat_one":
        return torch.full(shape, 1.0, dtype=F64)
    if family == "flat_half":
        return torch.full(shape, 0.5, dtype=F64)
    v = torch.randn(shape, generator=g, dtype=F64)
    if family == "radiance":
        v = v.abs() * torch.exp(torch.randn(shape, generator=g, dtype=F64))
        if H * W >= 16:
            v[:, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 0.0                          # a block of exact zeros
            v[:, H // 4, W // 4], v[:, H // 2, W // 2, 0] = 1e-6, 1e-6                # tiny values inside it
        flat = v.view(-1)
        if flat.numel() >= 4:
            flat[1], flat[flat.numel() - 1] = 1e-6, 1e4
        if flat.numel() >= 64:
            flat[flat.numel() // 3], flat[flat.numel() // 2] = 1e4, 1e-6
    return v.float().double()


def feature_params(family, branch):
    if branch == "identity":
        return params(**IDENTITY)
    return params(**dict(FAMILY_FP[family], **BRANCHES[branch]))


# dd_prepare_feature: every shape x every branch x cs, the family rotating; and every family x every branch at the two-tile ragged shape
def _prepare_cases():
    cases, seen = [], set()

    def add(family, shape, cs, branch):
        key = (family, shape, cs, branch)
        if key not in seen:
            seen.add(key)
            cases.append(dict(family=family, shape=shape, cs=cs, branch=branch, seed=1000 + len(cases),
                              name="%s-%dx%dx%d-cs%d-%s" % ((family,) + shape + (cs, branch))))
    for si, shape in enumerate(SHAPES):
        for bi, branch in enumerate(BRANCHES):
            for cs in (1, 3):
                add(FAMILIES[(si + bi + cs) % len(FAMILIES)], shape, cs, branch)
    for family in FAMILIES:
        for branch in BRANCHES:
            add(family, (2, 17, 33), 3, branch)
            add(family, (1, 5, 50), 1, branch)
    return cases


PREPARE_CASES = _prepare_cases()


@functools.lru_cache(maxsize=None)
def prepare_inputs(i):
    c = PREPARE_CASES[i]
    return make_values(c["family"], *c["shape"], c["cs"], c["seed"]), feature_params(c["family"], c["branch"])


@functools.lru_cache(maxsize=None)
def prepare_reference(i):
    v, fp = prepare_inputs(i)
    return pixel_record(v, fp)


# ---------------------------------------------------------------------------------------------------------------- dd_assemble_input tables
def P(family, cs, branch, std=None):
    """A pass.  std: None, or (ld_std, byte offset of the std_out pointer from a 16-byte boundary)."""
    return dict(kind=0, family=family, cs=cs, branch=branch, std=std)


def V(nch):
    return dict(kind=1, nch=nch)


def K2(nch):
    return dict(kind=2, nch=nch)


SKIP = dict(kind=2, nch=0)
# name -> (entry specs in dst_ch order, c_pad, ld).  Passes with different parameters sit side by side; no relative variance of a raw or
# unscaled signed plane and no absolute variance of raw radiance, which 1e4 would take past the fp16 range.
TABLES = {
    # (a) the usual order: passes of 4 channels, auxiliaries of 4, the embedding row; 23 used of c_pad 24: one padding channel
    "usual": ([P("radiance", 3, "default", (4, 0)), P("signed_log1p", 3, "neighbor_relative_compressed", (4, 4)), P("dyadic", 3, "uniform_absolute", (3, 0)),
               P("radiance", 1, "before_standardization", (8, 0)), P("signed", 1, "uniform_absolute"), V(3)], 24, 32),
    # (b) 3, 4, 6, 4 channels + a plane: both 4-channel passes on an odd dst_ch, a per-channel variance
    "odd": ([P("signed", 3, "no_variance", (4, 0)), P("radiance", 3, "before_standardization", (4, 0)), P("signed_log1p", 3, "uniform_relative_per_channel", (4, 0)),
             P("flat_half", 1, "neighbor_relative_compressed", (3, 4)), K2(2)], 24, 24),
    # (c) one 1-channel pass
    "single": ([P("radiance", 1, "default", (4, 4))], 8, 8),
    # (d) passes only after a vector and a plane, and a skipped entry between them
    "late": ([V(2), K2(3), P("dyadic", 3, "neighbor_absolute_per_channel", (8, 0)), SKIP, P("radiance", 1, "before_standardization_neighbor_per_channel"),
              P("flat_one", 3, "default", (4, 0))], 24, 40),
}
ASSEMBLE_CASES = [(name, T, shape) for name in TABLES for T in (1, 3) for shape in SHAPES]


@functools.lru_cache(maxsize=None)
def assemble_entries(name, T, shape):
    """Per tuple: the entries of network_input() (src values filled in) with the spec's std field kept."""
    specs = TABLES[name][0]
    B, H, W = shape
    tuples = []
    for t in range(T):
        entries, dst = [], 0
        for k, sp in enumerate(specs):
            seed = 5000 + 97 * t + 13 * k + sum(shape) + len(name)
            g = torch.Generator().manual_seed(seed)
            if sp["kind"] == 0:
                fp = feature_params(sp["family"], sp["branch"])
                en = dict(kind=0, src=make_values(sp["family"], B, H, W, sp["cs"], seed), cs=sp["cs"], fp=fp,
                          nch=3 + n_variance_channels(fp, sp["cs"]), dst_ch=dst, std=sp["std"])
            elif sp["kind"] == 1:      # values every storage type holds exactly
                en = dict(kind=1, src=torch.randint(-16, 17, (sp["nch"],), generator=g).double() / 8, nch=sp["nch"], dst_ch=dst, std=None)
            else:
                en = dict(kind=2, src=torch.randint(-16, 17, (B, H, W, sp["nch"]), generator=g).double() / 8, nch=sp["nch"], dst_ch=dst, std=None)
            dst += en["nch"]
            entries.append(en)
        tuples.append(entries)
    return tuples


@functools.lru_cache(maxsize=None)
def assemble_reference(name, T, shape):
    """[(value, budget, records)] per tuple."""
    c_pad = TABLES[name][1]
    return [network_input(entries, *shape, c_pad) for entries in assemble_entries(name, T, shape)]
