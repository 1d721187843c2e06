"""Float64 reference, error budget, mutants and fp32 emulation of ONE scale's fused kernel-prediction head: dd_kpcn_head_fwd, dd_kpcn_head_bwd and
dd_kpcn_head_bwd_multi (csrc/dd_head.hip).  Never touches a GPU.  The helpers of tests/conv_bwd_ref.py (half_ulp, gate_f32, ratio, worst_ratio,
to_storage, representable) are reused, not copied.

THE REFERENCE restates the head as explicit sums in torch float64, no autograd inside, and rounds exactly where the kernel rounds (T = the storage
type, round to nearest even):
    WaT = T(wa), WbT = T(wb)                    (pack8t of the fp32 masters; the biases stay fp32)
    pre = ba + x . WaT        hidT = T(relu(pre))        logT = T(bb + hidT . WbT)        p = softmax(logT) over the K = ks^2 channels
    out_c = sum_t p_t src[sym(y + t / ks - P), sym(x + t % ks - P)][c]
    dp_t = sum_c dout_c src_t,c        dlT = T(p_t (dp_t - sum_u p_u dp_u))        dhT = T(dlT . WbT^T), +0 where hidT is not > 0
    dx = T(dhT . WaT^T), +0 where x is not > 0; with accumulate_dx rounded a second time after the stored gradient is added
    dWb[m][n] += sum_pix hidT_m dlT_n     dbb[n] += sum_pix dlT_n     dWa[c][m] += sum_pix x_c dhT_m     dba[m] += sum_pix dhT_m      (fp32, ADDED)
"x > 0" is "positive as a 16-bit integer" (mask_bf16x2, csrc/dd_common.h): -0 and negative values drop the gradient.

THE BUDGET.  u = 2^-24.  An fp32 sum of n terms is off by at most n u S in ANY order (S = the sum of the terms' magnitudes); as everywhere in
this suite the gate takes twice that.  What is new here is that the reference ROUNDS its intermediates too, as the kernel does.  Two values
within g of each other usually round to the SAME storage value and sometimes to neighbours a whole ulp apart -- so the bound of a rounded
intermediate is not "g plus half an ulp" (that bounds the distance to the UNROUNDED value) but, rounding being monotone,
    flip(v, g) = max(|T(v + g) - T(v)|, |T(v - g) - T(v)|)                      >= |T(v') - T(v)| for every |v' - v| <= g:
zero on all but the few elements that sit within g of a rounding boundary, one ulp there.  It is carried per element through |WbT|, |WaT| and
the pixel sums, so the gates of out, dx and the weight gradients are a few fp32 ulps where nothing can flip (dx: ZERO, the stored bits must
match) and a storage ulp's worth exactly where the kernel may legitimately differ.  No element is left out, nothing is tuned.
  * logits: g = 2 (K + 1) u S (+ flip of hidT through |WbT| where GEMM 1 is not exact); delta = flip(logits, g).
  * softmax: logits off by at most delta move every probability by a factor within [e^-2 delta_max, e^2 delta_max] (rigorous, not first order: numerator
    and denominator each move by at most e^delta_max); plus the fp32 terms -- argument subtraction u |arg|, __expf EXP_REL, the 32-slot sum, the
    reciprocal and the product.
  * out, dp, d logits, d hid, d x: n u S of their own sums plus what their operands may be off, as written next to each line of evaluate().
  * weight and bias gradients: 2 (n_pix + 1) u (S + |what the buffer held|) plus the flips of dlT / dhT (/ hidT) summed over the pixels.

THE INPUTS come in three kinds (the ("int", "real") precedent of pointwise_ref.POOL_KINDS):
  grid        x a multiple of 2^-3 in [0, 4), wa a multiple of 2^-4 s (|wa| <= 15/16 s, s a power of two per C), ba an odd multiple of 2^-8 s: every
              partial sum of GEMM 1 is a multiple of 2^-8 s below 2^17 of them -- exact in fp32 in any order -- and pre is never 0.
  grid-exact  ... and every logit is exactly representable: each column of wb holds at most one non-zero entry, a power of two (then bb = 0), the other
              columns carry a bb on the grid.  Every rounding up to the softmax is exact and the forward gate is the fp32 softmax / apply terms alone.
  real        wa, wb, ba, bb arbitrary fp32, NOT representable (the weight rounding is under test), x representable.  The hidden units with
              |pre| <= 2 n u S (their ReLU could go either way) are returned as `undecided`: the seeds below are chosen so that the set is empty.

EXP_REL, the allowance for __expf, is an ASSUMPTION confirmed by measurement (no accuracy figure of the hardware exponential is on record
here); see the constant.

MUTANTS: plausible mistakes of the kernel, switchable in evaluate(); tests/test_head_ref.py records by which factor each exceeds the gates."""
import functools
import math

import torch

from conv_bwd_ref import F64, STORAGE, U, gate_f32, half_ulp, ratio, representable, to_storage, worst_ratio      # noqa: F401 (re-exported)

F32 = torch.float32
SLOTS = 32               # a pixel's hid / logit row in the kernel: 32 slots, zero beyond K
FLIP_SLACK = 1.0 + 2.0 ** -16      # a legitimate flip is off by the WHOLE bound and the tests ask for error / gate < 1, strictly; zero stays zero


def EXP_REL(arg):
    """Relative error allowed to __expf(arg), arg <= 0: the scaling arg * log2(e) (a rounded product with a rounded constant: 2 u |arg| in the
    result) plus one ulp (2 u) of the exp2 instruction, doubled like every fp32 term here: u (2 |arg| + 4).
    MEASURED on an MI355X through dd_kpcn_fwd against float64 (tests/test_gpu_head_ops.py::test_fast_exponential_stays_within_its_allowance,
    2026-10-20, 23 700 probabilities with arguments down to -18.7): the worst relative error of a whole PROBABILITY -- exponential, sum,
    reciprocal and product together -- was 1.085e-6 = 18.2 u, at argument -12.06, where this allowance alone is 28.1 u; 0.174 of the softmax
    allowance at worst.  The assumption holds, so the constant stays as assumed (it was not derived from the head's output)."""
    return U * (2.0 * arg.abs() + 4.0)


SOFTMAX_F32_TERMS = SLOTS + 3      # in units of u: the sum over 32 slots, the reciprocal, the product p = e * inv, the subtraction (u |arg|, added apart)

MUTANTS = {
    "taps_transposed": ("index", "tap t read at (t % ks, t / ks) instead of (t / ks, t % ks)"),
    "pad_reflect_not_symmetric": ("index", "REFLECT padding (edge sample not repeated) instead of SYMMETRIC"),
    "pad_clamp": ("index", "taps outside the image clamped to the edge"),
    "slot_perm_identity": ("index", "the rows of Wb not permuted with the slot order of hid"),
    "softmax_no_max_shift": ("index", "exp(logit) without subtracting the maximum (fp32 overflow at large logits)"),
    "softmax_over_32": ("index", "the pad channels K..31 (logit 0) inside the softmax sum"),
    "hid_not_rounded": ("rounding", "hid kept in fp32 between the two GEMMs"),
    "logits_not_rounded": ("rounding", "the logits not rounded to the storage type"),
    "weights_truncated": ("rounding", "the fp32 masters truncated (round toward zero) instead of rounded to nearest even"),
    "relu_mask_on_pre_not_hidT": ("index", "d hid masked by pre > 0 instead of by the stored hid > 0"),
    "x_mask_dropped": ("index", "d x not masked by x > 0"),
    "x_mask_ge0": ("index", "d x masked by x >= 0: +0 and -0 keep their gradient"),
    "dlogits_missing_dot": ("index", "d logits = p dp without the - p sum(p dp) term"),
    "dx_overwrites_when_accumulating": ("index", "accumulate_dx ignored: the stored gradient overwritten"),
    "dx_single_rounding_when_accumulating": ("rounding", "the fp32 d x added to the stored gradient and rounded once"),
    "dbb_from_unrounded_dl": ("rounding", "d bb summed from the fp32 d logits instead of the rounded ones"),
    "dba_unmasked": ("index", "d ba summed from d hid before the ReLU mask"),
    "dWa_rows_beyond_C_written": ("index", "rows C .. 32 * NCH - 1 of dWa added to as well"),
    "dW_overwrite_not_add": ("index", "the weight and bias gradients stored instead of added"),
    "last_segment_dropped": ("index", "pixels with x >= 16 (nseg - 1) missing from the weight and bias sums"),
    "image_base_of_first_image": ("index", "the taps of image b read from image 0"),
}
# these change no value on any input the kernel admits, so no gate can see them (tests/test_head_ref.py asserts exactly that):
#   dWa_rows_beyond_C_written  x is zero beyond C in the kernel's fragments, so the extra rows would receive atomicAdd(+0): a guard word keeps its bits;
#   relu_mask_on_pre_not_hidT  differs only where pre > 0 rounds to a stored 0, i.e. below the smallest subnormal of the storage type (fp16: 2^-25).
EQUIVALENT_MUTANTS = ("dWa_rows_beyond_C_written", "relu_mask_on_pre_not_hidT")


# ---------------------------------------------------------------------------------------------------------------- rounding
def _rne(v, dtype):
    return v.to(F32).to(STORAGE[dtype][0]).to(v.dtype)


def _rtz(v, dtype):
    """Round toward zero: the nearest-even value, stepped back by one ulp where it overshot."""
    r = _rne(v, dtype)
    a = r.abs().double()
    pred = a - 2.0 * half_ulp(a * (1.0 - 2.0 ** -13), dtype)      # the storage value just below |r| (the finer spacing below a power of two)
    return torch.where(r.abs() > v.abs(), (torch.sign(r).double() * pred).to(v.dtype), r)


def flip(v, g, dtype, relu=False):
    """max |T(f(v')) - T(f(v))| over |v' - v| <= g, f = relu or the identity: rounding (and relu) are monotone, so the ends of the interval decide."""
    f = torch.relu if relu else (lambda t: t)
    r = to_storage(f(v), dtype)
    return torch.maximum((to_storage(f(v + g), dtype) - r).abs(), (to_storage(f(v - g), dtype) - r).abs()) * FLIP_SLACK


def positive16(x):
    """The kernel's mask: positive as a 16-bit integer -- sign clear and not zero (x holds storage values: NaN cannot occur in the tests' x)."""
    return (x > 0) & ~torch.signbit(x)


# ---------------------------------------------------------------------------------------------------------------- geometry
def slot_ch(q, e):
    return (e >> 2) * 16 + q * 4 + (e & 3)


def _index(i, n, mode):
    if mode == "clamp":
        return i.clamp(0, n - 1)
    if mode == "reflect":
        return torch.where(i < 0, -i, torch.where(i >= n, 2 * n - 2 - i, i)).clamp(0, n - 1)
    return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))      # sym() of dd_head.hip


def gather_taps(src, ks, mut=frozenset()):
    """[N, H, W, K, 3]: the source pixel tap t of every pixel stands for."""
    N, H, W, _ = src.shape
    P = (ks - 1) // 2
    t = torch.arange(ks * ks)
    ty, tx = t // ks, t % ks
    if "taps_transposed" in mut:
        ty, tx = tx, ty
    mode = "reflect" if "pad_reflect_not_symmetric" in mut else "clamp" if "pad_clamp" in mut else "symmetric"
    yy = _index(torch.arange(H)[:, None] + ty[None, :] - P, H, mode)
    xx = _index(torch.arange(W)[:, None] + tx[None, :] - P, W, mode)
    base = src[:1].expand(N, -1, -1, -1) if "image_base_of_first_image" in mut else src
    return base[:, yy[:, None, :], xx[None, :, :], :]


# ---------------------------------------------------------------------------------------------------------------- sums, in float64 or as the fp32 emulation
class Sums:
    """The reductions of the head: plain float64 matmuls, or (emulate=True) fp32 sums over 32-wide channel chunks and 32-pixel steps taken in a
    scrambled order -- what a correct kernel may do."""

    def __init__(self, emulate=False, seed=0):
        self.emulate = emulate
        self.gen = torch.Generator().manual_seed(seed)
        self.acc = F32 if emulate else F64

    def _chunks(self, n):
        order = torch.randperm(-(-n // 32), generator=self.gen).tolist()
        return [(32 * i, min(n, 32 * i + 32)) for i in order]

    def gemm(self, a, w, bias=None):
        """a[..., k] @ w[k, n] (+ bias first, as the kernel's accumulator starts from it)."""
        if not self.emulate:
            r = a @ w
            return r if bias is None else bias + r
        r = torch.zeros(a.shape[:-1] + (w.shape[1],), dtype=F32) if bias is None else bias.expand(a.shape[:-1] + (w.shape[1],)).clone()
        for k0, k1 in self._chunks(a.shape[-1]):
            r = r + a[..., k0:k1] @ w[k0:k1]
        return r

    def over_pixels(self, a, b=None, keep=None):
        """sum over pixels of a[pix, i] * b[pix, j] (b None: of a[pix, i]); keep: 0 / 1 per pixel."""
        a = a.reshape(-1, a.shape[-1])
        b = None if b is None else b.reshape(-1, b.shape[-1])
        if keep is not None:
            a = a * keep.reshape(-1, 1).to(a.dtype)
        if not self.emulate:
            return a.sum(0) if b is None else a.T @ b
        perm = torch.randperm(a.shape[0], generator=self.gen)
        a = a[perm]
        b = None if b is None else b[perm]
        r = None
        for p0, p1 in self._chunks(a.shape[0]):
            part = a[p0:p1].sum(0) if b is None else a[p0:p1].T @ b[p0:p1]
            r = part if r is None else r + part
        return r


# ---------------------------------------------------------------------------------------------------------------- the head
def evaluate(inp, ks, dtype, backward=True, accumulate=False, prefilled=False, mut=frozenset(), rounding=True, budget=True, emulate=False,
             exact1=False, exact2=False, seed=0):
    """One scale's head.  inp: x [N, H, W, C], src / dout [N, H, W, 3], wa [C, K], ba [K], wb [K, K], bb [K], dx_old [N, H, W, C] and the buffers'
    earlier contents w_old = {dwa, dba, dwb, dbb}, all float64.  Returns a dict of values (float64) and, with budget=True (reference only: no
    mutant, no emulation), `gate_<name>` next to every output.  exact1 / exact2: GEMM 1 / GEMM 2 are exact in fp32 by construction of the inputs."""
    mut = frozenset(mut)
    budget = budget and not mut and not emulate and rounding
    sums = Sums(emulate, seed)
    acc = sums.acc
    rnd = (lambda v: _rne(v, dtype)) if rounding else (lambda v: v)
    K = ks * ks
    g = {k: v.to(acc) for k, v in inp.items() if torch.is_tensor(v)}
    x, src = g["x"], g["src"]
    N, H, W, C = x.shape
    npix = N * H * W
    wrnd = (lambda v: _rtz(v, dtype)) if "weights_truncated" in mut else rnd
    WaT, WbT = wrnd(g["wa"]), wrnd(g["wb"])
    out = {}

    # ---- forward
    pre = sums.gemm(x, WaT, g["ba"])
    hid = torch.relu(pre)
    hidT = hid if "hid_not_rounded" in mut else rnd(hid)
    Wb2 = WbT
    if "slot_perm_identity" in mut:      # slot (q, e) holds channel slot_ch(q, e) of hid but is multiplied with row q * 8 + e of Wb
        Wb2 = torch.zeros_like(WbT)
        for q in range(4):
            for e in range(8):
                if (e >> 2) < (K + 15) // 16 and slot_ch(q, e) < K and q * 8 + e < K:
                    Wb2[slot_ch(q, e)] = WbT[q * 8 + e]
    lg = sums.gemm(hidT, Wb2, g["bb"])
    logT = lg if "logits_not_rounded" in mut else rnd(lg)
    if "softmax_no_max_shift" in mut:
        e32 = torch.exp(logT.to(F32))
        p = (e32 / e32.sum(-1, keepdim=True)).to(acc)
    else:
        allv = torch.cat([logT, torch.zeros(logT.shape[:-1] + (SLOTS - K,), dtype=acc)], -1) if "softmax_over_32" in mut else logT
        arg = allv - allv.max(-1, keepdim=True).values
        ex = torch.exp(arg)
        p = (ex / ex.sum(-1, keepdim=True))[..., :K]
        arg = arg[..., :K]
    tp = gather_taps(src, ks, mut)                               # [N, H, W, K, 3]
    out["out"] = (p[..., None] * tp).sum(-2)
    out.update(pre=pre, hidT=hidT, logT=logT, p=p)

    if budget:
        S_pre = g["ba"].abs() + x.abs() @ WaT.abs()
        e_pre = torch.zeros_like(pre) if exact1 else 2 * (C + 1) * U * S_pre
        # undecided: the ReLU (or the stored hid > 0 the backward masks by) could go either way within the budget of pre
        out["undecided"] = int(((pre.abs() <= e_pre) | ((pre > 0) & ~(hidT > 0))).sum())
        d_hid = torch.zeros_like(pre) if exact1 else flip(pre, e_pre, dtype, relu=True)
        S_lg = g["bb"].abs() + hidT @ WbT.abs()
        g_lg = torch.zeros_like(lg) if (exact1 and exact2) else 2 * (K + 1) * U * S_lg + d_hid @ WbT.abs()
        d_log = flip(lg, g_lg, dtype)
        dmax = d_log.max(-1, keepdim=True).values
        er = EXP_REL(arg)
        rel32 = er + er.max(-1, keepdim=True).values + U * arg.abs() + SOFTMAX_F32_TERMS * U
        g_p = p * (torch.expm1(2 * dmax) + 2 * rel32)
        out["gate_out"] = 2 * SLOTS * U * (p[..., None] * tp.abs()).sum(-2) + (g_p[..., None] * tp.abs()).sum(-2)
        out["gate_p"] = g_p
        out["spread"] = float((logT.max(-1).values - logT.min(-1).values).median())
    if not backward:
        return out

    # ---- backward
    dout = g["dout"]
    dp = (dout[..., None, :] * tp).sum(-1)                       # [N, H, W, K]
    dot = (p * dp).sum(-1, keepdim=True)
    a = dp if "dlogits_missing_dot" in mut else dp - dot
    dl = p * a
    dlT = rnd(dl)
    dh = sums.gemm(dlT, WbT.T)
    hmask = (pre > 0) if "relu_mask_on_pre_not_hidT" in mut else (hidT > 0)
    dhT_all = rnd(dh)
    dhT = torch.where(hmask, dhT_all, torch.zeros_like(dh))
    dxp = sums.gemm(dhT, WaT.T)
    xmask = torch.ones_like(x, dtype=torch.bool) if "x_mask_dropped" in mut else (x >= 0) if "x_mask_ge0" in mut else positive16(x)
    dx1 = torch.where(xmask, rnd(dxp), torch.zeros_like(dxp))
    if accumulate and "dx_overwrites_when_accumulating" not in mut:
        if "dx_single_rounding_when_accumulating" in mut:
            dx = rnd(torch.where(xmask, dxp, torch.zeros_like(dxp)) + g["dx_old"])
        else:
            dx = rnd(dx1 + g["dx_old"])
    else:
        dx = dx1
    out["dx"] = dx
    keep = None
    if "last_segment_dropped" in mut:
        keep = (torch.arange(W) < 16 * ((W + 15) // 16 - 1)).to(acc).expand(N, H, W)
    grads = {"dwb": sums.over_pixels(hidT, dlT, keep), "dbb": sums.over_pixels(dl if "dbb_from_unrounded_dl" in mut else dlT, None, keep),
             "dwa": sums.over_pixels(x, dhT, keep), "dba": sums.over_pixels(dhT_all if "dba_unmasked" in mut else dhT, None, keep)}
    for name, v in grads.items():
        old = g["w_old_" + name] if prefilled else None
        out[name] = v if old is None or "dW_overwrite_not_add" in mut else old + v
    out.update(dlT=dlT, dhT=dhT)

    if budget:
        e_dp = 2 * 3 * U * (dout.abs()[..., None, :] * tp.abs()).sum(-1)
        e_dot = (g_p * dp.abs()).sum(-1, keepdim=True) + ((p + g_p) * e_dp).sum(-1, keepdim=True) + 2 * SLOTS * U * (p * dp.abs()).sum(-1, keepdim=True)
        e_a = e_dp + e_dot
        e_a = e_a + 2 * U * (a.abs() + e_a)
        g_dl = g_p * (a.abs() + e_a) + p * e_a + 2 * U * dl.abs()
        d_dl = flip(dl, g_dl, dtype)
        g_dh = 2 * K * U * (dlT.abs() @ WbT.abs().T) + d_dl @ WbT.abs().T
        d_dh = torch.where(hmask, flip(dh, g_dh, dtype), torch.zeros_like(dh))
        g_dx = 2 * K * U * (dhT.abs() @ WaT.abs().T) + d_dh @ WaT.abs().T
        d_dx = torch.where(xmask, flip(dxp, g_dx, dtype), torch.zeros_like(dxp))
        if accumulate:      # the fp32 sum of two storage values (rounded: u |sum|), then the second rounding
            s = dx1 + g["dx_old"]
            d_dx = flip(s, d_dx + 2 * U * s.abs(), dtype)
        out["gate_dx"] = d_dx
        flat = lambda t: t.reshape(npix, -1)      # noqa: E731
        S = {"dwb": flat(hidT).T @ flat(dlT).abs(), "dbb": flat(dlT).abs().sum(0), "dwa": flat(x).abs().T @ flat(dhT).abs(), "dba": flat(dhT).abs().sum(0)}
        extra = {"dwb": flat(d_hid).T @ (flat(dlT).abs() + flat(d_dl)) + flat(hidT).T @ flat(d_dl), "dbb": flat(d_dl).sum(0),
                 "dwa": flat(x).abs().T @ flat(d_dh), "dba": flat(d_dh).sum(0)}
        for name in grads:
            old = g["w_old_" + name].abs() if prefilled else 0.0
            out["gate_" + name] = gate_f32((npix + 1) * U * (S[name] + old)) + extra[name]
        out["flips"] = {"logT": int((d_log > 0).sum()), "dlT": int((d_dl > 0).sum()), "dhT": int((d_dh > 0).sum()), "dx": int((d_dx > 0).sum())}
    return out


OUTPUTS_FWD = ("out",)
OUTPUTS_BWD = ("dx", "dwa", "dba", "dwb", "dbb")


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU tests
# (ks, C, N, H, W, flag)      flag "neg": x with -0 and negative entries in two channels; "big": logits near 96 (grid-exact kind only)
CASES = [
    (5, 8, 1, 2, 2, ""),             # one ragged segment, both pads at their limit (H = W = P)
    (3, 8, 2, 1, 1, ""),             # the same for the 3 x 3 head (NT = 1)
    (5, 32, 2, 3, 15, ""), (5, 32, 2, 3, 16, ""), (5, 32, 2, 3, 17, ""),      # W below, at and above one segment
    (3, 24, 1, 5, 33, ""),           # two segments and a ragged one: an odd segment count (the even-step rounding of a wave's range)
    (5, 24, 2, 6, 18, ""), (5, 40, 2, 6, 18, ""), (5, 72, 2, 6, 18, ""), (5, 104, 2, 6, 18, ""),      # ragged channel chunks, one per NCH
    (5, 32, 1, 8, 20, ""), (5, 64, 1, 8, 20, ""), (5, 96, 1, 8, 20, ""), (5, 128, 1, 8, 20, ""),      # full chunks
    (3, 32, 1, 8, 20, ""), (3, 64, 1, 8, 20, ""), (3, 96, 1, 8, 20, ""), (3, 128, 1, 8, 20, ""),
    (5, 64, 3, 20, 18, ""),          # several workgroups flush; the image base of b > 0
    (5, 40, 1, 6, 18, "neg"),        # x with -0 and negative entries
    (3, 8, 1, 2, 2, "big"),          # logits 96 .. 100: exp() without the maximum shift overflows fp32
]
EXACT_CASES = CASES[:6] + [CASES[18], CASES[20]]      # the rows that also run the grid-exact kind
KINDS = ("grid", "real")
DTYPES = ("bf16", "f16")
# problems of the dd_kpcn_head_bwd_multi launches (rows of CASES with one kernel size); the second problem of each accumulates into dx
MULTI = [(CASES[0], CASES[18]), (CASES[0], CASES[18], CASES[7]), (CASES[1], CASES[5]), (CASES[1], CASES[5], CASES[16])]
# salt of the generator per (case, dtype, kind) where it is not 0: the first salt at which the undecided set is empty and the median logit spread
# lies in [2, 8] (tests/test_head_ref.py asserts both for every entry of the table)
SALT = {("ks3-C8-2x1x1", "f16", "grid"): 2, ("ks3-C8-2x1x1", "f16", "real"): 1}      # (two pixels each: their median spread fell below 2)


def case_id(case):
    return "ks%d-C%d-%dx%dx%d%s" % (case[:5] + (("-" + case[5]) if case[5] else "",))


def kinds_of(case):
    if case[5] == "big":
        return ("grid-exact",)
    return KINDS + (("grid-exact",) if case in EXACT_CASES else ())


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _randint(lo, hi, shape, gen):
    return torch.randint(lo, hi, shape, generator=gen).to(F64)


@functools.lru_cache(maxsize=None)
def head_inputs(case, dtype, kind):
    ks, C, N, H, W, flag = case
    K = ks * ks
    salt = SALT.get((case_id(case), dtype, kind), 0)
    gen = _gen(ks, C, N, H, W, len(flag), DTYPES.index(dtype), ("grid", "real", "grid-exact").index(kind), salt)
    inp = {}
    if kind == "real":
        x = torch.randn(N, H, W, C, generator=gen, dtype=F64) * 1.5
        inp["x"] = representable(torch.where(torch.rand(N, H, W, C, generator=gen, dtype=F64) < 0.4, torch.zeros_like(x), x.abs()), dtype)
        inp["wa"] = (torch.randn(C, K, generator=gen, dtype=F64) / math.sqrt(C)).float().double()
        inp["ba"] = (0.3 * torch.randn(K, generator=gen, dtype=F64)).float().double()
        inp["wb"] = (torch.randn(K, K, generator=gen, dtype=F64) * (0.3 if ks == 5 else 0.6)).float().double()
        inp["bb"] = (0.5 * torch.randn(K, generator=gen, dtype=F64)).float().double()
    else:
        s = 2.0 ** -round(0.5 * math.log2(C))
        inp["x"] = _randint(-12, 32, (N, H, W, C), gen).clamp_min(0) / 8
        inp["wa"] = _randint(-15, 16, (C, K), gen) / 16 * s
        inp["ba"] = (2 * _randint(-64, 64, (K,), gen) + 1) / 256 * s
        if kind == "grid":
            inp["wb"] = _randint(-15, 16, (K, K), gen) / 16 * (0.5 if ks == 5 else 1.0)
            inp["bb"] = _randint(-8, 9, (K,), gen) / 8
        elif flag == "big":
            inp["wb"] = torch.zeros(K, K, dtype=F64)
            inp["bb"] = 96 + 0.5 * torch.arange(K, dtype=F64)[torch.randperm(K, generator=gen)]
        else:      # even columns: one power-of-two entry and no bias; odd columns: a bias on the grid and no weight
            wb, bb = torch.zeros(K, K, dtype=F64), torch.zeros(K, dtype=F64)
            rows = torch.randperm(K, generator=gen)
            for n in range(K):
                if n % 2 == 0:
                    wb[rows[n], n] = 2.0
                else:
                    bb[n] = float(torch.randint(-8, 9, (1,), generator=gen)) / 4
            inp["wb"], inp["bb"] = wb, bb
    if flag == "neg":      # channels 1 and 5: negative values and -0 (the sign survives the storage type)
        v = inp["x"][..., [1, 5]]
        r = torch.rand(v.shape, generator=gen, dtype=F64)
        inp["x"][..., [1, 5]] = representable(torch.where(r < 0.3, -torch.zeros_like(v), torch.where(r < 0.6, -(v + 0.125), v)), dtype)
    inp["src"] = torch.randn(N, H, W, 3, generator=gen, dtype=F64).float().double()
    inp["dout"] = torch.randn(N, H, W, 3, generator=gen, dtype=F64).float().double()
    inp["dx_old"] = representable(torch.randn(N, H, W, C, generator=gen, dtype=F64), dtype)
    for name, shape in (("dwa", (C, K)), ("dba", (K,)), ("dwb", (K, K)), ("dbb", (K,))):      # a known fp32 pattern at the gradients' own scale
        inp["w_old_" + name] = _randint(-128, 129, shape, gen) / 64
    for k in ("x", "wa", "wb", "ba", "bb"):
        assert bool((inp[k].float().double() == inp[k]).all())
    return inp


def is_exact(kind):
    """(GEMM 1 exact, GEMM 2 exact) by construction of the kind."""
    return kind != "real", kind == "grid-exact"


@functools.lru_cache(maxsize=None)
def head_reference(case, dtype, kind, accumulate=False, prefilled=False, backward=True):
    e1, e2 = is_exact(kind)
    return evaluate(head_inputs(case, dtype, kind), case[0], dtype, backward=backward, accumulate=accumulate, prefilled=prefilled, exact1=e1, exact2=e2)
