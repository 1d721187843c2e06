"""Float64 reference, error budget, mutants and fp32 emulation of the LAYER-WISE kernel-prediction launches dd_kpcn_fwd, dd_kpcn_bwd,
dd_kpcn_hidden_fwd and dd_kpcn_hidden_bwd (kpcn_fwd_kernel / kpcn_bwd_kernel of csrc/dd_pointwise.hip with their VEC and HID variants).  Never
touches a GPU.  gather_taps, _index, EXP_REL, flip and the rounding helpers come from tests/head_ref.py, the gates' helpers from
tests/conv_bwd_ref.py: nothing is copied.

THE REFERENCE restates the launches as explicit sums in torch float64, no autograd inside, and rounds exactly where the kernel rounds
(T = the storage type; for f32 storage T is fp32 and nothing is rounded below fp32).  K = ks^2, P = (ks - 1) / 2, member j of a tuple of M:
    stored logits   logit_t = row[j K + t], the T values as they are
    HID             logit_t = bb[t] + sum_{k < kh} hid_k wb[k ldw + t]        from the fp32 masters, NOT rounded to T
    forward         p = softmax(logit) with max shift          out_c = sum_t p_t src[sym(y + t / ks - P), sym(x + t % ks - P)][c]       (fp32)
    backward        dp_t = sum_c dout_c src_t,c                dl_t = T(p_t (dp_t - sum_u p_u dp_u))
                    channels K .. dl_pad - 1 of the member's d logits are written +0, everything beyond dl_pad and before the member is untouched
The d logits are returned as the WHOLE row of lddl channels after the call, so "untouched" and "+0" are gated like every value (gate 0: exact).

THE BUDGET, per element.  u = 2^-24.  An fp32 sum of n terms is off by at most n u S in ANY order, fused or not (S = the sum of the terms'
magnitudes); the gate takes 2 n u S as everywhere in this suite.
  * HID logits: kh fused multiply-adds behind the bias: delta_t = 2 (kh + 1) u S_t, S_t = |bb_t| + sum_k |hid_k| |wb_kt|.  Stored logits: delta = 0.
  * softmax: logits off by at most delta_max move every probability by a factor within [e^-2 delta_max, e^2 delta_max] (rigorous: numerator and
    denominator each move by at most e^delta_max; the max shift cancels).  The fp32 terms, relative to p_t and in units of u: the subtraction
    logit - max (|arg|), __expf of the numerator and of the largest term of the denominator (head_ref.EXP_REL each), the sum of K positive terms
    (K -- not the fused head's 32 slots), the reciprocal (2: one ulp, the hardware reciprocal) and the product e_t * inv (1):
        rel32_t = EXP_REL(arg_t) + max_u EXP_REL(arg_u) + u |arg_t| + (K + 3) u            g_p = p (expm1(2 delta_max) + 2 rel32).
    EXP_REL was measured for arguments down to -18.7 only: evaluate() ASSERTS arg >= -18 on every input it budgets.
  * out_c: K products and additions: 2 K u sum_t p_t |src_t,c|, plus sum_t g_p,t |src_t,c|.
  * dp_t: 3 terms: e_dp = 6 u sum_c |dout_c| |src_t,c|.     dot = sum_u p_u dp_u: e_dot = sum g_p |dp| + sum (p + g_p) e_dp + 2 K u sum p |dp|.
    a_t = dp_t - dot: e_a = e_dp + e_dot, + 2 u (|a| + e_a) for the subtraction.     dl_t = p_t a_t: g_dl = g_p (|a| + e_a) + p e_a + 2 u |dl|.
  * the stored d logits: f32 storage -- the plain fp32 budget g_dl.  bf16 / f16 -- head_ref.flip(dl, g_dl, T): ZERO wherever no fp32 error within
    g_dl can move the rounding (the stored bits must be the reference's), one storage ulp where it can.
Nothing is tuned against the kernel.

THE DISPATCH RULE of kpcn_dispatch is restated in dispatch(): which of the four template routes (VEC, HID) a call takes follows from the byte
alignment of the logit / d logit pointers and the row lengths; tests/test_gpu_kpcn_ops.py asserts the route of every problem from it.

THE INPUTS come in three kinds:
  real    arbitrary representable logits in [-7, 8] (HID: representable post-ReLU hid, fp32 wb / bb that are NOT representable in T); the median
          logit spread of a case is at least 2.
  offset  the same logits, quantised so that the sum stays exactly representable in T, plus a common offset that needs the max shift: 96 (bf16, f32,
          and every HID case, whose logits are fp32) or 24 (f16 stored logits).  With 96, exp(logit) overflows fp32 in every pixel (asserted).
  flat    all K logits of a pixel equal (HID: wb = 0 and one bias): p = 1 / K.
The fourth channel of src / dout, the pad channels of hid and of the logit row, and wb / bb outside the member window hold finite DECOYS here (a
mutant that reads them changes a value); the GPU tests put NaN there.

MUTANTS: plausible mistakes of the kernels, switchable in evaluate(); tests/test_kpcn_ref.py records by which factor each exceeds the gates.
THE FP32 EMULATION (order = "forward" | "reverse" | "pairwise" | "fma_free") evaluates the same formulas in torch float32: fused multiply-adds
taken front to back or back to front, a pairwise tree over rounded products, or sequential without fusing."""
import collections
import functools

import torch

from conv_bwd_ref import F64, U, ratio, worst_ratio      # noqa: F401 (re-exported)
from head_ref import EXP_REL, _index, _rne, _rtz, flip, gather_taps      # noqa: F401 (re-exported)

F32 = torch.float32
SENTINEL = 12288.0      # what the d logits rows hold before a call: exact in fp32, bf16 and fp16 (conv_ops_util.SENTINEL)
DTYPES = ("f32", "bf16", "f16")
KINDS = ("real", "offset", "flat")
ORDERS = ("forward", "reverse", "pairwise", "fma_free")
ROUTES = ("vec", "scalar", "hid_vec", "hid_scalar")
ARG_MIN = -18.0
WB_C0 = 3               # first column of the tuple's window inside the wider wb matrix / bb vector
WB_GUARD_ROWS = 8       # rows kh .. kh + 7 of the wb buffer: never read by a correct kernel

MUTANTS = {
    "taps_transposed": "tap t read at (t % ks, t / ks) instead of (t / ks, t % ks)",
    "pad_reflect_not_symmetric": "REFLECT padding (edge sample not repeated) instead of SYMMETRIC",
    "pad_clamp": "taps outside the image clamped to the edge",
    "softmax_no_max_shift": "exp(logit) without subtracting the maximum (fp32 overflow at large logits)",
    "softmax_over_k2p": "the pad channels K .. K2P - 1 of the 16-byte vectors inside the softmax",
    "image_base_of_first_image": "the taps of image b read from image 0",
    "dlogits_missing_dot": "d logits = p dp without the - p sum(p dp) term",
    "dot_unnormalised": "sum(e dp) taken over the exponentials before they are divided by their sum",
    "pad_channels_unwritten": "channels K .. dl_pad - 1 of the member's d logits left as they were",
    "beyond_dl_pad_zeroed": "channels beyond dl_pad zeroed (the whole rest of the row)",
    "member_offset_ignored_logits": "member j's logits read from channel 0 instead of j K",
    "member_offset_ignored_wb": "member j's wb / bb columns read from the window's first column instead of j K",
    "member_offset_ignored_store": "member j's d logits stored at channel 0 instead of j K",
    "ldw_as_kh": "row k of wb taken at k * kh instead of k * ldw",
    "hid_pad_channel_used": "the pad channels kh .. of the last 16-byte vector of hid multiplied in",
    "src_fourth_channel_used": "channel 3 of a src row read in place of channel 2",
    "dout_fourth_channel_used": "channel 3 of a dout row read in place of channel 2",
    "dlogits_truncated": "d logits rounded toward zero instead of to nearest even",
    "hid_logits_rounded": "the HID logits rounded to the storage type",
}
# mutants that change no value on any input the kernels admit (tests/test_kpcn_ref.py asserts exactly that; at most two may stand here)
EQUIVALENT_MUTANTS = ()

Case = collections.namedtuple("Case", "route ks B H W M j")
Layout = collections.namedtuple("Layout", "N K K2P hid off ldl lddl dl_pad kh ldh ldw rows_w")


def per16(dtype):
    return 4 if dtype == "f32" else 8


def _up(a, b):
    return (a + b - 1) // b * b


def esize(dtype):
    return 4 if dtype == "f32" else 2


def layout(case, dtype):
    """Row lengths and offsets (in elements) of a problem.  Stored logits: member j at channel j K of a row of ldl; VEC problems have one member,
    the scalar ones several.  The d logits row is one vector longer than what the last member pads to, so there are channels beyond dl_pad."""
    N, K = per16(dtype), case.ks * case.ks
    K2P, hid, M, j = _up(K, N), case.route.startswith("hid"), case.M, case.j
    cp = _up(M * K, N)
    if case.route in ("vec", "hid_vec"):
        assert M == 1 and j == 0
        ldl, lddl, dl_pad = K2P + N, K2P + 2 * N, K2P + N          # (dl_pad > K2P: the zero vectors behind the value vectors)
    else:
        assert M > 1 and j > 0
        ldl, lddl, dl_pad = cp + N, cp + N, (K if j < M - 1 else cp - j * K)      # dl_pad as prediction_head.py passes it
    kh = (K + 2 if case.route == "hid_vec" else M * K) if hid else 0
    ldh = _up(kh, N) + N if hid else 0
    ldw = max(M * K, kh) + 8 if hid else 0
    return Layout(N, K, K2P, hid, j * K, ldl, lddl, dl_pad, kh, ldh, ldw, kh + WB_GUARD_ROWS)


def dispatch(dtype, ks, fwd, hid, logits_byte_off, ldl, dl_byte_off=0, lddl=0, dl_pad=0):
    """(VEC, HID) of kpcn_dispatch (csrc/dd_pointwise.hip) for buffers that are themselves 16-byte aligned: the byte offsets are the member's."""
    n = per16(dtype)
    k2p = _up(ks * ks, n)
    vec = True if hid else (logits_byte_off % 16 == 0 and ldl % n == 0 and ldl >= k2p)
    if not fwd:
        vec = dl_byte_off % 16 == 0 and lddl % n == 0 and dl_pad % n == 0 and dl_pad >= k2p and vec
    return vec, bool(hid)


def route_of(case, dtype, fwd):
    lay = layout(case, dtype)
    return dispatch(dtype, case.ks, fwd, lay.hid, 0 if lay.hid else lay.off * esize(dtype), lay.ldh if lay.hid else lay.ldl,
                    lay.off * esize(dtype), lay.lddl, lay.dl_pad)


EXPECTED_ROUTE = {      # route -> ((VEC, HID) forward, (VEC, HID) backward)
    "vec": ((True, False), (True, False)), "scalar": ((False, False), (False, False)),
    "hid_vec": ((True, True), (True, True)), "hid_scalar": ((True, True), (False, True)),
}


# ---------------------------------------------------------------------------------------------------------------- rounding
def store(v, dtype):
    """v rounded to the storage type (nearest even), in float64."""
    return v.to(F32).to(F64) if dtype == "f32" else _rne(v.to(F64), dtype)


def store_rtz(v, dtype):
    v = v.to(F64)
    if dtype != "f32":
        return _rtz(v, dtype)
    r = v.to(F32)
    return torch.where(r.double().abs() > v.abs(), torch.nextafter(r, torch.zeros_like(r)), r).to(F64)


def representable(v, dtype):
    return store(v, dtype)


# ---------------------------------------------------------------------------------------------------------------- sums
def accumulate(n, term, init, order):
    """init + sum_{i < n} a_i b_i with (a_i, b_i) = term(i).  order None: float64.  Otherwise float32 in one of ORDERS."""
    if order is None:
        acc = init
        for i in range(n):
            a, b = term(i)
            acc = acc + a * b
        return acc
    if order in ("forward", "reverse"):      # fused multiply-add: the product is exact in float64, one rounding per step
        acc = init
        for i in (range(n) if order == "forward" else reversed(range(n))):
            a, b = term(i)
            acc = (acc.double() + a.double() * b.double()).to(F32)
        return acc
    if order == "fma_free":
        acc = init
        for i in range(n):
            a, b = term(i)
            acc = acc + a * b
        return acc
    assert order == "pairwise"
    parts = [a * b for a, b in (term(i) for i in range(n))]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0] + init


# ---------------------------------------------------------------------------------------------------------------- the launches
def evaluate(inp, case, dtype, backward=True, mut=frozenset(), rounding=True, budget=True, order=None):
    """One member's launch(es).  inp: src / dout [B, H, W, 4], and lg [B, H, W, ldl] (stored logits) or hid [B, H, W, ldh], wb [kh + 8, ldw],
    bb [ldw]; dl_old [B, H, W, lddl].  Returns out [B, H, W, 3], dl_row [B, H, W, lddl] (the row AFTER the call) and, with budget=True (reference
    only), gate_out and gate_dl_row."""
    mut = frozenset(mut)
    assert mut <= set(MUTANTS)
    budget = budget and not mut and order is None and rounding
    acc = F32 if order else F64
    lay = layout(case, dtype)
    ks, K, j = case.ks, lay.K, case.j
    g = {k: v.to(acc) for k, v in inp.items() if torch.is_tensor(v)}
    src = g["src"][..., [0, 1, 3]] if "src_fourth_channel_used" in mut else g["src"][..., :3]
    dout = g["dout"][..., [0, 1, 3]] if "dout_fourth_channel_used" in mut else g["dout"][..., :3]
    zero = torch.zeros((), dtype=acc)
    res = {}

    # ---- logits
    if lay.hid:
        hid, wbw, bbw = g["hid"], g["wb"], g["bb"]
        col = WB_C0 + (0 if "member_offset_ignored_wb" in mut else lay.off)
        kk = _up(lay.kh, lay.N) if "hid_pad_channel_used" in mut else lay.kh
        if "ldw_as_kh" in mut:
            flat = wbw.reshape(-1)
            Wm = flat[col + torch.arange(kk)[:, None] * lay.kh + torch.arange(K)[None, :]]
        else:
            Wm = wbw[:kk, col:col + K]
        bias = bbw[col:col + K]
        lg = accumulate(kk, lambda k: (hid[..., k:k + 1], Wm[k]), bias.expand(hid.shape[:-1] + (K,)), order)
        if "hid_logits_rounded" in mut:
            lg = store(lg, dtype).to(acc)
        pads = torch.zeros(lg.shape[:-1] + (lay.K2P - K,), dtype=acc)
    else:
        off = 0 if "member_offset_ignored_logits" in mut else lay.off
        lg = g["lg"][..., off:off + K]
        pads = g["lg"][..., off + K:off + lay.K2P]

    # ---- softmax
    if "softmax_no_max_shift" in mut:
        e32 = torch.exp(lg.to(F32))
        ex, arg = e32.to(acc), lg
        inv = (1.0 / e32.sum(-1, keepdim=True)).to(acc)
    else:
        allv = torch.cat([lg, pads], -1) if "softmax_over_k2p" in mut else lg
        arg = allv - allv.max(-1, keepdim=True).values
        ex = torch.exp(arg)
        inv = 1.0 / accumulate(allv.shape[-1], lambda t: (ex[..., t], zero + 1.0), zero, order)[..., None]
        ex, arg = ex[..., :K], arg[..., :K]
    p = ex * inv
    tp = gather_taps(src, ks, mut)                                   # [B, H, W, K, 3]
    res["out"] = accumulate(K, lambda t: (p[..., t:t + 1], tp[..., t, :]), zero, order)
    res["p"], res["logits"] = p, lg

    if budget:
        assert float(arg.min()) >= ARG_MIN, "exponential argument %.2f below %.0f: EXP_REL is not measured there" % (float(arg.min()), ARG_MIN)
        if lay.hid:
            S_lg = bias.abs() + hid[..., :lay.kh].abs() @ Wm.abs()
            dmax = (2 * (lay.kh + 1) * U * S_lg).max(-1, keepdim=True).values
        else:
            dmax = torch.zeros_like(lg[..., :1])
        er = EXP_REL(arg)
        rel32 = er + er.max(-1, keepdim=True).values + U * arg.abs() + (K + 3) * U
        g_p = p * (torch.expm1(2 * dmax) + 2 * rel32)
        res["gate_out"] = 2 * K * U * (p[..., None] * tp.abs()).sum(-2) + (g_p[..., None] * tp.abs()).sum(-2)
        res["gate_p"] = g_p
        res["spread"] = float((lg.max(-1).values - lg.min(-1).values).median())
        res["arg_min"] = float(arg.min())
    if not backward:
        return res

    # ---- backward
    dp = accumulate(3, lambda c: (dout[..., None, c], tp[..., c]), zero, order)              # [B, H, W, K]
    wdot = ex if "dot_unnormalised" in mut else p
    dot = accumulate(K, lambda t: (wdot[..., t], dp[..., t]), zero, order)[..., None]
    a = dp if "dlogits_missing_dot" in mut else dp - dot
    dl = p * a
    if not rounding or (dtype == "f32" and order is None):
        dlT = dl.to(F64)
    elif "dlogits_truncated" in mut:
        dlT = store_rtz(dl, dtype)
    else:
        dlT = store(dl, dtype)
    row = inp["dl_old"].to(F64).clone()
    off = 0 if "member_offset_ignored_store" in mut else lay.off
    row[..., off:off + K] = dlT
    if "pad_channels_unwritten" not in mut:
        row[..., off + K:off + lay.dl_pad] = 0.0
    if "beyond_dl_pad_zeroed" in mut:
        row[..., off + lay.dl_pad:] = 0.0
    res["dl_row"], res["dl"] = row, dl

    if budget:
        e_dp = 2 * 3 * U * (dout.abs()[..., None, :] * tp.abs()).sum(-1)
        e_dot = (g_p * dp.abs()).sum(-1, keepdim=True) + ((p + g_p) * e_dp).sum(-1, keepdim=True) + 2 * K * U * (p * dp.abs()).sum(-1, keepdim=True)
        e_a = e_dp + e_dot
        e_a = e_a + 2 * U * (a.abs() + e_a)
        g_dl = g_p * (a.abs() + e_a) + p * e_a + 2 * U * dl.abs()
        gate = torch.zeros_like(row)
        gate[..., lay.off:lay.off + K] = g_dl if dtype == "f32" else flip(dl, g_dl, dtype)
        res["gate_dl_row"] = gate
        res["flips"] = int((gate > 0).sum()) if dtype != "f32" else 0
    return res


# ---------------------------------------------------------------------------------------------------------------- the cases
def shapes(ks):
    """(B, H, W): both axes at the pad limit P; the fewest rows / columns the pad admits (a single row / column for ks 3) next to a longer axis;
    three images; more than one block of 128 pixels, not a multiple of it; 960 pixels."""
    P = (ks - 1) // 2
    return [(1, P, P), (1, P, 7), (1, 7, P), (3, 5, 7), (2, 9, 11), (1, 24, 40)]


MEMBERS = {"vec": {3: [(1, 0)], 5: [(1, 0)], 7: [(1, 0)]}, "scalar": {3: [(3, 1), (3, 2)], 5: [(2, 1)], 7: [(2, 1)]}}
MEMBERS["hid_vec"], MEMBERS["hid_scalar"] = MEMBERS["vec"], MEMBERS["scalar"]


def cases(route, ks):
    return [Case(route, ks, B, H, W, M, j) for (M, j) in MEMBERS[route][ks] for (B, H, W) in shapes(ks)]


ALL_CASES = [c for route in ROUTES for ks in (3, 5, 7) for c in cases(route, ks)]


def case_id(case):
    return "%s-ks%d-%dx%dx%d-M%dj%d" % case


def offset_of(case, dtype):
    return 24.0 if (dtype == "f16" and not case.route.startswith("hid")) else 96.0


def offset_grid(dtype):
    """Spacing of the storage type over the whole range offset + [-7, 8]: bf16 [64, 128): 2^-1; f16 [16, 32]: 2^-6; f32: far finer than 2^-10."""
    return {"bf16": 0.5, "f16": 2.0 ** -6, "f32": 2.0 ** -10}[dtype]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def generate(case, dtype, kind):
    ks, B, H, W = case.ks, case.B, case.H, case.W
    P = (ks - 1) // 2
    if H < P or W < P:
        raise ValueError("image smaller than the symmetric pad")
    lay = layout(case, dtype)
    gen = _gen(ROUTES.index(case.route), ks, B, H, W, case.M, case.j, DTYPES.index(dtype))      # (the kinds share their random draws)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)      # noqa: E731
    inp = {}
    for name in ("src", "dout"):
        v = rn(B, H, W, 4).float().double()
        v[..., 3] = (64.0 + v[..., 3]).float().double()              # decoy
        inp[name] = v
    if lay.hid:
        hid = representable(torch.relu(rn(B, H, W, lay.ldh)), dtype)
        hid[..., lay.kh:] = 3.0                                      # decoy
        wb = (rn(lay.rows_w, lay.ldw) * 1.2 / (0.5 * lay.kh) ** 0.5).float().double()
        bb = (0.5 * rn(lay.ldw)).float().double()
        if kind == "offset":
            bb = (bb + offset_of(case, dtype)).float().double()
        elif kind == "flat":
            wb[:, WB_C0:WB_C0 + case.M * lay.K] = 0.0
            bb[WB_C0:WB_C0 + case.M * lay.K] = 0.75
        inp.update(hid=hid, wb=wb, bb=bb)
    else:
        base = (rn(B, H, W, lay.ldl) * 1.5).clamp(-7.0, 8.0)
        if kind == "real":
            lg = representable(base, dtype)
        elif kind == "offset":
            q = offset_grid(dtype)
            lg = torch.round(base / q) * q + offset_of(case, dtype)
        else:
            lg = representable(rn(B, H, W, 1) * 2.0, dtype).expand(B, H, W, lay.ldl).clone()
        lg[..., case.M * lay.K:] = 0.0                               # decoy: the pad channels of the row
        inp["lg"] = lg
    inp["dl_old"] = torch.full((B, H, W, lay.lddl), SENTINEL, dtype=F64)
    return inp


@functools.lru_cache(maxsize=None)
def kpcn_inputs(case, dtype, kind):
    return generate(case, dtype, kind)


@functools.lru_cache(maxsize=None)
def kpcn_reference(case, dtype, kind):
    return evaluate(kpcn_inputs(case, dtype, kind), case, dtype)
