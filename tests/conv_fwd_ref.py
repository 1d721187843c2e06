"""Float64 reference, error budget, gates, expected kernel routes and the case table of tests/test_gpu_conv_fwd_ops.py: dd_conv_igemm
(csrc/dd_conv_igemm.hip, csrc/dd_conv_rw.hip, csrc/dd_conv_pw.hip), dd_conv_wgrad (csrc/dd_conv_wgrad.hip, csrc/dd_conv_pw.hip) and
dd_conv3x3_ks in mode 0 and in its transposed-conv parity modes 1 - 5 (csrc/dd_conv_ks.hip and the nine-tap GEMM route into
csrc/dd_conv_pw.hip) and in mode 6 on both of its routes.  Never touches a GPU.  The rounding helpers, gates, shifted slices and the 3x3 weight
gradient are those of tests/conv_bwd_ref.py, imported.

Every operation is restated as explicit shifted-slice sums in torch float64 -- no autograd, no oracle code; tests/test_conv_fwd_ref.py ties it
to both.  THE BUDGET next to every value is n * u * S (S the magnitude sum over the same slices plus |bias| and |residual|, n the number of
terms, u = 2^-24): the worst case of any fp32 summation order.  Inputs of the 2-byte paths are representable in the storage type, so their
products are exact in fp32.  The DD_F32 path has two input sets: "f32" holds bf16-representable values (exact products, n u S) and "f32full"
any float32 value (every product rounds as well: (n + 1) u S).

THE ROUNDINGS of a storage-type output, read off the epilogues (not the header):
  * every route packs the launch's fp32 sum (bias included, ReLU applied when there is no residual) to the storage type FIRST --
    conv_igemm_ws_kernel: `if (out_relu && !R) ...; pk.x = pack2<T>(a[0], a[1])` into the stage; conv_igemm_kernel (2-byte): the same lines of
    its BF epilogue; conv_rw_kernel / conv_rw8_kernel: `o2.x = pack2<T>(v[0], v[1])`;
  * a residual is then added to the ROUNDED sum and the result rounded again (`unpack8t<T>(o4, v); ... v[e] += t[e]; if (out_relu) ...;
    o4 = pack8t<T>(v)`; conv_rw*: "the conv result is rounded where the layer-wise path stores it, then the residual is added");
  * the mask selects bits (mask_bf16x8 / mask_bf16x2_cmp): no rounding;
  * DD_ACCUM adds what is stored to the ROUNDED (masked) value and rounds once more (`unpack8t<T>(o4, v); unpack8t<T>(av[k], t); v[e] += t[e];
    o4 = pack8t<T>(v)`).
So dd_conv_igemm with DD_ACCUM rounds the launch's sum BEFORE it is added (unlike dd_conv3x3_ks, documented as rounded once) on these routes.
  * conv_pw_kernel is the exception: ReLU, mask and `v[e] += o8[e]` all act on the fp32 sum and `const uint4 o = pack8t<T>(v)` rounds ONCE.
    The reference therefore carries two point lists, `points` and `points_pw` (empty: the add is one more fp32 rounding, u |y|, in the
    budget), and gate_y / emulate_y take the route that ran.  The f32 kernel (`store4<T>`) keeps fp32 throughout: no storage rounding; a residual or the stored value is
added to the finished sum in fp32, one more fp32 rounding (one fp32 ulp of the result is added to the gate)."""
import functools
import math

import torch

from conv_bwd_ref import (F64, STORAGE, U, conv3_dw, gate_f32, gate_storage, half_ulp, pack_dims, pack_params, pack_weights, ratio,  # noqa: F401
                          representable, round_up, shifted, tap_offset, to_storage, worst_ratio)

DD_IN_RELU, DD_OUT_RELU, DD_ACCUM, DD_PIXSHUF, DD_GATHER2X2 = 1, 2, 4, 8, 16
DTYPES2 = ("bf16", "f16")
F32SETS = ("f32", "f32full")


def is_f32(dtype):
    return dtype in F32SETS


def esize(dtype):
    return 4 if is_f32(dtype) else 2


def values_of(t, dtype):
    """t rounded to what the input set `dtype` may hold."""
    if dtype == "f32full":
        return t.float().to(F64)
    return representable(t, "bf16" if dtype == "f32" else dtype)


def ulp32(v):
    """One fp32 ulp at |v| (0 at 0)."""
    v = v.abs()
    _, ex = torch.frexp(v)
    return torch.where(v == 0, torch.zeros_like(v), torch.pow(torch.tensor(2.0, dtype=F64), (ex - 1).clamp_min(-126).to(F64) - 23))


# ---------------------------------------------------------------------------------------------------------------- dd_conv_igemm
def tap_input(x, taps, flags, t):
    """in(x)[map_t(p)] over the GEMM-row grid: 9 taps SAME (zero outside), 1 tap, or the 2x2 gather (tap t = 2a + b reads pixel (2y+a, 2x+b))."""
    if flags & DD_GATHER2X2:
        return x[:, (t >> 1)::2, (t & 1)::2]
    if taps == 9:
        return shifted(x, *tap_offset(t))
    return x


def conv_sum(x, w, taps, flags, tap_list=None, k0=0, k1=None):
    """sum over the taps of tap_list and channels [k0, k1) of in(x)[map_t(p)][k] * w[t][n][k], and the magnitude sum; w: [taps][n][cin]."""
    xin = torch.relu(x) if flags & DD_IN_RELU else x
    v = s = None
    for t in (range(taps) if tap_list is None else tap_list):
        xs = tap_input(xin, taps, flags, t)[..., k0:k1]
        wt = w[t][:, k0:k1]
        a, b = xs @ wt.T, xs.abs() @ wt.abs().T
        v, s = (a, b) if v is None else (v + a, s + b)
    return v, s


def pixshuf(v, swap=False):
    """[B, H, W, 4 cout], n = (2a + b) cout + co  ->  [B, 2H, 2W, cout] at (2y + a, 2x + b)."""
    B, H, W, n = v.shape
    c = n // 4
    out = torch.zeros(B, 2 * H, 2 * W, c, dtype=v.dtype)
    for ab in range(4):
        a, b = (ab & 1, ab >> 1) if swap else (ab >> 1, ab & 1)
        out[:, a::2, b::2] = v[..., ab * c:(ab + 1) * c]
    return out


def bias_vector(bias, nbias, n, flags):
    """bias[n] for n < nbias (DD_PIXSHUF: bias[n mod cout], cout = n / 4), zero elsewhere."""
    b = torch.zeros(n, dtype=F64)
    if bias is None:
        return b
    idx = torch.arange(n) % (n // 4) if flags & DD_PIXSHUF else torch.arange(n)
    ok = idx < nbias
    b[ok] = bias[idx[ok]]
    return b


def epilogue(v, s, nterms, res=None, mask=None, y_old=None, flags=0, res_after_relu=False, mask_ge=False, overwrite=False):
    """The epilogue of dd_conv_igemm on the sum v (bias included; already scattered for DD_PIXSHUF).  Returns y, budget, points (the values a
    2-byte path rounds before the result, see the module docstring) and `late` (a residual / stored value is added after the sum).  The three
    last arguments are mutants."""
    relu = bool(flags & DD_OUT_RELU)
    pts = []
    if res is None:
        y = torch.relu(v) if relu else v
    else:
        pts.append(v)
        s = s + res.abs()
        nterms += 1
        y = (torch.relu(v) + res) if res_after_relu else (v + res)
        y = torch.relu(y) if relu and not res_after_relu else y
    budget = nterms * U * s
    live = torch.ones_like(y)
    if mask is not None:
        live = ((mask >= 0) if mask_ge else (mask > 0)).to(F64)
        y, budget, pts = y * live, budget * live, [p * live for p in pts]
    late = res is not None
    budget_pw = budget
    if flags & DD_ACCUM and y_old is not None and not overwrite:
        pts.append(y)
        y = y + y_old
        late = True
        budget_pw = budget + U * y.abs() * live
    return dict(y=y, budget=budget, points=pts, budget_pw=budget_pw, points_pw=[], late=late, live=live, S=s, n=nterms)


def conv_fwd(x, w, bias=None, res=None, mask=None, y_old=None, taps=9, flags=0, nbias=None, full_precision=False):
    """include/dd_hip.h, dd_conv_igemm: y = epi(sum_{t,k} in(x)[map_t(p)][k] w[t][n][k] + bias[n] (n < nbias) + res); epi: optional ReLU, then
    * (mask > 0), then + y_old with DD_ACCUM.  w: the logical weight image [taps][n][cin].  Returns the dict of epilogue() (y, budget, points,
    S, n, late) plus `sum`, the pre-epilogue value."""
    n = w.shape[1]
    v, s = conv_sum(x, w, taps, flags)
    nterms = taps * x.shape[3] + (1 if full_precision else 0)
    if bias is not None:
        b = bias_vector(bias, n if nbias is None else nbias, n, flags)
        v, s, nterms = v + b, s + b.abs(), nterms + 1
    if flags & DD_PIXSHUF:
        v, s = pixshuf(v), pixshuf(s)
    out = epilogue(v, s, nterms, res, mask, y_old, flags)
    out["sum"] = v
    return out


def gate_y(ref, dtype, route=None):
    """The elementwise gate of a dd_conv_igemm output: 2 budget + half a storage ulp per rounding; f32 storage: 2 budget, plus one fp32 ulp where
    a residual or the stored value is added after the sum."""
    if is_f32(dtype):
        g = gate_f32(ref["budget"])
        return g + ulp32(ref["y"]) * ref["live"] if ref["late"] else g      # (a masked-out element is exactly 0, or exactly what was stored)
    if route == "pw":
        return gate_storage(ref["y"], ref["budget_pw"], dtype, ref["points_pw"])
    return gate_storage(ref["y"], ref["budget"], dtype, ref["points"])


def emulate_y(v32, res, mask, y_old, flags, dtype, route=None):
    """What a correct kernel stores, given its fp32 sum v32 (bias included, scattered): the roundings of the module docstring."""
    relu = bool(flags & DD_OUT_RELU)
    f = v32.float()
    if is_f32(dtype) or route == "pw":      # everything in fp32, one rounding at the store
        if res is not None:
            f = f + res.float()
        f = torch.relu(f) if relu else f
        if mask is not None:
            f = torch.where(mask > 0, f, torch.zeros_like(f))
        if flags & DD_ACCUM:
            f = f + y_old.float()
        return f.to(F64) if is_f32(dtype) else to_storage(f, dtype)
    if res is None:
        y = to_storage(torch.relu(f) if relu else f, dtype)
    else:
        y = to_storage(f, dtype).float() + res.float()
        y = to_storage(torch.relu(y) if relu else y, dtype)
    if mask is not None:
        y = y * (mask > 0).to(F64)
    if flags & DD_ACCUM:
        y = to_storage(y.float() + y_old.float(), dtype)
    return y


# ---------------------------------------------------------------------------------------------------------------- dd_conv_wgrad
def wgrad(p, q, taps=9, flags=0, bias_mode=0, pixels=None):
    """include/dd_hip.h, dd_conv_wgrad: out[t][m][n] = sum_p in(P)[map_t(p)][m] Q[p][n]; bias_mode 1: column sums of Q, 2: column sums of P (over
    P's own grid, the fine one under DD_GATHER2X2).  pixels: an optional [B, H, W, 1] 0/1 plane of the reduction pixels that count (a mutant).
    Returns dict(out [taps, m, n], out_budget, bias, bias_budget)."""
    B, H, W, n = q.shape
    m = p.shape[3]
    pin = torch.relu(p) if flags & DD_IN_RELU else p
    qq = q if pixels is None else q * pixels
    out = torch.zeros(taps, m, n, dtype=F64)
    s = torch.zeros_like(out)
    q2, qa = qq.reshape(-1, n), qq.abs().reshape(-1, n)
    if taps == 9 and not flags & DD_GATHER2X2:
        dw, sw, _, _ = conv3_dw(pin, qq)
        out, s = dw.reshape(9, m, n), sw.reshape(9, m, n)
    else:
        for t in range(taps):
            ps = tap_input(pin, taps, flags, t).reshape(-1, m)
            out[t], s[t] = ps.T @ q2, ps.abs().T @ qa
    npix = B * H * W
    r = dict(out=out, out_budget=npix * U * s, bias=None, bias_budget=None)
    if bias_mode == 1:
        r["bias"], r["bias_budget"] = q2.sum(0), npix * U * qa.sum(0)
    elif bias_mode == 2:
        r["bias"], r["bias_budget"] = p.reshape(-1, m).sum(0), p.shape[0] * p.shape[1] * p.shape[2] * U * p.abs().reshape(-1, m).sum(0)
    return r


def stacked_block(full, j, m0, width, shift=0):
    """Conv j of a dense block out of the full product [9][m][n]: column block j, rows below ITS input width m0 + j width.  shift = 1: the
    mutant that takes the prefix of block j - 1 (the rows above it stay zero)."""
    rows = m0 + j * width
    blk = full[:, :rows, j * width:(j + 1) * width].clone()
    if shift and j > 0:
        blk[:, m0 + (j - 1) * width:] = 0
    return blk


# ---------------------------------------------------------------------------------------------------------------- which kernel runs
# Restated from the dispatch code, NOT from running it: dd_conv_rw_eligible / dd_conv_rw_launch (csrc/dd_conv_rw.hip), dd_conv_pw_eligible
# (csrc/dd_conv_pw.hip), dispatch / launch_nt (csrc/dd_conv_igemm.hip), dispatch of csrc/dd_conv_wgrad.hip and dd_wgrad_pw_eligible.
LDS_ROW, TILE, LDS_BUDGET, PW_MIN_PIXELS = 128, 16, 158 * 1024, 32768


def _on(env, key):
    """`e ? atoi(e) : 1` of the switches read with getenv."""
    v = env.get(key)
    if v is None:
        return True
    try:
        return int(v) != 0
    except ValueError:
        return False


def _pw_on(env):
    return not env.get("DD_CONV_PW", "1").startswith("0")


def _ws_weight_bytes(taps, kchunks, nt):
    wb = nt * 16 * LDS_ROW
    return taps * ((kchunks + 1) // 2) * wb - (taps * (wb // 2) if kchunks & 1 else 0)


def igemm_route(c, dtype, env):
    """The route a dd_conv_igemm call takes.  c: an IgemmCase (its views are laid out as test_gpu_conv_fwd_ops.py lays them out: every pointer
    16-byte aligned and every ld a multiple of 8 elements, except a mask with mask_off8, which is 8-byte aligned only)."""
    two = not is_f32(dtype)
    es = esize(dtype)
    k_pad, n_pad = c.k_pad(dtype), c.n_pad
    relu, accum = bool(c.flags & DD_OUT_RELU), bool(c.flags & DD_ACCUM)
    mask16 = c.mask and not c.mask_off8
    bias = c.nbias is not None
    # ---- dd_conv_rw_eligible
    if _on(env, "DD_CONV_RW") and c.taps == 9 and two and (c.flags & ~(DD_OUT_RELU | DD_ACCUM)) == 0 and k_pad % 32 == 0:
        in96 = 64 < c.cin <= 96
        res_ok = not c.res or (not c.mask and not accum and in96)
        wide = 96 < c.cin <= 128 and k_pad <= 128
        mask_ok = not c.mask or (_on(env, "DD_CONV_RW8_MASK") and wide and not c.res and not bias and not relu and c.n % 8 == 0 and mask16)
        eligible = res_ok and ((in96 and k_pad <= 96) or (_on(env, "DD_CONV_RW8") and ((16 < c.cin <= 64 and k_pad <= 64) or wide) and mask_ok and not accum
                                                       and c.n >= 48))
        if eligible:      # ---- dd_conv_rw_launch
            on12, on12m = _on(env, "DD_CONV_RW12"), _on(env, "DD_CONV_RW12_MASK")
            masked12 = on12 and on12m and in96 and c.mask and not c.res and not bias and not accum and not relu and c.n >= 48 and c.n % 8 == 0 and mask16
            res12 = on12 and on12m and in96 and c.res and not c.mask and not accum and c.n >= 48 and c.n % 8 == 0
            twelve = on12 and in96 and ((not c.mask and not c.res and not accum) or masked12 or res12) and c.n >= 48
            if masked12:
                return "rw12_mask"
            if res12:
                return "rw12_res"
            if twelve:
                return "rw12"
            if in96:
                return "rw_6_2"
            if c.cin <= 64:
                return "rw8_kc2"
            return "rw8_kc4_mask" if c.mask else "rw8_kc4"
    # ---- dd_conv_pw_eligible
    if (_pw_on(env) and c.taps == 1 and two and not c.res and (c.flags & ~(DD_IN_RELU | DD_OUT_RELU | DD_ACCUM)) == 0 and n_pad > 64
            and c.B * c.H * c.W >= PW_MIN_PIXELS and c.cin % 8 == 0 and k_pad % 32 == 0 and (not c.mask or mask16)):
        return "pw"
    # ---- dispatch<T> and launch_nt<T, NT>
    kchunks = k_pad * es // 64
    tiles_n = n_pad // 16
    total_tiles = c.B * -(-c.H // TILE) * -(-c.W // TILE)
    cands = [w for w in (4, 3, 2, 1) if w == 1 or (-(-tiles_n // w) * w - tiles_n) * (5 if c.taps == 1 else 4) <= (2 if c.taps == 1 else 1) * tiles_n]
    nslabs = c.taps * ((kchunks + 1) // 2)
    patch = ((TILE + 2) ** 2 if c.taps == 9 else TILE * TILE) * LDS_ROW
    ws_ok = two and _on(env, "DD_CONV_WS")
    pick = 0
    for i, w in enumerate(cands):
        need = patch + (TILE * TILE * LDS_ROW + _ws_weight_bytes(c.taps, kchunks, w) + w * 64 if ws_ok else nslabs * w * 16 * LDS_ROW)
        if w >= (1 if ws_ok else 2) and need <= (160 * 1024 if ws_ok else LDS_BUDGET + 2048):
            pick = i
            break
    while pick + 1 < len(cands) and cands[pick] > 2 and total_tiles * -(-tiles_n // cands[pick]) < 256:
        pick += 1
    nt = cands[pick]
    if ws_ok and patch + TILE * TILE * LDS_ROW + _ws_weight_bytes(c.taps, kchunks, nt) + nt * 16 * 4 <= 160 * 1024:
        return "igemm_ws"
    return "igemm_resident" if patch + nslabs * nt * 16 * LDS_ROW <= LDS_BUDGET else "igemm_streamed"


def wgrad_route(c, dtype, env):
    """The route a dd_conv_wgrad call takes; "refused" where dispatch() returns DD_ERR_INVALID (the stacked form off the LDS-DMA kernel)."""
    two = not is_f32(dtype)
    gather = bool(c.flags & DD_GATHER2X2)
    if (_pw_on(env) and c.taps == 1 and two and c.bias_mode != 2 and (c.flags & ~DD_IN_RELU) == 0 and not (c.m <= 64 and c.n <= 64)
            and c.B * c.H * c.W >= PW_MIN_PIXELS):
        hi, lo = max(c.m, c.n), min(c.m, c.n)
        if not (128 < hi <= 256 and lo > 32 and not int(env.get("DD_WGRAD_PW_MID", "0") or 0)):
            return "wgrad_pw"
    kc = LDS_ROW // esize(dtype)
    if two and c.taps in (9, 1) and c.bias_mode != 2 and not gather and -(-c.m // kc) * -(-c.n // kc) <= 64 and _on(env, "DD_WGRAD_DMA"):
        return "wgrad_stacked" if c.stack else "wgrad_dma"
    return "refused" if c.stack else "wgrad_reg"


# ---------------------------------------------------------------------------------------------------------------- the cases
class IgemmCase:
    """One dd_conv_igemm call.  n: channels stored; n_pad: rows of the weight image (default: n rounded up to 16); nbias: None = no bias
    pointer; res / mask: operand present; mask_off8: the mask view starts 8 bytes off a 16-byte boundary; dtypes: the input sets it runs with."""

    def __init__(self, name, taps, cin, n, grid, flags=0, nbias=None, res=False, mask=False, n_pad=None, mask_off8=False, dtypes=DTYPES2, route=None):
        self.name, self.taps, self.cin, self.n, self.flags, self.nbias, self.res, self.mask = name, taps, cin, n, flags, nbias, res, mask
        self.B, self.H, self.W = grid
        self.n_pad = n_pad or round_up(n, 16)
        self.mask_off8, self.dtypes, self.route = mask_off8, dtypes, route      # route: what the issue names for the case with every switch on

    def k_pad(self, dtype):
        return round_up(self.cin, 16) if is_f32(dtype) else round_up(self.cin, 32)

    @property
    def accum(self):
        return bool(self.flags & DD_ACCUM)

    @property
    def id(self):
        return self.name

    def out_grid(self):
        return (self.B, 2 * self.H, 2 * self.W) if self.flags & DD_PIXSHUF else (self.B, self.H, self.W)

    def in_grid(self):
        return (self.B, 2 * self.H, 2 * self.W) if self.flags & DD_GATHER2X2 else (self.B, self.H, self.W)

    def out_channels(self):
        return self.n // 4 if self.flags & DD_PIXSHUF else self.n


R_, IR, AC, PS, GA = DD_OUT_RELU, DD_IN_RELU, DD_ACCUM, DD_PIXSHUF, DD_GATHER2X2
ALL3 = DTYPES2 + F32SETS
G2028, G933, G1716, G140, G371, G1616, G88 = (1, 20, 28), (2, 9, 33), (3, 17, 16), (2, 1, 40), (1, 37, 1), (2, 16, 16), (1, 8, 8)
IGEMM_CASES = [
    # ---- wave-specialised (2-byte); the same calls in f32 storage run on the plain kernel
    IgemmCase("ws 3x3 16->16", 9, 16, 16, G2028, nbias=16, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("ws 3x3 24->24 in-relu res", 9, 24, 24, G933, IR | R_, nbias=24, res=True, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("ws 3x3 192->96 relu", 9, 192, 96, G1716, R_, nbias=96, route="igemm_ws"),
    IgemmCase("3x3 96->192 mask", 9, 96, 192, G1616, mask=True, route="rw12_mask"),      # (96 input channels: by dd_conv_rw_eligible a register-weight layer)
    IgemmCase("ws 3x3 136->192 mask", 9, 136, 192, G1616, mask=True, route="igemm_ws"),
    IgemmCase("ws 1x1 64->25", 1, 64, 28, G140, nbias=25, n_pad=32, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("ws 1x1 8->24", 1, 8, 24, G371, nbias=24, dtypes=ALL3, route="igemm_ws"),      # (a 6-channel input is padded to 8: cin = 6 is refused, see the refusals)
    IgemmCase("ws 1x1 24->4 nbias 1", 1, 24, 4, G2028, nbias=1, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("ws 1x1 320->320 in-relu", 1, 320, 320, G88, IR, nbias=320, route="igemm_ws"),
    IgemmCase("ws 3x3 40->32 accum mask", 9, 40, 32, G933, AC, mask=True, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("ws 3x3 16->80 of 96", 9, 16, 80, G1716, R_, nbias=80, n_pad=96, dtypes=ALL3, route="igemm_ws"),
    # ---- a reduction too deep for resident weights: the plain kernel streams them, in 2-byte storage too
    IgemmCase("3x3 320->32 streamed", 9, 320, 32, G933, R_, nbias=32, route="igemm_streamed"),
    # ---- plain kernel, f32 storage: resident and streamed weights
    IgemmCase("f32 3x3 4->16", 9, 4, 16, G2028, R_, nbias=16, dtypes=F32SETS, route="igemm_resident"),
    IgemmCase("f32 3x3 32->64", 9, 32, 64, G933, R_, nbias=64, dtypes=F32SETS, route="igemm_resident"),
    IgemmCase("f32 3x3 96->96", 9, 96, 96, G1716, nbias=96, res=True, dtypes=F32SETS, route="igemm_resident"),
    IgemmCase("f32 3x3 192->96 streamed", 9, 192, 96, (1, 16, 16), R_, nbias=96, dtypes=F32SETS, route="igemm_streamed"),
    IgemmCase("f32 1x1 28->28", 1, 28, 28, G140, nbias=25, n_pad=32, dtypes=F32SETS, route="igemm_resident"),
    # ---- register-weight family (2-byte)
    IgemmCase("rw12 96->96", 9, 96, 96, G2028, R_, nbias=96, route="rw12"),
    IgemmCase("rw12 72->48", 9, 72, 48, G1716, R_, nbias=48, route="rw12"),
    IgemmCase("rw12 80->72", 9, 80, 72, G933, R_, nbias=72, route="rw12"),
    IgemmCase("rw12 mask 96->96", 9, 96, 96, G1716, mask=True, route="rw12_mask"),
    IgemmCase("rw12 mask 88->128", 9, 88, 128, G933, mask=True, route="rw12_mask"),
    IgemmCase("rw12 res 96->96", 9, 96, 96, G933, R_, nbias=96, res=True, route="rw12_res"),
    IgemmCase("rw12 res 80->64", 9, 80, 64, G2028, R_, nbias=64, res=True, route="rw12_res"),
    IgemmCase("rw6+2 96->96 accum", 9, 96, 96, G1716, AC, route="rw_6_2"),
    IgemmCase("rw6+2 72->16", 9, 72, 16, G2028, R_, nbias=16, route="rw_6_2"),
    IgemmCase("rw6+2 96->96 mask at 8 bytes", 9, 96, 96, G933, mask=True, mask_off8=True, route="rw_6_2"),
    IgemmCase("rw8 kc2 32->64", 9, 32, 64, G2028, R_, nbias=64, route="rw8_kc2"),
    IgemmCase("rw8 kc2 24->48", 9, 24, 48, G933, R_, nbias=48, route="rw8_kc2"),
    IgemmCase("rw8 kc2 64->96", 9, 64, 96, G1716, nbias=96, route="rw8_kc2"),
    IgemmCase("rw8 kc4 128->128", 9, 128, 128, G1716, R_, nbias=128, route="rw8_kc4"),
    IgemmCase("rw8 kc4 104->112", 9, 104, 112, G933, R_, nbias=112, route="rw8_kc4"),
    IgemmCase("rw8 kc4 mask 128->112", 9, 128, 112, (2, 13, 19), mask=True, route="rw8_kc4_mask"),
    # ---- just outside the eligibility borders of the family
    IgemmCase("border cin 16 -> ws", 9, 16, 64, G933, R_, nbias=64, route="igemm_ws"),
    IgemmCase("border cin 136 -> ws", 9, 136, 64, G933, R_, nbias=64, route="igemm_ws"),
    IgemmCase("border n 44, cin 64 -> ws", 9, 64, 44, G933, R_, nbias=44, route="igemm_ws"),
    IgemmCase("border n 44, cin 96 -> 6+2", 9, 96, 44, G933, R_, nbias=44, route="rw_6_2"),
    IgemmCase("border n 48, cin 64 -> kc2", 9, 64, 48, G933, R_, nbias=48, route="rw8_kc2"),
    IgemmCase("border cin 104 mask + bias -> ws", 9, 104, 64, G933, nbias=64, mask=True, route="igemm_ws"),
    # ---- 2x2 gather (transposed-conv data gradient) and pixel shuffle (its forward)
    IgemmCase("gather 96->64", 4, 96, 64, G933, GA, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("gather 96->64 mask", 4, 96, 64, G1716, GA, mask=True, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("gather 32->16", 4, 32, 16, G2028, GA, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("gather 32->16 mask", 4, 32, 16, G140, GA, mask=True, dtypes=ALL3, route="igemm_ws"),
    IgemmCase("pixshuf 128->4x24", 1, 128, 96, G933, PS | R_, nbias=24, dtypes=("bf16", "f32", "f32full"), route="igemm_ws"),
    IgemmCase("pixshuf 64->4x16", 1, 64, 64, G1716, PS | R_, nbias=16, dtypes=("bf16", "f32", "f32full"), route="igemm_ws"),
    # the narrowest cout 2-byte storage takes (one 8-channel vector per output pixel: dd_conv_igemm refuses cout % 8 != 0 there)
    IgemmCase("pixshuf 32->4x8", 1, 32, 32, G2028, PS | R_, nbias=8, dtypes=ALL3, route="igemm_ws"),
]
# the wide 1x1 kernel needs 32 768 pixels: 2 x 128 x 128, here and nowhere else
G128 = (2, 128, 128)
PW_CASES = [
    IgemmCase("pw 176->176 in-relu", 1, 176, 176, G128, IR, nbias=176, route="pw"),
    IgemmCase("pw 80->320 relu", 1, 80, 320, G128, R_, nbias=320, route="pw"),
    IgemmCase("pw 176->72 mask accum", 1, 176, 72, G128, AC, mask=True, route="pw"),
]


class WgradCase:
    """One dd_conv_wgrad call; stack = (m0, width, blocks) for the stacked dense-block form (then m, n follow from it)."""

    def __init__(self, name, taps, m, n, grid, flags=0, bias_mode=0, ksplit=0, stack=None, dtypes=DTYPES2 + ("f32",), prefill=False, route=None):
        if stack:
            m0, width, blocks = stack
            m, n = m0 + (blocks - 1) * width, blocks * width
        self.name, self.taps, self.m, self.n, self.flags, self.bias_mode, self.ksplit, self.stack = name, taps, m, n, flags, bias_mode, ksplit, stack
        self.B, self.H, self.W = grid
        self.dtypes, self.prefill, self.route = dtypes, prefill, route

    @property
    def id(self):
        return self.name

    def p_grid(self):
        return (self.B, 2 * self.H, 2 * self.W) if self.flags & DD_GATHER2X2 else (self.B, self.H, self.W)


WGRAD_CASES = [
    # the 2-byte sets run on the LDS-DMA kernel, the f32 set of the same call on the register-staged one
    WgradCase("3x3 32x64", 9, 32, 64, G2028, bias_mode=1, route="wgrad_dma", prefill=True),
    WgradCase("3x3 72x16 in-relu", 9, 72, 16, G933, IR, bias_mode=1, ksplit=1, route="wgrad_dma"),
    WgradCase("3x3 96x96", 9, 96, 96, G1716, bias_mode=1, ksplit=3, route="wgrad_dma"),
    WgradCase("3x3 192x96 ksplit>tiles", 9, 192, 96, G1616, bias_mode=1, ksplit=50, route="wgrad_dma"),
    WgradCase("3x3 24x40", 9, 24, 40, G140, bias_mode=1, route="wgrad_dma"),
    WgradCase("3x3 20x12 odd pads", 9, 20, 12, G371, bias_mode=1, route="wgrad_dma"),
    WgradCase("1x1 64x25", 1, 64, 25, G2028, bias_mode=1, route="wgrad_dma"),
    WgradCase("1x1 400x400", 1, 400, 400, G88, IR, route="wgrad_dma"),
    WgradCase("gather 64x96 bias of P", 4, 64, 96, G933, GA, bias_mode=2, route="wgrad_reg", prefill=True),
    WgradCase("gather 16x32", 4, 16, 32, G1716, GA, bias_mode=2, route="wgrad_reg"),
    WgradCase("1x1 576x576 (81 slice pairs)", 1, 576, 576, G88, dtypes=DTYPES2, route="wgrad_reg"),
    WgradCase("stacked 16+16x4", 9, 0, 0, G2028, IR, bias_mode=1, stack=(16, 16, 4), dtypes=DTYPES2, route="wgrad_stacked", prefill=True),
    WgradCase("stacked 40+24x4", 9, 0, 0, G933, IR, bias_mode=1, stack=(40, 24, 4), dtypes=DTYPES2, route="wgrad_stacked"),
    WgradCase("stacked 64+32x2", 9, 0, 0, G1716, bias_mode=0, stack=(64, 32, 2), dtypes=DTYPES2, route="wgrad_stacked"),
    WgradCase("stacked 24+8x3", 9, 0, 0, G140, IR, bias_mode=1, stack=(24, 8, 3), dtypes=DTYPES2, route="wgrad_stacked"),
]
WGRAD_PW_CASES = [
    WgradCase("pw 1x1 176x176 (mid: stays on dma)", 1, 176, 176, G128, bias_mode=1, dtypes=DTYPES2, route="wgrad_dma"),
    WgradCase("pw 1x1 80x320", 1, 80, 320, G128, IR, bias_mode=1, dtypes=DTYPES2, route="wgrad_pw", prefill=True),
    WgradCase("pw 1x1 64x64 (stays on dma)", 1, 64, 64, G128, bias_mode=1, dtypes=DTYPES2, route="wgrad_dma"),
]


class KsCase:
    """One dd_conv3x3_ks call in mode 0: output channels [n0, n0 + n) of a layer whose weight image has n0 + n rows, written into channels
    cin .. cin + n of the very buffer whose first cin channels are the input (a dense block's concat buffer).  grad: the gradient epilogue
    (DD_ACCUM and / or a mask, no bias, rounded once: `o2.x = pack2<T>(o8[0] + ((!has_mask || m8[0] > 0.f) ? v[0] : 0.f), ...)`)."""

    def __init__(self, name, cin, n, n0, grid, flags=0, nbias=None, mask=False, mask_off8=False, route="ks"):
        self.name, self.cin, self.n, self.n0, self.flags, self.nbias, self.mask, self.mask_off8, self.route = name, cin, n, n0, flags, nbias, mask, mask_off8, route
        self.B, self.H, self.W = grid
        self.taps, self.res, self.dtypes = 9, False, DTYPES2
        self.n_pad = round_up(n0 + n, 16)

    @property
    def id(self):
        return self.name

    @property
    def accum(self):
        return bool(self.flags & DD_ACCUM)

    @property
    def grad(self):
        return self.accum or self.mask

    def k_pad(self, dtype):
        return round_up(self.cin, 32)


def ks_route(c, env):
    """dd_conv_pw_taps_eligible (csrc/dd_conv_pw.hip) for mode 0: the gradient epilogue with more than 128 channels from n0 = 0 on at least
    2 048 pixels goes to the nine-tap GEMM form; the test's views are 16-byte aligned with ld % 8 == 0 unless mask_off8."""
    if (_pw_on(env) and c.grad and c.n > 128 and c.n0 == 0 and not (c.flags & (DD_IN_RELU | DD_OUT_RELU)) and c.B * c.H * c.W >= 2048 and c.cin % 8 == 0
            and (not c.mask or not c.mask_off8)):
        return "ks_pw_taps"
    return "ks"


G3232 = (2, 32, 32)
KS_CASES = [
    KsCase("16->16 at 0", 16, 16, 0, G2028, IR | R_, nbias=16),
    KsCase("72->24 at 16", 72, 24, 16, G933, IR | R_, nbias=40),
    KsCase("168->48 at 64 nbias short", 168, 48, 64, G1716, IR, nbias=100),
    KsCase("296->64 at 0", 296, 64, 0, G140, IR | R_, nbias=64),
    KsCase("1088->96 at 16", 1088, 96, 16, G933, IR | R_, nbias=112),
    KsCase("72->128 at 0 no bias", 72, 128, 0, G371, IR),
    KsCase("grad 72->24 at 16 accum mask", 72, 24, 16, G933, AC, mask=True),
    KsCase("grad 168->64 at 0 accum", 168, 64, 0, G1716, AC),
    KsCase("grad 40->96 at 64 mask", 40, 96, 64, G2028, mask=True),
    KsCase("grad 72->48 at 0 accum mask at 8 bytes", 72, 48, 0, G140, AC, mask=True, mask_off8=True),
    KsCase("grad 96->192 nine-tap GEMM", 96, 192, 0, G3232, AC, mask=True, route="ks_pw_taps"),
]


# dd_conv3x3_ks modes 1 .. 5: (cin, n, n0, grid, relu, nbias)
KST_CASES = [(40, 16, 0, (1, 8, 8), 1, 16), (136, 64, 16, (2, 9, 13), 0, 70), (40, 96, 0, (1, 1, 5), 1, 96), (136, 16, 64, (1, 9, 13), 1, 80)]


def convt3_image(k):
    """The weight image of modes 1 .. 5: what dd_pack_weights builds for the zero-stuffed form, taps flipped -- image tap (uy, ux) =
    K[2 - uy][2 - ux]; k: TensorFlow layout [3][3][cout][cin]; returns the logical image [9][cout][cin]."""
    return k.flip(0).flip(1).reshape(9, k.shape[2], k.shape[3])


def conv_ks_t(x, k, bias, n0, n, nbias, relu):
    """include/dd_hip.h, dd_conv3x3_ks modes 1 .. 5: the 3x3 / stride-2 SAME transposed conv, rows / columns 2H, 2W dropped --
    y[2i + py][2j + px][n0 + c] = act(bias + sum over the taps a = py, b = px (mod 2) of x[i - a/2][j - b/2][ci] K[a][b][n0 + c][ci]).
    Returns (y [B, 2H, 2W, n], budget); rounded once."""
    B, H, W, cin = x.shape
    y = torch.zeros(B, 2 * H, 2 * W, n, dtype=F64)
    s = torch.zeros_like(y)
    terms = torch.zeros(1, 2 * H, 2 * W, 1, dtype=F64)
    for a in range(3):
        for b in range(3):
            xs = shifted(x, -(a // 2), -(b // 2))
            kab = k[a, b, n0:n0 + n]
            y[:, a % 2::2, b % 2::2] += xs @ kab.T
            s[:, a % 2::2, b % 2::2] += xs.abs() @ kab.abs().T
            terms[:, a % 2::2, b % 2::2] += cin
    if bias is not None:
        bv = bias_vector(bias, nbias, n0 + n, 0)[n0:]
        y, s, terms = y + bv, s + bv.abs(), terms + 1
    return (torch.relu(y) if relu else y), terms * U * s


# ---- dd_conv3x3_ks mode 6, as csrc/dd_conv_ks.hip (PY = PX = 2: image taps 1 and 2 of each axis at input offsets 0 and +1) and
# dd_conv_pw_taps_launch (csrc/dd_conv_pw.hip: "tap t reads pixel (i + (t >> 1), j + (t & 1)) of the H x W grid (zero outside) against image tap
# (1 + (t >> 1)) * 3 + 1 + (t & 1)") define it: a 2 x 2-tap conv on the input grid,
#     y[i][j][n0 + c] = epi( sum_{dy, dx in {0, 1}} sum_k x[i + dy][j + dx][k] * w[(1 + dy) * 3 + (1 + dx)][n0 + c][k] ),
# with the epilogues of mode 0 (bias / ReLU, or the gradient epilogue), rounded once; image taps 0, 1, 2, 3, 6 are never read.  Its one use is the
# data gradient of the 3x3 / stride-2 transposed conv over the output gradient rearranged by parity, s[i][j][plane * cp + co] =
# dy[2i + py][2j + px][co], plane = 2 py + px: kernel tap (a, b) sits at image tap (1 + (a == 2)) * 3 + 1 + (b == 2), columns of plane
# 2 (a & 1) + (b & 1).  The GEMM route skips the (tap, 64-channel chunk) pairs that meet no such block (py <= 1 - dy and px <= 1 - dx), so the
# other blocks of the image must be zero -- as they are here.
# (cp, n, n0, grid, flags, nbias or None, mask, route with every switch on)
K6_CASES = [(10, 24, 16, (2, 9, 13), DD_ACCUM, None, True, "ks"), (18, 16, 0, (1, 8, 8), DD_OUT_RELU, 12, False, "ks"),
            (34, 64, 0, (1, 1, 5), 0, None, True, "ks"), (24, 192, 0, (2, 32, 32), DD_ACCUM, None, True, "ks_pw_taps"),
            (8, 136, 0, (2, 32, 32), 0, 136, False, "ks_pw_taps")]


def s2d_blocks():
    """[(a, b, dy, dx, plane, image tap)] of the nine kernel taps (the arithmetic of deepdenoiser_amd.engine.convt3_s2d_blocks, restated)."""
    return [(a, b, int(a == 2), int(b == 2), (a & 1) * 2 + (b & 1), (1 + int(a == 2)) * 3 + 1 + int(b == 2)) for a in range(3) for b in range(3)]


def space_to_depth(dy):
    """s[i][j][plane * cp + co] = dy[2i + py][2j + px][co], plane = 2 py + px."""
    return torch.cat([dy[:, py::2, px::2] for py in range(2) for px in range(2)], dim=3)


def mode6_image(k, filler=None):
    """The logical weight image [9][ci][4 cp] of mode 6 from the kernel K[a][b][co][ci] (TensorFlow layout [3][3][cout][cin]); the taps mode 6
    never reads hold `filler` (so that a read of them shows), the blocks no kernel tap fills are zero."""
    cp, n = k.shape[2], k.shape[3]
    w = torch.zeros(9, n, 4 * cp, dtype=k.dtype)
    if filler is not None:
        for t in (0, 1, 2, 3, 6):
            w[t] = filler[t]
    for a, b, _, _, plane, tap in s2d_blocks():
        w[tap][:, plane * cp:(plane + 1) * cp] = k[a, b].T
    return w


def conv_ks6(x, w, bias, mask, y_old, n0, n, flags, nbias, swap_offsets=False):
    """dd_conv3x3_ks mode 6 (see above).  x [B, H, W, cin], w the logical image [9][n0 + n][cin].  swap_offsets: the mutant that reads
    (i + dx, j + dy).  Returns the dict of epilogue(); gate it with gate_y(ref, dtype, "pw") (one rounding)."""
    v = torch.zeros(x.shape[:3] + (n,), dtype=F64)
    s = torch.zeros_like(v)
    live = 0
    for dy in range(2):
        for dx in range(2):
            wt = w[(1 + dy) * 3 + 1 + dx][n0:n0 + n]
            xs = shifted(x, dx, dy) if swap_offsets else shifted(x, dy, dx)
            v, s = v + xs @ wt.T, s + xs.abs() @ wt.abs().T
            live = live + (wt != 0).sum(1).max().item()
    nterms = max(int(live), 1)      # the products that are not exact zeros (9 cp for the transposed conv's image)
    if bias is not None:
        b = bias_vector(bias, nbias, n0 + n, 0)[n0:]
        v, s, nterms = v + b, s + b.abs(), nterms + 1
    out = epilogue(v, s, nterms, None, mask, y_old, flags)
    out["sum"] = v
    return out


def ks6_route(case, env):
    """dd_conv_pw_taps_eligible for mode 6 (the test's views are 16-byte aligned with ld % 8 == 0)."""
    cp, n, n0, (B, H, W), flags, _, _, _ = case
    cin = 4 * cp
    if (_pw_on(env) and n > 128 and n0 == 0 and not (flags & (DD_IN_RELU | DD_OUT_RELU)) and 2048 <= B * H * W < 2 ** 31 and cin % 4 == 0
            and 4 * -(-cin // 64) <= 40 and cin % 8 == 0):
        return "ks_pw_taps"
    return "ks"


@functools.lru_cache(maxsize=None)
def k6_inputs(case, dtype):
    """dy (fine grid), K [3][3][cp][n0 + n], bias, mask, the stored values, and the filler of the unread image taps."""
    cp, n, n0, grid, _, _, _, _ = case
    B, H, W = grid
    g = _gen("k6", case, dtype)
    dy = _signed((B, 2 * H, 2 * W, cp), g)
    k = torch.randn(3, 3, cp, n0 + n, generator=g, dtype=F64) / math.sqrt(9 * cp)
    bias = torch.randn(n0 + n, generator=g, dtype=F64).float().to(F64)
    mask = _signed((B, H, W, n), g)
    old = torch.randn(B, H, W, n, generator=g, dtype=F64)
    filler = 3.0 + torch.rand(9, n0 + n, 4 * cp, generator=g, dtype=F64)
    dy, k, mask, old, filler = (values_of(t, dtype) for t in (dy, k, mask, old, filler))
    return dy, k, bias, mask, old, filler


@functools.lru_cache(maxsize=None)
def k6_reference(case, dtype):
    cp, n, n0, grid, flags, nbias, use_mask, _ = case
    dy, k, bias, mask, old, filler = k6_inputs(case, dtype)
    return conv_ks6(space_to_depth(dy), mode6_image(k, filler), bias if nbias is not None else None, mask if use_mask else None,
                    old if flags & DD_ACCUM else None, n0, n, flags, nbias)


@functools.lru_cache(maxsize=None)
def kst_inputs(case, dtype):
    cin, n, n0, grid, _, _ = case
    g = _gen("kst", case, dtype)
    x = _signed(grid + (cin,), g)
    k = torch.randn(3, 3, n0 + n, cin, generator=g, dtype=F64) / math.sqrt(4 * cin)
    bias = torch.randn(n0 + n, generator=g, dtype=F64).float().to(F64)
    return values_of(x, dtype), values_of(k, dtype), bias


@functools.lru_cache(maxsize=None)
def kst_reference(case, dtype):
    cin, n, n0, grid, relu, nbias = case
    x, k, bias = kst_inputs(case, dtype)
    return conv_ks_t(x, k, bias, n0, n, nbias, relu)


# ---------------------------------------------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def ks_inputs(case_id, dtype):
    """x, the whole logical weight image [9][n0 + n][cin], bias (n0 + n fp32 values), mask and the stored values [.., n]."""
    c = KS_BY_ID[case_id]
    g = _gen("ks", case_id, dtype)
    x = _signed((c.B, c.H, c.W, c.cin), g)
    w = torch.randn(9, c.n0 + c.n, c.cin, generator=g, dtype=F64) / math.sqrt(9 * c.cin)
    bias = torch.randn(c.n0 + c.n, generator=g, dtype=F64).float().to(F64)
    mask = _signed((c.B, c.H, c.W, c.n), g)
    old = torch.randn(c.B, c.H, c.W, c.n, generator=g, dtype=F64)
    x, w, mask, old = (values_of(t, dtype) for t in (x, w, mask, old))
    return x, w, bias, mask, old


def conv_ks(x, w, bias, mask, y_old, n0, n, flags, nbias, bias_from_zero=False):
    """include/dd_hip.h, dd_conv3x3_ks mode 0: y[p][n0 + c] = act(bias[n0 + c] (n0 + c < nbias) + sum_{t,ci} w[t][n0 + c][ci] in(x[p + off(t)][ci])), or
    with the gradient epilogue y[p][n0 + c] += (mask > 0) sum -- no bias, no activation, rounded once.  bias_from_zero: the mutant that
    ignores n0 for the bias.  Returns the dict of conv_fwd(); gate it with gate_y(ref, dtype, "pw") (one rounding)."""
    b = None
    if bias is not None:
        full = bias_vector(bias, nbias, n0 + n, 0)
        b = full[:n] if bias_from_zero else full[n0:n0 + n]
    return conv_fwd(x, w[:, n0:n0 + n], b, None, mask, y_old, 9, flags)


@functools.lru_cache(maxsize=None)
def ks_reference(case_id, dtype):
    c = KS_BY_ID[case_id]
    x, w, bias, mask, old = ks_inputs(case_id, dtype)
    return conv_ks(x, w, None if c.grad or c.nbias is None else bias, mask if c.mask else None, old if c.accum else None, c.n0, c.n, c.flags, c.nbias)


def _gen(*key):
    h = 0
    for v in key:
        for ch in str(v):
            h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _signed(shape, g, shift=0.43, zeros=0.06):
    """Normal values of which about a third are <= 0, with some exact +0.0 and -0.0."""
    t = torch.randn(*shape, generator=g, dtype=F64) + shift
    r = torch.rand(*shape, generator=g, dtype=F64)
    t = torch.where(r < zeros, torch.zeros_like(t), t)
    return torch.where(r < zeros / 2, -torch.zeros_like(t), t)


@functools.lru_cache(maxsize=None)
def igemm_inputs(case_id, dtype):
    """x, w [taps][n][cin], bias (fp32 values, n of them), res, mask, y_old -- all in the value set of `dtype`; the operands a case does not use
    are still drawn, so that a case's inputs do not depend on its flags."""
    c = IGEMM_BY_ID[case_id]
    g = _gen(case_id, dtype)
    og, oc = c.out_grid(), c.out_channels()
    x = _signed(c.in_grid() + (c.cin,), g)
    w = torch.randn(c.taps, c.n, c.cin, generator=g, dtype=F64) / math.sqrt(c.taps * c.cin)
    bias = torch.randn(c.n, generator=g, dtype=F64).float().to(F64)
    res = torch.randn(*og, oc, generator=g, dtype=F64)
    mask = _signed(og + (oc,), g)
    old = torch.randn(*og, oc, generator=g, dtype=F64)
    x, w, res, mask, old = (values_of(t, dtype) for t in (x, w, res, mask, old))
    return x, w, bias, res, mask, old


@functools.lru_cache(maxsize=None)
def igemm_reference(case_id, dtype):
    c = IGEMM_BY_ID[case_id]
    x, w, bias, res, mask, old = igemm_inputs(case_id, dtype)
    return conv_fwd(x, w, bias if c.nbias is not None else None, res if c.res else None, mask if c.mask else None, old if c.accum else None,
                    c.taps, c.flags, c.nbias, full_precision=dtype == "f32full")


def prefilled(value, budget, npix):
    """value / budget of an fp32 output the launch adds to PREFILL: one more term of that magnitude."""
    return value + PREFILL, (npix + 1) * (budget / npix + U * PREFILL)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(case_id, dtype):
    c = WGRAD_BY_ID[case_id]
    g = _gen(case_id, dtype)
    p = _signed(c.p_grid() + (c.m,), g)
    q = torch.randn(c.B, c.H, c.W, c.n, generator=g, dtype=F64)
    return values_of(p, dtype), values_of(q, dtype)


@functools.lru_cache(maxsize=None)
def wgrad_reference(case_id, dtype):
    c = WGRAD_BY_ID[case_id]
    p, q = wgrad_inputs(case_id, dtype)
    return wgrad(p, q, c.taps, c.flags, c.bias_mode)


PREFILL = 0.375      # what `out` / bias_out hold before a prefill case: the launch must ADD to it (exact in fp32; its rounding is one more term)
IGEMM_BY_ID = {c.id: c for c in IGEMM_CASES + PW_CASES}
WGRAD_BY_ID = {c.id: c for c in WGRAD_CASES + WGRAD_PW_CASES}
KS_BY_ID = {c.id: c for c in KS_CASES}
assert len(KS_BY_ID) == len(KS_CASES)
assert len(IGEMM_BY_ID) == len(IGEMM_CASES) + len(PW_CASES) and len(WGRAD_BY_ID) == len(WGRAD_CASES) + len(WGRAD_PW_CASES)
