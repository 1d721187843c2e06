"""Float64 reference, error budget and gates for the fused backward launches: dd_conv3x3_bwd (csrc/dd_conv_bwd.hip, csrc/dd_conv_bwd96.hip),
dd_conv3x3_bwd_multi, dd_convt2x2_fwd / dd_convt2x2_bwd (csrc/dd_convt.hip) and dd_pack_weights(_batched).  Never touches a GPU.

Every operation is restated as explicit shifted-slice sums over its 9 (or 4) taps in torch float64 -- no autograd, no oracle/np_ops, so that
tests/test_conv_bwd_ref.py can tie it to both.  Inputs are NHWC and representable in the storage type, so a bf16 x bf16 (f16 x f16) product is
exact in fp32 and the ONLY error of a correct kernel is the order of its fp32 sums and the rounding of its stores.

THE BUDGET next to every value is n * u * S: S = sum |a_i| |b_i| over the same slices (plus |bias| where it enters), n the number of terms,
u = 2^-24 -- the worst-case bound of ANY fp32 summation order (n - 1 additions, each off by at most u times a partial sum that never exceeds S).
THE GATES
    gate_f32(budget)                         = 2 * budget                                    (dw, db: fp32 atomics)
    gate_storage(ref, budget, dtype, points) = 2 * budget + half a storage ulp of (|v| + what may already be off) for every value v the path
                                               rounds: the partial sum of each launch, the running sum it is added to, and the result itself
(the same convention as tests/input_ref.py; the factor 2 covers second-order terms).  The kernels round a launch's sum BEFORE they add it to
what is stored (write_row of dd_conv_bwd.hip: pack, mask, unpack, add, pack), so `accumulate`, the per-64 launches of wide layers and of the
transposed conv each add half-ulps, taken from the reference's own partial sums."""
import functools
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
STORAGE = {"bf16": (torch.bfloat16, 8, -126), "f16": (torch.float16, 11, -14)}      # type, precision p, exponent of the smallest normal


# ---------------------------------------------------------------------------------------------------------------- rounding and gates
def representable(t, dtype):
    return t.to(STORAGE[dtype][0]).to(F64)


def to_storage(x, dtype):
    """x (fp32 or fp64 holding an fp32 value) rounded to the storage type as the kernels' stores do (round to nearest even), in float64."""
    return x.to(torch.float32).to(STORAGE[dtype][0]).to(F64)


def half_ulp(v, dtype):
    """Half an ulp of the storage type at |v| (subnormal spacing below the smallest normal)."""
    _, p, emin = STORAGE[dtype]
    v = v.abs()
    _, ex = torch.frexp(v)                               # |v| = m * 2^ex, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(ex, emin), (ex - 1).clamp_min(emin)).to(F64)
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=F64), e - (p - 1))


def gate_f32(budget, factor=2.0):
    return factor * budget


def gate_storage(ref, budget, dtype, roundings=(), factor=2.0):
    """2 * budget + half an ulp at every rounding.  `roundings`: the reference values the path rounds BEFORE the result (partial sums of
    earlier launches, running sums); the result `ref` is rounded last.  Each half-ulp is taken at |v| + everything that may be off by then."""
    g = factor * budget
    for v in list(roundings) + [ref]:
        g = g + half_ulp(v.abs() + g, dtype)
    return g


def ratio(got, ref, gate):
    """|got - ref| / gate per element; where the gate is 0 the value must be exact (ratio 0 or inf).  No element is left out."""
    diff = (got.to(F64) - ref).abs()
    return torch.where(gate > 0, diff / gate.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))


def worst_ratio(got, ref, gate):
    return float(ratio(got, ref, gate).max()) if ref.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- shifted slices
def shifted(a, oy, ox):
    """s[b, y, x] = a[b, y + oy, x + ox], zero outside the image (SAME padding)."""
    B, H, W, _ = a.shape
    s = torch.zeros_like(a)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        s[:, y0:y1, x0:x1] = a[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return s


def tap_offset(t):
    return t // 3 - 1, t % 3 - 1


def co_blocks(cout, block=64):
    return [(c, min(cout, c + block)) for c in range(0, cout, block)]


# ---------------------------------------------------------------------------------------------------------------- 3x3 SAME backward
def conv3_dx_part(dy, k, co0, co1, taps=range(9), flip=False, magnitudes=True):
    """sum over taps t and output channels [co0, co1) of dy[p - off(t)][co] * K[t][ci][co]  (include/dd_hip.h:117 with wd[t] = K[8 - t]);
    returns (value, magnitude sum; zero with magnitudes=False).  flip=True: the taps NOT flipped (a mutant)."""
    B, H, W, _ = dy.shape
    v = torch.zeros(B, H, W, k.shape[2], dtype=dy.dtype)
    s = torch.zeros_like(v)
    for t in taps:
        oy, ox = tap_offset(t)
        d = shifted(dy[..., co0:co1], -oy, -ox)
        kt = k.reshape(9, *k.shape[2:])[(8 - t) if flip else t]
        v += d @ kt[:, co0:co1].T
        if magnitudes:
            s += d.abs() @ kt[:, co0:co1].abs().T
    return v, s


def conv3_dw(x, dy):
    """dw[t][ci][co] = sum_p x[p + off(t)][ci] * dy[p][co] (TensorFlow layout [3][3][cin][cout]), db[co] = sum_p dy[p][co], with magnitudes."""
    cin, cout = x.shape[3], dy.shape[3]
    dw = torch.zeros(9, cin, cout, dtype=x.dtype)
    sw = torch.zeros_like(dw)
    d2, a2 = dy.reshape(-1, cout), dy.abs().reshape(-1, cout)
    for t in range(9):
        oy, ox = tap_offset(t)
        xs = shifted(x, oy, ox).reshape(-1, cin)
        dw[t] = xs.T @ d2
        sw[t] = xs.abs().T @ a2
    return dw.reshape(3, 3, cin, cout), sw.reshape(3, 3, cin, cout), d2.sum(0), a2.sum(0)


def dx_points(parts, mask, dx_old):
    """The values a path rounds, in order: every launch rounds its (masked) partial sum and, when it adds to what is stored, the new sum.  The
    last point is the result."""
    pts, run = [], dx_old
    for p in parts:
        p = p * mask if mask is not None else p
        pts.append(p)
        if run is not None:
            run = run + p
            pts.append(run)
        else:
            run = p
    return pts


def conv3_bwd(x, dy, k, use_mask=False, dx_old=None, per64=False):
    """Reference of dd_conv3x3_bwd.  per64: the data gradient runs as one launch per 64 output channels (cout > 96, or 65..96 with
    DD_CONV_BWD96=0), each rounding.  Returns a dict: dx / dx_budget / dx_points / dx_parts (per-64 partial sums, unmasked) and
    dw / dw_budget / db / db_budget."""
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    parts, S = [], torch.zeros(B, H, W, cin, dtype=x.dtype)
    for c0, c1 in co_blocks(cout):
        v, s = conv3_dx_part(dy, k, c0, c1)
        parts.append(v)
        S += s
    if dx_old is not None:
        S = S + dx_old.abs()
    mask = (x > 0).to(x.dtype) if use_mask else None
    launches = parts if per64 else [sum(parts)]
    pts = dx_points(launches, mask, dx_old)
    dw, sw, db, sb = conv3_dw(x, dy)
    n = B * H * W
    return dict(dx=pts[-1], dx_budget=9 * cout * U * S, dx_points=pts[:-1], dx_parts=parts,
                dw=dw, dw_budget=n * U * sw, db=db, db_budget=n * U * sb)


# ---------------------------------------------------------------------------------------------------------------- 2x2 / stride-2 transposed conv
def _fine(v, a, b):
    """The (a, b) parity plane of a fine-grid tensor [B, 2H, 2W, C]: pixel (2i + a, 2j + b) at (i, j)."""
    return v[:, a::2, b::2]


def convt_fwd(x, k, bias=None, relu=False, swap_ab=False):
    """y[2i+a][2j+b][co] = act(bias[co] + sum_ci x[i][j][ci] K[a][b][co][ci]); returns (y, budget)."""
    B, H, W, cin = x.shape
    cout = k.shape[2]
    y = torch.zeros(B, 2 * H, 2 * W, cout, dtype=x.dtype)
    s = torch.zeros_like(y)
    for a in range(2):
        for b in range(2):
            kab = k[b, a] if swap_ab else k[a, b]
            y[:, a::2, b::2] = x @ kab.T
            s[:, a::2, b::2] = x.abs() @ kab.abs().T
    if bias is not None:
        y, s = y + bias, s + bias.abs()
    return (torch.relu(y) if relu else y), cin * U * s


def convt_dx_part(dy, k, co0, co1, swap_ab=False):
    B, H2, W2, _ = dy.shape
    v = torch.zeros(B, H2 // 2, W2 // 2, k.shape[3], dtype=dy.dtype)
    s = torch.zeros_like(v)
    for a in range(2):
        for b in range(2):
            kab = (k[b, a] if swap_ab else k[a, b])[co0:co1]
            d = _fine(dy, a, b)[..., co0:co1]
            v += d @ kab
            s += d.abs() @ kab.abs()
    return v, s


def convt_bwd(x, dy, k, use_mask=False, dx_old=None):
    """Reference of dd_convt2x2_bwd (one launch per 64 output channels, each rounding dx)."""
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    parts, S = [], torch.zeros(B, H, W, cin, dtype=x.dtype)
    for c0, c1 in co_blocks(cout):
        v, s = convt_dx_part(dy, k, c0, c1)
        parts.append(v)
        S += s
    if dx_old is not None:
        S = S + dx_old.abs()
    mask = (x > 0).to(x.dtype) if use_mask else None
    pts = dx_points(parts, mask, dx_old)
    dw = torch.zeros(2, 2, cout, cin, dtype=x.dtype)
    sw = torch.zeros_like(dw)
    x2, xa = x.reshape(-1, cin), x.abs().reshape(-1, cin)
    for a in range(2):
        for b in range(2):
            d = _fine(dy, a, b).reshape(-1, cout)
            dw[a, b] = d.T @ x2
            sw[a, b] = d.abs().T @ xa
    db, sb = dy.reshape(-1, cout).sum(0), dy.abs().reshape(-1, cout).sum(0)
    n = B * H * W
    return dict(dx=pts[-1], dx_budget=4 * cout * U * S, dx_points=pts[:-1], dx_parts=parts,
                dw=dw, dw_budget=n * U * sw, db=db, db_budget=4 * n * U * sb)      # db reduces over the fine grid: 4 B H W terms


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation (CPU test)
def emulate_dx(parts32, x, use_mask, dx_old, dtype):
    """What a correct kernel stores: every launch's fp32 sum rounded to storage, masked, added in fp32 to what is stored, rounded."""
    run = None if dx_old is None else dx_old.clone()
    for p in parts32:
        v = to_storage(p, dtype)
        if use_mask:
            v = v * (x > 0).to(F64)
        run = v if run is None else to_storage((run.float() + v.float()), dtype)
    return run


# ---------------------------------------------------------------------------------------------------------------- weight packing
def round_up(a, b):
    return (a + b - 1) // b * b


def pack_dims(n, k):
    """n_pad / k_pad of engine.Layer.packed() for 2-byte storage."""
    return round_up(n, 16), round_up(round_up(k, 8), 32)


def pack_params(kind, role, cin, cout):
    """(taps, n, k, s_tap, s_n, s_k, tap_flip) of engine.Layer.packed(role) for a 3x3 conv ('conv') or the 2x2 transposed conv ('convT2')."""
    if kind == "conv":
        return (9, cout, cin, cin * cout, 1, cout, 0) if role == "fwd" else (9, cin, cout, cin * cout, cout, 1, 1)
    return (1, 4 * cout, cin, 0, cin, 1, 0) if role == "fwd" else (4, cin, cout, cout * cin, 1, cin, 0)


def pack_weights(src, dtype, taps, n, k, n_pad, k_pad, s_tap, s_n, s_k, tap_flip, dst=None, dst_off=0, dst_ld=0, dst_tap_stride=0):
    """numpy restatement of dd_pack_weights(_batched): dst[t][nn][kk] = src[tsrc * s_tap + nn * s_n + kk * s_k], tsrc = tap_flip ? taps-1-t : t,
    zero padded to [n_pad][k_pad], written at row stride dst_ld and tap stride dst_tap_stride (0: dense).  src: flat float32 array; returns the
    flat image in the storage type (torch, round to nearest even).  dst: an existing flat image to write into at element dst_off."""
    src = np.asarray(src, dtype=np.float32).reshape(-1)
    ld = dst_ld or k_pad
    ts = dst_tap_stride or n_pad * k_pad
    t, nn, kk = np.meshgrid(np.arange(taps), np.arange(n_pad), np.arange(k_pad), indexing="ij")
    valid = (nn < n) & (kk < k)
    idx = np.where(valid, (taps - 1 - t if tap_flip else t) * s_tap + nn * s_n + kk * s_k, 0)
    vals = np.where(valid, src[idx], np.float32(0)).astype(np.float32)
    if dst is None:
        dst = torch.zeros(dst_off + (taps - 1) * ts + (n_pad - 1) * ld + k_pad, dtype=STORAGE[dtype][0])
    where = torch.from_numpy((dst_off + t * ts + nn * ld + kk).reshape(-1).astype(np.int64))
    dst[where] = torch.from_numpy(vals.reshape(-1)).to(STORAGE[dtype][0])
    return dst


# ---------------------------------------------------------------------------------------------------------------- the cases of the GPU tests
# (cin, cout, B, H, W)
CONV_LE64 = [(8, 16, 1, 1, 1), (20, 40, 1, 3, 5), (64, 64, 2, 16, 16), (72, 40, 1, 17, 33), (136, 64, 1, 9, 20)]
CONV_96 = [(96, 96, 1, 16, 16), (40, 72, 1, 9, 35), (20, 70, 1, 3, 5), (24, 96, 1, 1, 16), (192, 80, 1, 17, 18)]
CONV_WIDE = [(64, 128, 2, 16, 16), (32, 160, 1, 17, 5), (72, 100, 1, 9, 20)]
CONV_WONLY = [(32, 128, 1, 16, 16), (24, 200, 1, 5, 33), (16, 40, 1, 3, 3)]
MULTI_GRIDS = [(2, 16, 16), (1, 9, 20)]
MULTI_CHANNELS = [(128, 128), (72, 40), (20, 200), (136, 70)]      # problem i of a multi launch: (cin, cout); a launch of n takes the first n
CONVT_FWD = [(128, 96, 1, 8, 8), (72, 48, 1, 5, 30), (8, 16, 1, 1, 1), (100, 32, 1, 3, 17)]
CONVT_BWD = [(96, 64, 1, 16, 16), (128, 96, 1, 8, 8), (72, 128, 1, 5, 30), (8, 16, 1, 1, 1), (40, 80, 1, 3, 17)]
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]      # (use_mask, accumulate)


def uneven_grid(ksplits):
    """(H, W) of two rows of 16 x 16 tiles (the last row one pixel high, the last column three wide) whose tile count is above every ksplit and
    a multiple of none -- and no larger than that needs, so that the worst-case budget of dw / db (n^2 u) stays below one pixel's term."""
    for n in range(2, 800):
        if all(n > k and n % k for k in ksplits):
            ty = 2 if n % 2 == 0 else 3 if n % 3 == 0 else 1      # (an odd count: three rows, or one)
            return 16 * (ty - 1) + 1, 16 * (n // ty - 1) + 3
    raise AssertionError("no uneven grid for %s" % (ksplits,))


def uneven_cases(cus=256):
    """One shape per route whose tiles are NOT dealt evenly: a workgroup walks tiles tile0, tile0 + ksplit, ... so with tiles % ksplit != 0 some
    workgroups walk one tile more than others.  ksplit = cus // (workgroup columns), capped at the tile count (dd_conv3x3_bwd,
    dd_conv_bwd96_launch); the transposed conv deals 8 x 8-pixel tiles to min(tiles, cus) workgroups.  The channel counts are chosen so that
    ksplit is about 20 and two dozen tiles suffice (cus = 256: 11 columns -> ksplit 23, 2 x 12 = 24 tiles = 23 + 1)."""
    nb = max(1, -(-cus // 24))                                   # workgroup columns that bring ksplit to <= 24
    out = {}
    H, W = uneven_grid([cus // nb])
    out["le64"] = (64 * nb - 4, 16, 1, H, W)                     # nblk = ceil(cin / 64) = nb
    out["bwd96"] = (32 * nb - 4, 72, 1, H, W)                    # nblk = ceil(cin / 32) = nb
    out["wide"] = (64 * nb - 4, 104, 1, H, W)                    # two launches of the cout <= 64 kernel
    nbw = -(-nb // 2)
    Hw, Ww = uneven_grid([cus // (2 * nbw)])
    out["wonly"] = (64 * nbw, 128, 1, Hw, Ww)                    # nblk * nblk_co = 2 * nbw columns
    tx = -(-(cus + 2) // 2)                                      # transposed conv: two rows of 8 x 8 tiles, cus + 2 (+ 1) tiles in all
    assert cus < 2 * tx < 2 * cus
    out["convt_fwd"] = (16, 16, 1, 9, 8 * (tx - 1) + 3)
    out["convt_bwd"] = (16, 16, 1, 9, 8 * (tx - 1) + 3)
    return out


def uneven_multi(cus=256):
    """Problems (cin, cout) of a 3-problem multi launch and its grid: problem i gets ksplit_i = cus // (3 * nblk_i * nblk_co_i) workgroups per
    column; the grid has more tiles than the largest ksplit_i and is a multiple of none of them (cus = 256: ksplit 14, 14, 10 and 16 tiles)."""
    probs = [(192, 128), (136, 70), (200, 100)]
    ks = [max(1, cus // (3 * -(-ci // 64) * -(-co // 64))) for ci, co in probs]
    H, W = uneven_grid(ks)
    return probs, (1, H, W)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def conv_inputs(shape, dtype):
    """x (about half of it <= 0, some exact zeros), dy, the HWIO kernel and an existing gradient, all representable in `dtype`."""
    cin, cout, B, H, W = shape
    g = _gen(*shape, 1 if dtype == "bf16" else 2)
    x = torch.randn(B, H, W, cin, generator=g, dtype=F64)
    x = torch.where(torch.rand(B, H, W, cin, generator=g, dtype=F64) < 0.1, torch.zeros_like(x), x)
    dy = torch.randn(B, H, W, cout, generator=g, dtype=F64)
    k = torch.randn(3, 3, cin, cout, generator=g, dtype=F64) / (3 * math.sqrt(cin))
    old = torch.randn(B, H, W, cin, generator=g, dtype=F64)
    return tuple(representable(t, dtype) for t in (x, dy, k, old))


@functools.lru_cache(maxsize=None)
def conv_reference(shape, dtype, use_mask, accumulate, per64):
    x, dy, k, old = conv_inputs(shape, dtype)
    return conv3_bwd(x, dy, k, bool(use_mask), old if accumulate else None, per64)


@functools.lru_cache(maxsize=None)
def convt_inputs(shape, dtype):
    """x, dy (fine grid), the kernel [2][2][cout][cin], bias and an existing gradient, representable (the bias is fp32: any float32 value)."""
    cin, cout, B, H, W = shape
    g = _gen(*shape, 3 if dtype == "bf16" else 4)
    x = torch.randn(B, H, W, cin, generator=g, dtype=F64)
    x = torch.where(torch.rand(B, H, W, cin, generator=g, dtype=F64) < 0.1, torch.zeros_like(x), x)
    dy = torch.randn(B, 2 * H, 2 * W, cout, generator=g, dtype=F64)
    k = torch.randn(2, 2, cout, cin, generator=g, dtype=F64) / math.sqrt(cin)
    bias = torch.randn(cout, generator=g, dtype=F64).float().to(F64)
    old = torch.randn(B, H, W, cin, generator=g, dtype=F64)
    x, dy, k, old = (representable(t, dtype) for t in (x, dy, k, old))
    return x, dy, k, bias, old


@functools.lru_cache(maxsize=None)
def convt_bwd_reference(shape, dtype, use_mask, accumulate):
    x, dy, k, _, old = convt_inputs(shape, dtype)
    return convt_bwd(x, dy, k, bool(use_mask), old if accumulate else None)


@functools.lru_cache(maxsize=None)
def convt_fwd_reference(shape, dtype, relu):
    x, _, k, bias, _ = convt_inputs(shape, dtype)
    return convt_fwd(x, k, bias, bool(relu))
