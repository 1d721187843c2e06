"""Float64 reference, per-element bounds, mutants and case tables of the single-pass kernels of csrc/dd_pointwise.hip: max-pool
forward / backward, masked add, zero-stuffing and its inverse, space-to-depth, channel conversion, the layer-wise compose path, the column
sums, tile extraction and stitching.  Never touches a GPU; tests/test_pointwise_ref.py (CPU) and tests/test_gpu_pointwise_ops.py (-m gpu) read
the very same inputs from here.

Everything is written from the formulas (oracle/tf_ops.py) as loops over windows / index arithmetic on whole NHWC
float64 tensors, not from the kernels' thread mapping.  A function evaluated with `mut={"name"}` is a MUTANT (MUTANTS below), evaluated with
dtype=torch.float32 (where it adds) an honest float32 evaluation.

GATES (none is tuned to the code under test)
    selection and copies            bit-equal to the reference; padding exactly +0; a store into a 2-byte type is round-to-nearest-even of the
                                    fp32 value (tensor.to(dtype))
    integer-valued adding cases     bit-equal: every partial sum of every order stays below 2^24 in magnitude (sum |terms| < 2^24) and the result
                                    is representable in the storage type -- exact_in_fp32() asserts both on the CPU for the inputs used
    real-valued adding cases        |got - ref| <= r_T(ref) + (n - 1) * 2^-24 * sum |terms|, n = the addends of that element (the windows whose
                                    code points at the pixel, plus one for accumulate), r_T = half an ulp of the storage type at ref (0 for fp32):
                                    (n - 1) u sum|terms| bounds any order of fp32 additions (Higham (4.4), first order), the one store rounds once
    sigmoid of the blend            rel-L2 by kind, gpu_util.ACC32 (fp32 out, d_small, d_fine) / gpu_util.ROUND[dtype] (dwl): the device's fast
                                    exponential has no published accuracy here
    real-valued column sums         gpu_util.ACC32"""
import functools

import torch

import conv_bwd_ref as CR

F64 = torch.float64
U = 2.0 ** -24
SENTINEL = 12288.0      # exact in fp32, bf16 and fp16 (conv_ops_util.SENTINEL)
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPES = ("f32", "bf16", "f16")
PER16 = {"f32": 4, "bf16": 8, "f16": 8}

# what each mutant gets wrong -> the functions whose gate must catch it (tests/test_pointwise_ref.py asserts every row)
MUTANTS = {
    "last_max_wins": "the last maximum of a window wins instead of the first",
    "pad_before": "the odd padding cell put before the image instead of after it (even sizes)",
    "padded_cells_win": "a padded cell competes with value 0",
    "offset2_as_1": "window offset 2 decoded as 1 in the backward",
    "out_of_image_window": "a window outside the output grid (read at a clamped address) contributes its gradient",
    "relu_mask_ignored": "a non-positive maximum keeps its code",
    "mask_after_accumulate": "the mask applied to gradient + old instead of to the gradient",
    "accumulate_dropped": "the old value overwritten",
    "parity_swapped": "space-to-depth planes px * 2 + py",
    "stuffed_even": "the stuffed sample at (even, even) instead of (odd, odd)",
    "x_not_halved": "compose_pack reads small at column x instead of x / 2",
    "low_not_quarter": "the 2 x 2 sum of fine not multiplied by 0.25",
    "wl_gate_dropped": "dwl without the wl > 0 gate of the ReLU before the sigmoid",
    "dsmall_overwrites": "d_small of the blend backward overwritten where accumulate_small = 1",
    "pads_unwritten": "pad channels left as they were",
    "truncate": "truncation instead of round-to-nearest-even in the store",
    "segment_shifted": "the rows of every segment after the first shifted by one",
}
BLEND_MUTANTS = ("low_not_quarter", "wl_gate_dropped", "dsmall_overwrites", "pads_unwritten")      # measured by rel-L2: must miss by >= 100x


# ---------------------------------------------------------------------------------------------------------------- rounding, bounds
def rne(v, dtype, mut=()):
    """v (float64 holding an fp32 value) stored in the storage type: round to nearest even, as float64."""
    v32 = v.to(torch.float32)
    if dtype == "f32":
        return v32.to(F64)
    r = v32.to(TDT[dtype])
    if "truncate" in mut:      # sign-magnitude bits: one step towards zero wherever rounding went away from it
        away = (r.to(F64).abs() > v32.to(F64).abs()) & torch.isfinite(r.to(F64))
        r = torch.where(away, (r.view(torch.int16) - 1).view(TDT[dtype]), r)
    return r.to(F64)


def representable(v, dtype):
    return rne(v, dtype)


def r_T(ref, dtype):
    return torch.zeros_like(ref) if dtype == "f32" else CR.half_ulp(ref, dtype)


def sum_bound(ref, n, abs_sum, dtype):
    """r_T(ref) + (n - 1) * 2^-24 * sum |terms| per element."""
    return r_T(ref, dtype) + (n.to(F64) - 1).clamp_min(0) * U * abs_sum


def exact_in_fp32(ref, abs_sum, dtype):
    """The condition of the bit-equal gate of an integer-valued case: integers, every partial sum of every order below 2^24, result storable."""
    return bool((ref == ref.round()).all()) and float(abs_sum.max()) < 2.0 ** 24 and torch.equal(rne(ref, dtype), ref)


def worst_ratio(got, ref, bound):
    return CR.worst_ratio(got.to(F64), ref, bound)


def rel_l2(a, b):
    return float((a.to(F64) - b).norm() / b.norm().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------- max pooling (TF SAME)
def same_pad(size, k, s, mut=()):
    """(outputs, padding before): out = ceil(size / s), the odd cell goes AFTER the image."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, (total - total // 2 if "pad_before" in mut else total // 2)


def maxpool_fwd(x, pool, stride, relu_mask, mut=()):
    """y and the argmax-code plane (int64, values 0 .. pool^2 - 1 or 255).  Code a * pool + b in window coordinates, padded cells included in the
    numbering; the first maximum in row-major order over the cells inside the image wins; 255 where relu_mask and the maximum is not > 0."""
    B, H, W, C = x.shape
    OH, pby = same_pad(H, pool, stride, mut)
    OW, pbx = same_pad(W, pool, stride, mut)
    y = torch.full((B, OH, OW, C), float("-inf"), dtype=x.dtype)
    codes = torch.zeros((B, OH, OW, C), dtype=torch.int64)
    for oy in range(OH):
        for ox in range(OW):
            best, arg = y[:, oy, ox], codes[:, oy, ox]      # views
            for a in range(pool):
                for b in range(pool):
                    sy, sx = oy * stride + a - pby, ox * stride + b - pbx
                    if 0 <= sy < H and 0 <= sx < W:
                        v = x[:, sy, sx]
                    elif "padded_cells_win" in mut:
                        v = torch.zeros_like(best)
                    else:
                        continue
                    take = (v >= best) if "last_max_wins" in mut else (v > best)
                    arg[take] = a * pool + b
                    best[take] = v[take]
    if relu_mask and "relu_mask_ignored" not in mut:
        codes[~(y > 0)] = 255
    return y, codes


def maxpool_bwd(dy, codes, shape, pool, stride, mask=None, old=None, dtype="f32", mut=(), eval_dtype=F64):
    """dx, its bound and sum |terms|: dy scattered by the codes, masked by (mask > 0), then added to `old`.  eval_dtype=torch.float32: the same sums in fp32."""
    B, H, W, C = shape
    OH, pby = same_pad(H, pool, stride)
    OW, pbx = same_pad(W, pool, stride)
    g = torch.zeros(shape, dtype=eval_dtype)
    gabs = torch.zeros(shape, dtype=F64)
    n = torch.zeros(shape, dtype=torch.int64)
    dye = dy.to(eval_dtype)

    def add(oy, ox, k, sy, sx):
        hit = codes[:, oy, ox] == k
        g[:, sy, sx] += torch.where(hit, dye[:, oy, ox], torch.zeros_like(dye[:, oy, ox]))
        gabs[:, sy, sx] += torch.where(hit, dy[:, oy, ox].abs(), torch.zeros_like(dy[:, oy, ox]))
        n[:, sy, sx] += hit.to(torch.int64)

    for oy in range(OH):
        for ox in range(OW):
            for k in range(pool * pool):
                a, b = divmod(k, pool)
                if "offset2_as_1" in mut:
                    a, b = (1 if a == 2 else a), (1 if b == 2 else b)
                sy, sx = oy * stride + a - pby, ox * stride + b - pbx
                if 0 <= sy < H and 0 <= sx < W:
                    add(oy, ox, k, sy, sx)
    if "out_of_image_window" in mut:      # the windows one step outside the output grid that would cover an image pixel, read at window (0, 0)
        for oy in range(-1, OH + 1):
            for ox in range(-1, OW + 1):
                if 0 <= oy < OH and 0 <= ox < OW:
                    continue
                for k in range(pool * pool):
                    a, b = divmod(k, pool)
                    sy, sx = oy * stride + a - pby, ox * stride + b - pbx
                    if 0 <= sy < H and 0 <= sx < W:
                        add(0, 0, k, sy, sx)
    return _mask_and_accumulate(g, gabs, n, mask, old, dtype, mut)


def _mask_and_accumulate(g, gabs, n, mask, old, dtype, mut):
    """mask first (where mask > 0), then + old; returns (value in float64, bound, sum |terms|)."""
    if "accumulate_dropped" in mut:
        old = None
    if mask is not None and "mask_after_accumulate" not in mut:
        keep = mask > 0
        g, gabs, n = torch.where(keep, g, torch.zeros_like(g)), torch.where(keep, gabs, torch.zeros_like(gabs)), torch.where(keep, n, torch.zeros_like(n))
    if old is not None:
        g, gabs, n = g + old.to(g.dtype), gabs + old.abs(), n + 1
    if mask is not None and "mask_after_accumulate" in mut:
        g = torch.where(mask > 0, g, torch.zeros_like(g))
    g = g.to(F64)
    return g, sum_bound(g, n, gabs, dtype), gabs


# ---------------------------------------------------------------------------------------------------------------- executor helpers
def masked_add(src, mask=None, old=None, dtype="f32", mut=(), eval_dtype=F64):
    """dst = (mask > 0 ? src : 0) (+ old): value, bound, sum |terms|."""
    return _mask_and_accumulate(src.to(eval_dtype), src.abs(), torch.ones(src.shape, dtype=torch.int64), mask, old, dtype, mut)


def zero_stuff(x, mut=()):
    """y[b, 2i + 1, 2j + 1] = x[b, i, j], exactly +0 elsewhere: the input grid conv2d_transpose_s2 correlates its flipped kernel with."""
    B, H, W, C = x.shape
    y = torch.zeros((B, 2 * H, 2 * W, C), dtype=x.dtype)
    o = 0 if "stuffed_even" in mut else 1
    y[:, o::2, o::2] = x
    return y


def zero_unstuff(dy, mask=None, old=None, dtype="f32", mut=(), eval_dtype=F64):
    """dx[b, i, j] = (mask > 0 ? dy[b, 2i + 1, 2j + 1] : 0) (+ old): value, bound, sum |terms|."""
    o = 0 if "stuffed_even" in mut else 1
    return masked_add(dy[:, o::2, o::2], mask, old, dtype, mut, eval_dtype)


def space_to_depth2(y, C, cp, mut=()):
    """s[b, i, j, (py * 2 + px) * cp + c] = y[b, 2i + py, 2j + px, c] for c < C, +0 for C <= c < cp.  y: [B, 2H, 2W, >= C]."""
    B, H2, W2, _ = y.shape
    s = torch.full((B, H2 // 2, W2 // 2, 4 * cp), SENTINEL if "pads_unwritten" in mut else 0.0, dtype=y.dtype)
    for py in range(2):
        for px in range(2):
            plane = px * 2 + py if "parity_swapped" in mut else py * 2 + px
            s[..., plane * cp:plane * cp + C] = y[:, py::2, px::2, :C]
    return s


def convert_channels(src, nch, dst_pad, dst_dtype, mut=()):
    """[npix, max(nch, dst_pad)]: the first nch channels of src stored in dst_dtype, +0 up to dst_pad."""
    d = torch.full((src.shape[0], max(nch, dst_pad)), SENTINEL if "pads_unwritten" in mut else 0.0, dtype=F64)
    d[:, :nch] = rne(src[:, :nch], dst_dtype, mut)
    return d


# ---------------------------------------------------------------------------------------------------------------- layer-wise compose path
def upsample2(x):
    """out[b, y, x] = in[b, y // 2, x // 2] (nearest neighbour, MultiScalePrediction.py:16-33)."""
    B, h, w, C = x.shape
    out = torch.empty((B, 2 * h, 2 * w, C), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            out[:, py::2, px::2] = x
    return out


def block_sum(x):
    """Sum over the 2 x 2 blocks: [B, H, W, C] -> [B, H/2, W/2, C] (value, sum of magnitudes)."""
    parts = [x[:, py::2, px::2] for py in range(2) for px in range(2)]
    return parts[0] + parts[1] + parts[2] + parts[3], parts[0].abs() + parts[1].abs() + parts[2].abs() + parts[3].abs()


def compose_pack(small, fine, c_pad, dtype, mut=()):
    """[B, H, W, c_pad] in the storage type: channels 0-2 small at (y / 2, x / 2), 3-5 fine, +0 up to c_pad."""
    B, H, W, _ = fine.shape
    if "x_not_halved" in mut:      # the linear address ((b * H/2 + y/2) * W/2 + x) of a kernel that forgot the division, inside the allocation
        flat = small[..., :3].reshape(-1, 3)
        b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
        up = flat[((b * (H // 2) + y // 2) * (W // 2) + x) % flat.shape[0]]
    else:
        up = upsample2(small[..., :3])
    out = torch.full((B, H, W, c_pad), SENTINEL if "pads_unwritten" in mut else 0.0, dtype=F64)
    out[..., 0:3] = rne(up, dtype, mut)
    out[..., 3:6] = rne(fine[..., :3], dtype, mut)
    return out


def _low(fine, mut, dt):
    s, _ = block_sum(fine.to(dt))
    return upsample2(s if "low_not_quarter" in mut else s * 0.25)


def compose_blend_fwd(small, fine, wl, mut=(), eval_dtype=F64):
    """out = fine - w * low + w * up(small), w = sigmoid(wl), low = up(2 x 2 mean of fine) (MultiScalePrediction.compose_scales :36-54)."""
    f, w = fine.to(eval_dtype), torch.sigmoid(wl.to(eval_dtype))
    return (f - w * _low(fine, mut, eval_dtype) + w * upsample2(small.to(eval_dtype))).to(F64)


def compose_blend_bwd(dout, small, fine, wl, d_small_old, accumulate_small, dw_pad, dtype, mut=(), eval_dtype=F64, one_minus_w="e*w"):
    """(d_small, d_fine, dwl [B, H, W, max(dw_pad, 1)] in the storage type).  wl is a ReLU output: dwl carries that ReLU's gate (wl > 0).
    one_minus_w: how 1 - sigmoid(wl) is formed, "e*w" (e = exp(-wl), e / (1 + e)) or "1-w" (the subtraction, which cancels in fp32 for a large
    wl); in float64 the two agree to 1e-13."""
    g, s = dout.to(eval_dtype), upsample2(small.to(eval_dtype))
    wlv = wl.to(eval_dtype)
    e = torch.exp(-wlv)
    w = 1.0 / (1.0 + e)
    tsum, _ = block_sum(w * g)
    d_small = tsum + (d_small_old.to(eval_dtype) if accumulate_small and "dsmall_overwrites" not in mut else 0.0)
    d_fine = g - 0.25 * upsample2(tsum)
    dw = ((g * (s - _low(fine, mut, eval_dtype))).sum(dim=3, keepdim=True)) * w * (e * w if one_minus_w == "e*w" else 1.0 - w)
    if "wl_gate_dropped" not in mut:
        dw = torch.where(wlv > 0, dw, torch.zeros_like(dw))
    dwl = torch.full(tuple(dw.shape[:3]) + (max(dw_pad, 1),), SENTINEL if "pads_unwritten" in mut else 0.0, dtype=F64)
    dwl[..., :1] = rne(dw.to(F64), dtype, mut)
    return d_small.to(F64), d_fine.to(F64), dwl


def compose_unpack_bwd(dnet, d_small_old, d_fine_old, mut=(), eval_dtype=F64):
    """d_small += the 2 x 2 block sums of dnet[..., 0:3], d_fine += dnet[..., 3:6] (fp32 outputs): (value, bound, sum |terms|) of each."""
    if "accumulate_dropped" in mut:
        d_small_old, d_fine_old = torch.zeros_like(d_small_old), torch.zeros_like(d_fine_old)
    s, _ = block_sum(dnet[..., 0:3].to(eval_dtype))
    _, sabs = block_sum(dnet[..., 0:3])
    ds = (s + d_small_old.to(eval_dtype)).to(F64)
    df = (dnet[..., 3:6].to(eval_dtype) + d_fine_old.to(eval_dtype)).to(F64)
    five, two = torch.full(ds.shape, 5), torch.full(df.shape, 2)
    sabs, fabs = sabs + d_small_old.abs(), dnet[..., 3:6].abs() + d_fine_old.abs()
    return (ds, sum_bound(ds, five, sabs, "f32"), sabs), (df, sum_bound(df, two, fabs, "f32"), fabs)


# ---------------------------------------------------------------------------------------------------------------- column sums
def colsum(x, out_old, eval_dtype=F64):
    """out[ch] = old[ch] + sum over the rows of x[row, ch]; also sum |terms| (the exactness condition of the integer cases)."""
    return (out_old.to(eval_dtype) + x.to(eval_dtype).sum(0)).to(F64), out_old.abs() + x.abs().sum(0)


def colsum_segments(x, rows, out_row, out_old, mut=(), eval_dtype=F64):
    """out[out_row[s]] += the column sums of rows [s * rows, (s + 1) * rows) of x, segment by segment."""
    out, oabs = out_old.to(eval_dtype).clone(), out_old.abs().clone()
    for s, r in enumerate(out_row):
        lo = s * rows + (1 if "segment_shifted" in mut and s > 0 else 0)
        seg = x[lo:lo + rows]
        out[r] += seg.to(eval_dtype).sum(0)
        oabs[r] += seg.abs().sum(0)
    return out.to(F64), oabs


# ---------------------------------------------------------------------------------------------------------------- tiles
def extract_tiles(frame, origins, ts):
    """tiles[t] = frame[oy : oy + ts, ox : ox + ts] (Prediction.py:396-427)."""
    return torch.stack([frame[oy:oy + ts, ox:ox + ts] for oy, ox in origins])


def stitch(tiles, entries, frame_old):
    """Every entry (tile, crop_y0, crop_y1, crop_x0, crop_x1, dst_img, dst_y, dst_x) copies its crop window into frame_old[dst_img]."""
    frame = frame_old.clone()
    for t, y0, y1, x0, x1, img, dy, dx in entries:
        frame[img, dy:dy + (y1 - y0), dx:dx + (x1 - x0)] = tiles[t, y0:y1, x0:x1]
    return frame


# ---------------------------------------------------------------------------------------------------------------- inputs and case tables
def _gen(*key):
    """A generator seeded by a tuple of integers (the same on every machine)."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, *key):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(*key)).to(F64)


def reals(shape, dtype, *key, scale=1.0):
    return representable(torch.randn(tuple(shape), generator=_gen(*key), dtype=F64) * scale, dtype)


# (pool, stride, H, W): the stride-2 rows take maxpool_bwd_s2_kernel<POOL>, the last three the generic backward (stride 1: up to 9 windows a pixel)
POOL_GEOMETRIES = [(3, 2, 8, 8), (3, 2, 7, 9), (3, 2, 1, 1), (3, 2, 1, 6), (3, 2, 2, 1), (2, 2, 6, 8), (2, 2, 5, 7), (2, 2, 1, 1),
                   (3, 3, 7, 8), (3, 1, 5, 6), (2, 1, 4, 5)]
POOL_B = 2
POOL_C = {"f32": 12, "bf16": 24, "f16": 24}
# (B, C, ld - C): B in {1, 2}, the two channel counts and the two row lengths; the operands of a smaller case are the leading images / channels
# of the full-size ones (pooling is independent per image and channel: so is the reference, which is computed once at full size)
POOL_BCL = {dt: [(B, C, extra) for B in (1, 2) for C in ((4, 12) if dt == "f32" else (8, 24)) for extra in (0, 8 if dt == "f32" else 16)] for dt in DTYPES}
POOL_MASKS = ("none", "input", "unrelated")
POOL_KINDS = ("int", "real")
# channels with a plane of their own in the integer inputs
CH_CONST, CH_ZERO, CH_NEG = 0, 1, 2


@functools.lru_cache(maxsize=None)
def pool_inputs(dtype, geometry, relu_mask, kind):
    """x, dy, old gradient, unrelated mask at full size (POOL_B images, POOL_C[dtype] channels), float64 holding storage-type values.
    int: x from {0 .. 3} (relu_mask) or {-3 .. 3}, channel 0 a constant plane, channel 1 all zero, channel 2 all negative (relu_mask = 0 only);
    dy and old from the integers of [-8, 8], dy of channels 1 and 2 never 0.  real: N(0, 1) rounded to the storage type, ReLU'd when relu_mask."""
    pool, stride, H, W = geometry
    B, C = POOL_B, POOL_C[dtype]
    OH, OW = same_pad(H, pool, stride)[0], same_pad(W, pool, stride)[0]
    key = (DTYPES.index(dtype), POOL_GEOMETRIES.index(geometry), relu_mask, POOL_KINDS.index(kind))
    if kind == "int":
        x = ints((B, H, W, C), 0 if relu_mask else -3, 3, 1, *key)
        x[..., CH_CONST] = 2.0
        x[..., CH_ZERO] = 0.0
        if not relu_mask:
            x[..., CH_NEG] = ints((B, H, W), -3, -1, 2, *key)
        dy, old, m = ints((B, OH, OW, C), -8, 8, 3, *key), ints((B, H, W, C), -8, 8, 4, *key), ints((B, H, W, C), -1, 1, 5, *key)
        for c in (CH_ZERO, CH_NEG):
            dy[..., c] = torch.where(dy[..., c] == 0, torch.ones_like(dy[..., c]), dy[..., c])
    else:
        x = reals((B, H, W, C), dtype, 1, *key)
        if relu_mask:
            x = torch.relu(x) + 0.0
        dy, old, m = reals((B, OH, OW, C), dtype, 3, *key), reals((B, H, W, C), dtype, 4, *key), reals((B, H, W, C), dtype, 5, *key)
    return x, dy, old, m


def pool_switches():
    """The 24 (relu_mask, mask, accumulate, kind) combinations every geometry runs with; the reference depends on nothing else."""
    return [dict(relu_mask=r, mask=m, acc=a, kind=k) for r in (0, 1) for m in POOL_MASKS for a in (0, 1) for k in POOL_KINDS]


def pool_cases(dtype, geometry):
    """Every switch combination with every (B, C, ld): 192 launches' worth per storage type and geometry."""
    return [dict(s, B=B, C=C, ld=C + extra) for s in pool_switches() for B, C, extra in POOL_BCL[dtype]]


def pool_reference(dtype, geometry, relu_mask, mask, acc, kind, mut=(), codes=None, eval_dtype=F64):
    """(y, codes, dx, dx bound, sum |terms| of dx) at full size; `codes`: scatter by these instead of the forward's own."""
    x, dy, old, m = pool_inputs(dtype, geometry, relu_mask, kind)
    pool, stride = geometry[:2]
    y, cd = _pool_fwd_cached(dtype, geometry, relu_mask, kind, tuple(sorted(mut)))
    mk = {"none": None, "input": x, "unrelated": m}[mask]
    dx, bound, gabs = maxpool_bwd(dy, cd if codes is None else codes, x.shape, pool, stride, mk, old if acc else None, dtype, mut, eval_dtype)
    return y, cd, dx, bound, gabs


@functools.lru_cache(maxsize=None)
def _pool_fwd_cached(dtype, geometry, relu_mask, kind, mut):
    x = pool_inputs(dtype, geometry, relu_mask, kind)[0]
    return maxpool_fwd(x, geometry[0], geometry[1], relu_mask, mut)


MASKED_ADD_C = (4, 12, 40)
MASKED_ADD_EXTRA = (0, 8, 24)
MASKED_ADD_NPIX = (1, 7, 257)


def masked_add_inputs(dtype, C, npix, kind):
    """src, mask, old as [1, 1, npix, C]."""
    key = (DTYPES.index(dtype), C, npix, POOL_KINDS.index(kind))
    shape = (1, 1, npix, C)
    if kind == "int":
        return ints(shape, -8, 8, 11, *key), ints(shape, -1, 1, 12, *key), ints(shape, -8, 8, 13, *key)
    return reals(shape, dtype, 11, *key), reals(shape, dtype, 12, *key), reals(shape, dtype, 13, *key)


STUFF_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 4, 1)]
STUFF_C = 8


def stuff_inputs(dtype, shape, kind):
    """x [B, H, W, C]; the stuffed gradient [B, 2H, 2W, C] whose three other parities hold the sentinel; mask and old on the coarse grid."""
    B, H, W = shape
    key = (DTYPES.index(dtype), STUFF_SHAPES.index(shape), POOL_KINDS.index(kind))
    mk = (lambda s, k: ints(s, -8, 8, k, *key)) if kind == "int" else (lambda s, k: reals(s, dtype, k, *key))
    x, g, old = mk((B, H, W, STUFF_C), 21), mk((B, H, W, STUFF_C), 22), mk((B, H, W, STUFF_C), 23)
    mask = ints((B, H, W, STUFF_C), -1, 1, 24, *key)
    dy = torch.full((B, 2 * H, 2 * W, STUFF_C), SENTINEL, dtype=F64)
    dy[:, 1::2, 1::2] = g
    return x, dy, mask, old


S2D_CHANNELS = [(4, 4), (5, 8), (16, 16), (22, 24)]
S2D_SHAPE = (2, 3, 5)      # coarse grid


def s2d_input(dtype, C):
    """[B, 2H, 2W, ceil4(C)]: the channels past C inside the last group of four are real values the kernel must zero."""
    B, H, W = S2D_SHAPE
    return reals((B, 2 * H, 2 * W, (C + 3) // 4 * 4), dtype, 31, DTYPES.index(dtype), C) + 0.0


CONVERT_NCH = (1, 3)
CONVERT_NPIX = 259


def convert_input(src_dtype, nch):
    """[npix, 3 * nch] logits rows: dd_convert_channels reads channel 3 j of it (program.py), values with more bits than bf16 / f16 keep."""
    v = torch.randn((CONVERT_NPIX, 9), generator=_gen(41, DTYPES.index(src_dtype), nch), dtype=F64) * 3.0
    v[0, :] = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 65504.0, -65504.0, 2.0 ** -20, 0.333251953125])      # ties of bf16, f16 range
    return representable(v, src_dtype)


COMPOSE_SHAPES = [(1, 2, 2), (2, 4, 6), (1, 6, 2), (2, 8, 10)]


def compose_inputs(dtype, shape, kind="real"):
    """small [N, H/2, W/2, 3], fine, dout, old d_fine [N, H, W, 3], old d_small (fp32 values), wl [N, H, W, 1] (storage type, >= 0, about half exact
    zeros, up to 8), dnet [N, H, W, 6] (storage type)."""
    N, H, W = shape
    key = (DTYPES.index(dtype), COMPOSE_SHAPES.index(shape), POOL_KINDS.index(kind))
    if kind == "int":
        mk = lambda s, k: ints(s, -8, 8, k, *key)
        dnet = ints((N, H, W, 6), -8, 8, 57, *key)
    else:
        mk = lambda s, k: reals(s, "f32", k, *key)
        dnet = reals((N, H, W, 6), dtype, 57, *key)
    small, fine, dout = mk((N, H // 2, W // 2, 3), 51), mk((N, H, W, 3), 52), mk((N, H, W, 3), 53)
    ds_old, df_old = mk((N, H // 2, W // 2, 3), 54), mk((N, H, W, 3), 55)
    wl = representable(torch.relu(torch.randn((N, H, W, 1), generator=_gen(56, *key), dtype=F64) * 3.0).clamp_max(8.0), dtype) + 0.0
    wl.view(-1)[0] = 0.0
    wl.view(-1)[-1] = 8.0
    return small, fine, dout, ds_old, df_old, wl, dnet


COLSUM_ROWS = (1, 3, 255, 1025, 4100)
# (dtype, c, ld, first channel, byte misalignment): dd_colsum must route the first group to colsum_segments_kernel, the second to colsum_kernel
COLSUM_VECTOR = [("bf16", 8, 8, 0, 0), ("f16", 24, 32, 8, 0), ("bf16", 64, 64, 0, 0), ("f16", 64, 80, 16, 0), ("f32", 4, 4, 0, 0), ("f32", 32, 40, 4, 0)]
COLSUM_LANE = [("bf16", 72, 72, 0, 0), ("f16", 100, 104, 0, 0), ("bf16", 100, 120, 8, 0), ("f32", 40, 40, 0, 0),
               ("bf16", 8, 16, 3, 0), ("f32", 4, 8, 1, 0),          # a view that does not start on a 16-byte vector
               ("bf16", 8, 12, 0, 0), ("f16", 24, 28, 0, 0), ("f32", 4, 6, 0, 0)]      # ld no whole number of vectors
# (dtype, c, ld, first channel, n_segments, rows per segment, out_row, out_ld)
COLSUM_SEGMENTS = [("bf16", 8, 16, 8, 1, 255, (0,), 8), ("f16", 24, 32, 0, 3, 33, (2, 0, 2), 27), ("f32", 5, 12, 4, 3, 1025, (1, 1, 0), 9),
                   ("bf16", 64, 64, 0, 64, 7, tuple((i * 7) % 9 for i in range(64)), 64), ("f32", 32, 32, 0, 64, 3, tuple(range(64)), 40)]


def colsum_input(dtype, rows, ld, kind, *key):
    return ints((rows, ld), -64, 64, 61, DTYPES.index(dtype), rows, ld, *key) if kind == "int" else reals((rows, ld), dtype, 61, DTYPES.index(dtype), rows, ld, *key)


def colsum_old(shape, *key):
    v = ints(shape, -9, 9, 62, *key)
    return torch.where(v == 0, torch.ones_like(v), v)


FRAME_H, FRAME_W, TILE = 37, 41, 16
# tile origins (y, x): even and odd columns, the last one flush with the frame's last row and column
TILE_ORIGINS = [(0, 0), (0, 16), (5, 7), (3, 24), (21, 1), (FRAME_H - TILE, FRAME_W - TILE)]
TILE_C = (1, 3, 4)
# (tile, crop_y0, crop_y1, crop_x0, crop_x1, dst_img, dst_y, dst_x): whole tiles, crops, crops of zero width on one side, an empty crop
STITCH_ENTRIES = [(0, 0, 16, 0, 16, 0, 0, 0), (1, 2, 16, 3, 16, 0, 2, 19), (2, 0, 9, 0, 7, 0, 21, 3), (3, 4, 4, 0, 16, 0, 30, 0),
                  (4, 0, 16, 5, 5, 0, 20, 20), (5, 1, 16, 2, 15, 0, FRAME_H - 15, FRAME_W - 13)]


def frame_input(C):
    return reals((FRAME_H, FRAME_W, C), "f32", 71, C)
