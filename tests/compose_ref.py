"""Inputs, float64 reference and per-element gates of the fused compose net (dd_compose_net_fwd / dd_compose_net_bwd), CPU and torch only.
Shared by tests/test_compose_ref.py (CPU: the gates are sound and sharp), tests/test_gpu_compose_ops.py and tests/test_gpu_ops.py.

THE CONTRACT OF THE TWO FORWARD KERNELS, as read from their code ("stream" = csrc/dd_compose_stream.hip, "tile" = csrc/dd_compose.hip):
  netin   the packed input [up(small) | fine | 0 0] rounded to the storage type T.  Channels 6 and 7 are written as +0 by both kernels (stream
          :283-288, the fine half's lanes store d[3] = d[4] = 0; tile :236-240, v.w = 0u of the 16-byte store).  Channels >= 8 of a wider row are
          not written.
  a1      = relu(round_T(netin_T . w_in_T + b_in)): the 1x1 layer reads the ROUNDED input (stream :277 pack2 of xin; tile :247) and rounded
          weights (stream :106 through Elem<T>::from_f32; tile :66), rounds once, ReLU on the packed bits (stream :292-293; tile :259-262).
  save_act[0..4] = a1, relu(r1), a2 (raw), relu(r3), a3 (stream :302-303, :375-376 for LAYER 0 and 2 -> act[1], act[3], :360-361 act[2] before
          the ReLU of :365, :385-389 act[4]; tile :271, :277, :283, :289, :329-333).
  relu(r1) = relu(round_T(conv3x3(a1_T, w1_T) + b1));  a2 = round_T(a1_T + conv3x3(relu(r1)_T, w2_T) + b2);  relu(r3) reads relu(a2_T) (stream:
          the producer stores relu(a2) beside the raw a2, :351-377; tile: RELU_IN on the operand, :122);  a3 = round_T(a2_T + conv(..) + b4).
          Every layer consumes the STORED-TYPE tensor of the layer before; residuals are the stored-type a1 / a2 (stream :223-235; tile :134-138).
  wl      = round_T(relu(a3_T . w_out_T + b_out)): a3 is rounded BEFORE the 24 -> 1 layer (stream :382-392, the packed a3 registers are the B
          operand; tile :322-328), the ReLU is applied to the fp32 value and then rounded (stream :393; tile :338).
  out     = fine - s * low + s * up(small), fp32, s = 1 / (1 + __expf(-wl_T)): the sigmoid reads the ROUNDED wl (stream :393-396; tile :338-339),
          low = 0.25 * the fp32 sum of the 2x2 block of fine (stream :400-404; tile :344).
  Zero padding is the IMAGE's: every stored tensor is forced to zero outside the image before the next layer reads it (stream :295-298,
  :353-356, :367-370; tile :142-143).
The one difference between the kernels that a reference can see is the BIAS: the tile kernel starts its accumulator from the fp32 bias (:109,
:119, :253, :300, :338), the streaming kernel multiplies the bias in as three storage-type terms hi + mid + lo times 1 (split3,
csrc/dd_compose_stream.h:107-112; stage_weights :93, :105, :106).  For bf16 the three terms carry 24 bits and the sum is the fp32 bias; for f16
the second and third term of a bias around 0.1 fall below 2^-14, where f16 steps by 2^-24: the sum is the bias rounded to a multiple of 2^-24
or so.  stage_reference(kernel="stream") therefore uses the split sum, stage_reference(kernel="tile") the fp32 bias; nothing else differs.

THE GATE of a stored stage:  |got - z| <= ulp_T(z) / 2 + E,  z the float64 value of the stage computed from the kernel's own stored input,
  E = n * 2^-24 * (sum |w_q x| + |b| + |res|) + |b| * 2^-24.
n is the number of terms of the longest fp32 addition chain of the layer -- the classical bound (n - 1) u sum |terms| of a sum of n terms in ANY
order, u = 2^-24:
  3x3 layers  226   stream: 14 K-steps of v_mfma_f32_32x32x16 (27 k-groups of 8 channels + the bias group, :120) = 224 products on top of the
                    residual in the accumulator = 225; tile: 7 K-chunks of v_mfma 16x16x32 = 224 products + the bias in the accumulator + the
                    residual added afterwards = 226
  6 -> 24     33    stream: one K-step of 16; tile: one K-chunk of 32 + the bias
  24 -> 1     33    stream: two K-steps of 16 (:391-392); tile: 8 products, 7 adds, two cross-lane adds and the bias (:334-338) = 11
The second term of E is the three-term bias split.  ulp_T steps by 2^-24 below 2^-14 for f16 (subnormals), by 2^-133 below 2^-126 for bf16.
ReLU commutes with the rounding (it is applied to the rounded bits), so the same gate holds against relu(z); where z < -E the stored element must
be exactly +0 (all 16 bits clear); elements with |z| <= E (the ReLU boundary) may be +0 or the tiny rounded value, both of which the same
inequality admits -- no element is excluded from a gate.

THE GATE of out:  |low - up(small)| * d_sigma + 4 * 2^-24 * (|fine| + s * avg|fine block| + s * |small|)  (a few fp32 ulps of the three terms;
avg|fine block| >= |low| also covers the three fp32 additions of the block sum).
  d_sigma = 2^-21.  Source: __expf(x) is __builtin_amdgcn_exp2f(log2(e) * x) (clang's __clang_hip_math.h, "float __expf(float __x)"), i.e.
  one fp32 multiply and v_exp_f32, whose accuracy the CDNA instruction set guide gives as 1 ULP; 1.f / x without fast-math is hipcc's correctly
  rounded fp32 division (OpenCL allows 2.5 ULP, taken here).  With wl >= 0 and e = exp(-wl) <= 1: |d e| <= e * 2^-24 * (2 + wl) <= 2 * 2^-24
  (1 ULP of the instruction + the rounded product in the exponent; e (2 + wl) falls from 2 at wl = 0), 1 + e rounds by <= 2^-24 (half an ulp
  in [1, 2)), so |d(1 + e)| <= 3 * 2^-24, |d s| <= 3 * 2^-24 / (1 + e)^2 + 2.5 ulp(s) <= 5.5 * 2^-24 < 2^-21 = d_sigma < 2^-16.
  Where wl == 0 the kernel's s is exactly 0.5 (v_exp_f32 of -0 is 1): the d_sigma term is dropped there.

THE BACKWARD REFERENCE (backward_reference) is the storage-emulating oracle.model.compose_scales under autograd, the kernel being fed the oracle's
own activations: no forward of ours in between, so no rounding flip of a stored activation can decorrelate the comparison."""
import torch
import torch.nn.functional as F

DTYPES = ("bf16", "f16")
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
PBITS = {"bf16": 8, "f16": 11}            # significand bits, the hidden one included
EMIN = {"bf16": -126, "f16": -14}         # exponent of the smallest normal number
FMAX = {"bf16": 3.3895313892515355e38, "f16": 65504.0}
U32 = 2.0 ** -24
D_SIGMA = 2.0 ** -21
N_TERMS = {"in": 33, "res": 226, "out": 33}
STAGES = ("netin", "a1", "r1", "a2", "r3", "a3", "wl", "out")
ACT_OF = {"a1": 0, "r1": 1, "a2": 2, "r3": 3, "a3": 4}      # index into save_act
RELU_STAGES = ("a1", "r1", "r3", "wl")

# (N, H, W) of the streaming forward cases; geometry at 256 compute units in tests/test_gpu_compose_ops.py and tests/test_compose_ref.py
FWD_SHAPES = [(1, 2, 2), (1, 18, 30), (2, 10, 50), (1, 20, 72), (1, 22, 126), (1, 8, 128), (1, 16, 130), (1, 6, 260), (1, 6, 390), (24, 22, 140),
              (260, 4, 8), (130, 6, 140)]
TILE_FWD_SHAPES = [(1, 2, 2), (1, 16, 16), (2, 20, 28), (1, 34, 18), (65, 32, 32)]
SMALL_SHAPES = [(1, 2, 2), (1, 18, 30), (2, 10, 50), (1, 20, 72), (1, 16, 130), (1, 6, 260)]      # what the CPU proof evaluates term by term
BWD_SHAPES = [(2, 16, 32), (1, 20, 72), (2, 36, 136), (1, 18, 200), (3, 64, 64)]                    # tests/test_gpu_ops.py, unchanged
BWD_NEW_SHAPES = [(260, 4, 8), (130, 6, 140), (1, 6, 260)]
TILE_BWD_SHAPES = [(2, 16, 32), (2, 20, 28), (1, 34, 18), (65, 32, 32)]
KINDS = ("normal", "tiny")
TINY = 2.0 ** -13       # the small-magnitude input kind: images and biases scaled so that f16 activations fall into the subnormal range


def shape_id(s):
    return "%dx%dx%d" % tuple(s)


# ---------------------------------------------------------------------------------------------------------------- number formats
def rnd(t, dtype):
    """fp32 -> storage type, round to nearest even (what v_cvt_pk_bf16_f32 / v_cvt_f16_f32 do); t is rounded to fp32 first, as the kernels'
    accumulators are fp32."""
    return t.float().to(TDT[dtype]).double()


def ulp(z, dtype):
    """The spacing of the storage type at |z| (float64 in, float64 out); the subnormal step below the smallest normal number."""
    _, e = torch.frexp(z.abs().double())
    e = torch.where(z == 0, torch.full_like(e, EMIN[dtype]), e - 1).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(z, dtype=torch.float64), e - (PBITS[dtype] - 1))


def split3(b, dtype):
    """The streaming kernel's bias: hi + mid + lo, each a storage-type number (csrc/dd_compose_stream.h split3)."""
    b = b.float()
    hi = b.to(TDT[dtype]).float()
    mid = (b - hi).to(TDT[dtype]).float()
    lo = (b - hi - mid).to(TDT[dtype]).float()
    return hi.double(), mid.double(), lo.double()


def bias_of(b, dtype, kernel):
    if kernel == "stream":
        hi, mid, lo = split3(b, dtype)
        return hi + mid + lo
    assert kernel == "tile", kernel
    return b.double()


# ---------------------------------------------------------------------------------------------------------------- inputs
def _glorot(g, shape):
    fan_in, fan_out = shape[0] * shape[1] * shape[2], shape[0] * shape[1] * shape[3]
    lim = (6.0 / (fan_in + fan_out)) ** 0.5
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * lim).float()


def compose_inputs(shape, dtype, seed=0, kind="normal"):
    """fp32 small [N, H/2, W/2, 3], fine and dout [N, H, W, 3]; the twelve fp32 masters in HWIO (glorot kernels, biases 0.1 * randn: away from
    zero, as after some training).  The weights depend on the seed alone, the images on seed and shape.  kind "tiny" scales images and biases by
    2^-13: every activation shrinks by that factor (the net is positively homogeneous up to wl) and lands in f16's subnormal range."""
    N, H, W = shape
    assert dtype in DTYPES and kind in KINDS
    g = torch.Generator().manual_seed(1000 + seed)
    c = TINY if kind == "tiny" else 1.0
    inp = {"shape": tuple(shape), "dtype": dtype, "kind": kind}
    inp["w_in"], inp["b_in"] = _glorot(g, (1, 1, 6, 24)), (torch.randn(24, generator=g, dtype=torch.float64) * 0.1 * c).float()
    inp["w_res"] = [_glorot(g, (3, 3, 24, 24)) for _ in range(4)]
    inp["b_res"] = [(torch.randn(24, generator=g, dtype=torch.float64) * 0.1 * c).float() for _ in range(4)]
    # (a1 >= 0 rides on the residual stream, so the 24 -> 1 layer's sum sits around +1.5 +- 0.43 for these weights: its bias centres it, or wl
    #  would be positive everywhere and a wrong ReLU in front of the sigmoid invisible; tests/test_compose_ref.py checks the 20 - 80 % condition)
    inp["w_out"], inp["b_out"] = _glorot(g, (1, 1, 24, 1)), (torch.randn(1, generator=g, dtype=torch.float64) * 0.1 * c - 1.45 * c).float()
    g = torch.Generator().manual_seed(2000 + seed + 7 * N + 131 * H + 17 * W)
    inp["small"] = (torch.randn(N, H // 2, W // 2, 3, generator=g, dtype=torch.float64) * 0.7 * c).float()
    inp["fine"] = (torch.randn(N, H, W, 3, generator=g, dtype=torch.float64) * 0.7 * c).float()
    inp["dout"] = torch.randn(N, H, W, 3, generator=g, dtype=torch.float64).float()
    return inp


# ---------------------------------------------------------------------------------------------------------------- the operations, float64
def up2(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def pool2(t):
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4)) * 0.25


def conv3(x, w):
    """TensorFlow SAME 3x3: y[b, y, x] = sum_{ky, kx} x[b, y + ky - 1, x + kx - 1] . w[ky, kx], zeros outside the image."""
    N, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = 0
    for ky in range(3):
        for kx in range(3):
            y = y + xp[:, ky:ky + H, kx:kx + W] @ w[ky, kx]
    return y


def _layer(x, w, b, res, n):
    """(z, E) of one layer: z = x * w + b + res in float64, E as in the module docstring.  x: the stored input, w: rounded weights as float64."""
    if w.shape[0] == 1:
        z, s = x @ w[0, 0], x.abs() @ w[0, 0].abs()
    else:
        z, s = conv3(x, w), conv3(x.abs(), w.abs())
    z, s = z + b, s + b.abs()
    if res is not None:
        z, s = z + res, s + res.abs()
    return z, n * U32 * s + b.abs() * U32


def netin_of(inp, dtype):
    x = torch.cat([up2(inp["small"].double()), inp["fine"].double()], dim=3)
    return torch.cat([x, torch.zeros(x.shape[:3] + (2,), dtype=torch.float64)], dim=3)


def out_of(inp, wl):
    """(z, gate) of out from the stored wl."""
    fine, small = inp["fine"].double(), up2(inp["small"].double())
    s = torch.sigmoid(wl.double())
    low, lowabs = up2(pool2(fine)), up2(pool2(fine.abs()))
    z = fine - s * low + s * small
    ds = torch.where(wl == 0, torch.zeros_like(s), torch.full_like(s, D_SIGMA))
    gate = (low - small).abs() * ds + 4 * U32 * (fine.abs() + s * lowabs + s * small.abs())
    return z, gate


def stage_reference(inp, got, kernel="stream"):
    """got: the tensors the kernel stored, float64 [N, H, W, C]: netin (8 channels), a1, r1 (= relu(r1)), a2, r3 (= relu(r3)), a3, wl.
    Returns {stage: {"z": unrounded float64 value (before the ReLU where the stage has one), "ref": what got is compared with, "gate", "E",
    "relu"}} for the eight stages; each from the kernel's own stored input of that stage."""
    dtype = inp["dtype"]
    q = lambda w: rnd(w, dtype)                                           # noqa: E731
    bias = lambda b: bias_of(b, dtype, kernel)                            # noqa: E731
    wr, br = [q(w) for w in inp["w_res"]], [bias(b) for b in inp["b_res"]]
    out = {}

    def put(name, z, E, relu):
        ref = torch.relu(z) if relu else z
        out[name] = {"z": z, "ref": ref, "E": E, "gate": ulp(ref, dtype) / 2 + E, "relu": relu}

    z = netin_of(inp, dtype)
    put("netin", z, torch.zeros_like(z), False)
    put("a1", *_layer(got["netin"][..., :6], q(inp["w_in"]), bias(inp["b_in"]), None, N_TERMS["in"]), True)
    put("r1", *_layer(got["a1"], wr[0], br[0], None, N_TERMS["res"]), True)
    put("a2", *_layer(got["r1"], wr[1], br[1], got["a1"], N_TERMS["res"]), False)
    put("r3", *_layer(torch.relu(got["a2"]), wr[2], br[2], None, N_TERMS["res"]), True)
    put("a3", *_layer(got["r3"], wr[3], br[3], got["a2"], N_TERMS["res"]), False)
    put("wl", *_layer(got["a3"], q(inp["w_out"]), bias(inp["b_out"]), None, N_TERMS["out"]), True)
    z, gate = out_of(inp, got["wl"])
    out["out"] = {"z": z, "ref": z, "E": gate, "gate": gate, "relu": False}
    return out


def stage_ratio(st, got):
    """error / gate per element; inf where a ReLU-masked element (z < -E) is not exactly +0."""
    r = (got.double() - st["ref"]).abs() / st["gate"]
    if st["relu"]:
        masked = st["z"] < -st["E"]
        bad = masked & ((got != 0) | torch.signbit(got))
        r = torch.where(bad, torch.full_like(r, float("inf")), r)
    return r


def boundary_fraction(st):
    """Share of elements at the ReLU boundary (|z| <= E): they may be +0 or the tiny rounded value."""
    return float((st["z"].abs() <= st["E"]).double().mean()) if st["relu"] else 0.0


def worst(inp, got, kernel="stream", stages=STAGES):
    ref = stage_reference(inp, got, kernel)
    return {s: float(stage_ratio(ref[s], got[s]).max()) for s in stages}


def within(worst_by_stage):
    """error / gate < 1 for every stage; netin, whose gate is the bare half ulp (E = 0), may reach 1: an fp32 input exactly half way between
    two storage-type numbers (one in 2^13 for f16) is a tie, and |got - z| <= ulp / 2 holds with equality."""
    return all((w <= 1.0) if s == "netin" else (w < 1.0) for s, w in worst_by_stage.items())


# ---------------------------------------------------------------------------------------------------------------- a restated kernel
# What a forward kernel stores, restated on the CPU: in float64 (order=None), or with every layer's terms added in fp32 in a chosen order;
# optionally with one mistake.  tests/test_compose_ref.py gates its output with stage_reference: the restatement passes, each mistake does not.
ORDERS = ("natural", "reversed", "random", "mfma16")
MISTAKES = ("tap_dropped", "taps_transposed", "frame_padding", "seam_left_zeroed", "seam_right_zeroed", "band_row_plus4", "bias_dropped",
            "bias_rounded", "weights_unrounded", "residual_after_relu", "residual_other_block", "rounded_twice", "nearest_up_off_by_one",
            "avg_pool_shifted", "sigmoid_of_conv", "small_fine_swapped", "blend_one_minus_w")


def relu0(x):
    """The kernels' ReLU on the stored bits (a signed 16-bit max with 0): negative numbers AND -0 become +0."""
    return torch.where(x > 0, x, torch.zeros_like(x))


def _sum32(terms, init, order, g):
    """fp32 sum of the list of fp32 tensors `terms` on top of `init` in the given order."""
    k = len(terms)
    if order == "mfma16":      # blocks of 16 terms summed on their own, then added to the accumulator (as a K-step of an MFMA may do)
        acc = init
        for i in range(0, k, 16):
            blk = terms[i]
            for t in terms[i + 1:i + 16]:
                blk = blk + t
            acc = acc + blk
        return acc
    idx = list(range(k))
    if order == "reversed":
        idx.reverse()
    elif order == "random":
        idx = torch.randperm(k, generator=g).tolist()
    acc = init
    for i in idx:
        acc = acc + terms[i]
    return acc


def _terms(x, w):
    """The fp32 products of a layer, one tensor [N, H, W, Co] per (tap, input channel)."""
    x, w = x.float(), w.float()
    if w.shape[0] == 1:
        return [x[..., ci:ci + 1] * w[0, 0, ci] for ci in range(w.shape[2])]
    N, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return [xp[:, ky:ky + H, kx:kx + W, ci:ci + 1] * w[ky, kx, ci] for ky in range(3) for kx in range(3) for ci in range(w.shape[2])]


def simulate(inp, kernel="stream", order=None, mistake=None, plan=None, layer=1):
    """The stored tensors of a forward launch, restated.  `mistake` (one of MISTAKES) is applied to 3x3 layer `layer` (0..3) where it concerns a
    3x3 layer; the seam / band mistakes need `plan` = the eight numbers of dd_compose_stream_plan."""
    dtype = inp["dtype"]
    assert mistake is None or mistake in MISTAKES, mistake
    g = torch.Generator().manual_seed(5)
    N, H, W = inp["shape"]

    def store(z):
        if mistake == "rounded_twice":
            other = "f16" if dtype == "bf16" else "bf16"
            return rnd(rnd(z, other), dtype)
        return rnd(z, dtype)

    def run(x, w, b, res, l3=None):
        """One layer: l3 = index of the 3x3 layer or None for a 1x1."""
        hit = l3 == layer
        wq = w.double() if mistake == "weights_unrounded" and hit else rnd(w, dtype)
        bs = list(split3(b, dtype)) if kernel == "stream" else [b.double()]
        if mistake == "bias_dropped" and hit:
            bs = [torch.zeros_like(bs[0])]
        if mistake == "bias_rounded" and hit:
            bs = [rnd(b, dtype)]
        if hit and mistake == "tap_dropped":
            wq = wq.clone()
            wq[0, 2] = 0
        if hit and mistake == "taps_transposed":
            wq = wq.transpose(0, 1).contiguous()
        if hit and mistake == "frame_padding":      # the halo is not zeroed: a border pixel reads what lies beyond (here: the opposite side)
            assert order is None
            xw = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="circular").permute(0, 2, 3, 1)
            return conv3(xw, wq)[:, 1:-1, 1:-1] + sum(bs) + (res if res is not None else 0)
        if hit and mistake in ("seam_left_zeroed", "seam_right_zeroed") and plan[3] > 1:
            x = x.clone()
            for s in range(1, plan[3]):
                col = s * plan[4] - (1 if mistake == "seam_left_zeroed" else 0)
                if col < W:
                    x[:, :, col] = 0
        if hit and mistake == "band_row_plus4" and plan[6] > 1:
            x = x.clone()
            for j in range(1, plan[6]):
                y0 = j * plan[5]
                if y0 + 3 < H:
                    x[:, y0 - 1] = x[:, y0 + 3]
        if order is None:
            z = (x @ wq[0, 0] if wq.shape[0] == 1 else conv3(x, wq)) + sum(bs)
            return z + res if res is not None else z
        terms = _terms(x, wq) + [bb.float().expand(x.shape[:3] + (wq.shape[3],)) for bb in bs]
        if res is not None and kernel == "tile":      # the tile kernel adds the residual after the products
            return (_sum32(terms, torch.zeros_like(terms[-1]), order, g) + res.float()).double()
        init = res.float() if res is not None else torch.zeros_like(terms[-1])
        if kernel == "tile":                           # ... and starts from the bias
            init, terms = terms[-1], terms[:-1]
        return _sum32(terms, init, order, g).double()

    small, fine = inp["small"].double(), inp["fine"].double()
    ups = up2(small)
    if mistake == "nearest_up_off_by_one":
        ups = torch.roll(ups, 1, dims=2)
    x = torch.cat([fine, ups] if mistake == "small_fine_swapped" else [ups, fine], dim=3)
    got = {"netin": torch.cat([rnd(x, dtype), torch.zeros(x.shape[:3] + (2,), dtype=torch.float64)], dim=3)}
    got["a1"] = relu0(store(run(got["netin"][..., :6], inp["w_in"], inp["b_in"], None)))
    got["r1"] = relu0(store(run(got["a1"], inp["w_res"][0], inp["b_res"][0], None, 0)))
    got["a2"] = store(run(got["r1"], inp["w_res"][1], inp["b_res"][1], got["a1"], 1))
    got["r3"] = relu0(store(run(relu0(got["a2"]), inp["w_res"][2], inp["b_res"][2], None, 2)))
    res = got["a2"]
    if mistake == "residual_after_relu":
        res = relu0(res)
    if mistake == "residual_other_block":      # a1 where a2 is due (the other direction cannot exist: a2 is not computed yet when a1 is due)
        res = got["a1"]
    got["a3"] = store(run(got["r3"], inp["w_res"][3], inp["b_res"][3], res, 3))
    pre = run(got["a3"], inp["w_out"], inp["b_out"], None)
    got["wl"] = store(relu0(pre))
    wl = got["wl"]
    if order is None:
        s = torch.sigmoid(rnd(pre, dtype) if mistake == "sigmoid_of_conv" else wl)
        pooled = pool2(torch.roll(fine, -1, dims=2)) if mistake == "avg_pool_shifted" else pool2(fine)
        low = up2(pooled)
        if mistake == "blend_one_minus_w":
            s = 1 - s
        got["out"] = (fine - s * low + s * up2(small)).float().double()
    else:      # fp32 throughout, two associations
        f32, s32 = fine.float(), up2(small).float()
        sg = 1.0 / (1.0 + torch.exp(-wl.float()))
        r = f32.reshape(N, H // 2, 2, W // 2, 2, 3)
        if order in ("natural", "mfma16"):
            low = up2(((r[:, :, 0, :, 0] + r[:, :, 0, :, 1]) + (r[:, :, 1, :, 0] + r[:, :, 1, :, 1])) * 0.25)
            got["out"] = (f32 - sg * low + sg * s32).double()
        else:
            low = up2((((r[:, :, 1, :, 1] + r[:, :, 0, :, 1]) + r[:, :, 1, :, 0]) + r[:, :, 0, :, 0]) * 0.25)
            got["out"] = ((f32 + sg * s32) - sg * low).double()
    return got


# ---------------------------------------------------------------------------------------------------------------- backward reference
LAYERS = ["s/conv2d"] + ["s/conv2d_%d" % i for i in range(1, 6)]
_BWD_CACHE = {}


def backward_reference(shape, dtype):
    """The teacher-forced reference of dd_compose_net_bwd: oracle.model.compose_scales with storage emulation under autograd.  Returns small, fine,
    gout (float64, fp32-representable), names (the variable names in creation order), vars {name: float64 master}, acts = [a1, relu(r1), a2,
    relu(r3), a3] and wl as the oracle stored them, grads = [d small, d fine, d var ...].  Computed once per (shape, dtype); do not modify."""
    key = (tuple(shape), dtype)
    if key in _BWD_CACHE:
        return _BWD_CACHE[key]
    from oracle import model as OM
    N, H, W = shape
    g = torch.Generator().manual_seed(11 + N + H + W)
    vs = OM.VarStore(torch.float64, seed=5, storage=dtype)
    vs.enter_scope("s")
    recorded = []
    conv2d = vs.conv2d

    def recording(*a, **k):
        y = conv2d(*a, **k)
        recorded.append(y)
        return y
    vs.conv2d = recording
    small = (torch.randn(N, H // 2, W // 2, 3, generator=g, dtype=torch.float64) * 0.7).float().double().requires_grad_(True)
    fine = (torch.randn(N, H, W, 3, generator=g, dtype=torch.float64) * 0.7).float().double().requires_grad_(True)
    gout = torch.randn(N, H, W, 3, generator=g, dtype=torch.float64).float().double()
    out = OM.compose_scales(vs, "s", small, fine)
    for name, v in vs.vars.items():      # glorot kernels, and biases away from zero (as after some training)
        if name.endswith("/bias"):
            with torch.no_grad():
                v.copy_(torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.1)
    recorded.clear()
    vs.enter_scope("s")
    out = OM.compose_scales(vs, "s", small, fine)
    names = list(vs.vars)
    grads = torch.autograd.grad((out * gout).sum(), [small, fine] + [vs.vars[n] for n in names])
    a1, r1, a2, r3, a3, wl = [t.detach() for t in recorded]
    ref = {"small": small.detach(), "fine": fine.detach(), "gout": gout, "names": names, "vars": {n: vs.vars[n].detach() for n in names},
           "acts": [a1, relu0(r1), a2, relu0(r3), a3], "wl": wl, "grads": [t.detach() for t in grads]}
    _BWD_CACHE[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------- launch geometry
PLAN_KEYS = ("FW", "R", "TPR", "strips", "SO", "BH", "nb", "VB")


def plan(lib, shape, cus=256):
    """dd_compose_stream_plan (host only) of an (N, H, W) launch on `cus` compute units."""
    import ctypes
    o = (ctypes.c_int * 8)()
    assert lib.dd_compose_stream_plan(shape[0], shape[1], shape[2], cus, o) == 0
    return list(o)


def coverage_lost(rows, cus):
    """The coverage properties the shape list must keep on a device with `cus` compute units; returns the names of the lost ones."""
    P = list(rows.items())
    units = lambda s, p: s[0] * p["strips"] * p["nb"]                      # noqa: E731
    have = {
        "FW 32, 64, 96, 128": {p["FW"] for _, p in P} >= {32, 64, 96, 128},
        "R 1, 2, 4": {p["R"] for _, p in P} >= {1, 2, 4},
        "strips 1, 2, 3, >= 4": {min(p["strips"], 4) for _, p in P} >= {1, 2, 3, 4},
        "a last strip narrower than SO": any(p["strips"] > 1 and s[2] - (p["strips"] - 1) * p["SO"] < p["SO"] for s, p in P),
        "nb > 1 with H % BH != 0": any(p["nb"] > 1 and s[1] % p["BH"] for s, p in P),
        "BH > 4": any(p["BH"] > 4 for _, p in P),
        "two shapes with units > CUs": sum(units(s, p) > cus for s, p in P) >= 2,
    }
    return [k for k, v in have.items() if not v]
