"""CPU checks of tests/conv_fwd_ref.py, the float64 reference, gates and expected routes of tests/test_gpu_conv_fwd_ops.py, on every input
those tests use (one case table, imported by both; dd_conv3x3_ks in modes 0 - 6):
  * the restated dispatch rules give, for every case, the route the case table names by hand -- with every switch on and under the two
    switched-off environments of tests/test_gpu_fallbacks.py;
  * the shifted-slice sums equal oracle/tf_ops.py (conv2d_same, conv2d_transpose_s2 and their autograd for the gather and weight-gradient
    forms) to 1e-12, and oracle/np_ops.py on the small cases;
  * an fp32 evaluation in three summation orders, rounded where the kernels round, stays within 1x the gate -- the worst ratio is printed;
  * the gate flags the mutants listed in test_the_gates_flag_every_mutant; those that change nothing on a shape are asserted equivalent there
    and printed.
No element of any output is left out of any comparison."""
import numpy as np
import torch

import conv_fwd_ref as F
from oracle import np_ops, tf_ops
from test_conv_bwd_ref import Tally, _close, _f32

F64 = torch.float64
ENV_PLAIN = {"DD_CONV_WS": "0", "DD_CONV_RW": "0", "DD_WGRAD_DMA": "0", "DD_CONV_PW": "0"}
ENV_NO12 = {"DD_CONV_RW12": "0", "DD_CONV_RW12_MASK": "0", "DD_CONV_RW8_MASK": "0", "DD_CONV_RW8": "0"}
SMALL = F.IGEMM_CASES                     # the 2 x 128 x 128 cases of the wide 1x1 kernels are kept apart: one summation order less
ALL_IGEMM = F.IGEMM_CASES + F.PW_CASES
ALL_WGRAD = F.WGRAD_CASES + F.WGRAD_PW_CASES


def _operands(c, dtype):
    x, w, bias, res, mask, old = F.igemm_inputs(c.id, dtype)
    return x, w, (bias if c.nbias is not None else None), (res if c.res else None), (mask if c.mask else None), (old if c.accum else None)


# ---------------------------------------------------------------------------------------------------------------- routes
def test_the_restated_dispatch_gives_the_route_each_case_names():
    for c in ALL_IGEMM:
        for dtype in c.dtypes:
            got = F.igemm_route(c, dtype, {})
            if F.is_f32(dtype):
                want = c.route if c.dtypes == F.F32SETS else "igemm_resident"      # (the mixed cases are small: their f32 weights are resident)
            else:
                want = c.route
            assert got == want, (c.name, dtype, got, want)
            if not F.is_f32(dtype):
                plain = F.igemm_route(c, dtype, ENV_PLAIN)
                assert plain in ("igemm_resident", "igemm_streamed"), (c.name, plain)
                no12 = F.igemm_route(c, dtype, ENV_NO12)
                if 64 < c.cin <= 96 and c.taps == 9 and not c.flags & F.DD_IN_RELU:
                    assert no12 == "rw_6_2", (c.name, no12)
                else:
                    assert no12 == (c.route if c.route in ("pw", "igemm_streamed") else "igemm_ws"), (c.name, no12)
    assert {F.igemm_route(c, d, {}) for c in ALL_IGEMM for d in c.dtypes} == {
        "igemm_resident", "igemm_streamed", "igemm_ws", "rw_6_2", "rw12", "rw12_mask", "rw12_res", "rw8_kc2", "rw8_kc4", "rw8_kc4_mask", "pw"}
    assert "igemm_streamed" in {F.igemm_route(c, d, ENV_PLAIN) for c in ALL_IGEMM for d in c.dtypes if not F.is_f32(d)}
    for c in ALL_WGRAD:
        for dtype in c.dtypes:
            assert F.wgrad_route(c, dtype, {}) == ("wgrad_reg" if F.is_f32(dtype) else c.route), (c.name, dtype)
            assert F.wgrad_route(c, dtype, ENV_PLAIN) == ("refused" if c.stack else "wgrad_reg"), (c.name, dtype)
    assert {F.wgrad_route(c, d, {}) for c in ALL_WGRAD for d in c.dtypes} == {"wgrad_dma", "wgrad_reg", "wgrad_pw", "wgrad_stacked"}
    for c in F.KS_CASES:
        assert F.ks_route(c, {}) == c.route and F.ks_route(c, ENV_PLAIN) == "ks" and F.ks_route(c, ENV_NO12) == c.route, c.name
    assert {c.route for c in F.KS_CASES} == {"ks", "ks_pw_taps"}
    for case in F.K6_CASES:
        assert F.ks6_route(case, {}) == case[7] and F.ks6_route(case, ENV_PLAIN) == "ks" and F.ks6_route(case, ENV_NO12) == case[7], case
    assert {case[7] for case in F.K6_CASES} == {"ks", "ks_pw_taps"}


# ---------------------------------------------------------------------------------------------------------------- tie to the oracle
def _oracle_conv(c, x, w, bias, res, mask, old):
    """The call through oracle/tf_ops.py, epilogue composed in plain torch."""
    xin = torch.relu(x) if c.flags & F.DD_IN_RELU else x
    n = c.n
    if c.flags & F.DD_PIXSHUF:
        co = n // 4
        k = w[0].reshape(2, 2, co, c.cin)                                  # K[a][b][co][ci] = w[0][(2a + b) co_n + co][ci]
        y = tf_ops.conv2d_transpose_s2(xin, k, None if bias is None else bias[:co])
        assert bias is None or c.nbias == co
    elif c.flags & F.DD_GATHER2X2:
        k = w.reshape(2, 2, n, c.cin).permute(0, 1, 3, 2).contiguous()   # K[a][b][co = k][ci = n]: x is the fine-grid output gradient
        z = torch.zeros(c.B, c.H, c.W, n, dtype=F64, requires_grad=True)
        (tf_ops.conv2d_transpose_s2(z, k) * xin).sum().backward()
        y = z.grad
    else:
        side = 3 if c.taps == 9 else 1
        k = w.reshape(side, side, n, c.cin).permute(0, 1, 3, 2).contiguous()      # HWIO
        b = None
        if bias is not None:
            b = torch.zeros(n, dtype=F64)
            b[:c.nbias] = bias[:c.nbias]
        y = tf_ops.conv2d_same(xin, k, b)
    if res is not None:
        y = y + res
    if c.flags & F.DD_OUT_RELU:
        y = torch.relu(y)
    if mask is not None:
        y = y * (mask > 0)
    return y + old if old is not None else y


def _tie_igemm(c, dtype):
    ref = F.igemm_reference(c.id, dtype)
    _close(ref["y"], _oracle_conv(c, *_operands(c, dtype)), "conv_fwd %s %s" % (c.name, dtype))
    assert bool((ref["S"] >= ref["sum"].abs() * (1 - 1e-12)).all())


def _tie_ks(c, dtype):
    """dd_conv3x3_ks mode 0: rows [n0, n0 + n) of the layer the oracle computes whole."""
    x, w, bias, mask, old = F.ks_inputs(c.id, dtype)
    rows = c.n0 + c.n
    k = w.reshape(3, 3, rows, c.cin).permute(0, 1, 3, 2).contiguous()
    b = F.bias_vector(bias, c.nbias, rows, 0) if c.nbias is not None and not c.grad else None
    y = tf_ops.conv2d_same(torch.relu(x) if c.flags & F.DD_IN_RELU else x, k, b)[..., c.n0:]
    y = torch.relu(y) if c.flags & F.DD_OUT_RELU else y
    y = y * (mask > 0) if c.mask else y
    y = y + old if c.accum else y
    _close(F.ks_reference(c.id, dtype)["y"], y, "conv_ks %s %s" % (c.name, dtype))


def _tie_kst(case, dtype):
    """Modes 1 .. 5: the oracle's 3x3 / stride-2 transposed conv, channels [n0, n0 + n)."""
    cin, n, n0, grid, relu, nbias = case
    x, k, bias = F.kst_inputs(case, dtype)
    y = tf_ops.conv2d_transpose_s2(x, k, F.bias_vector(bias, nbias, n0 + n, 0), relu=bool(relu))[..., n0:]
    _close(F.kst_reference(case, dtype)[0], y, "conv_ks_t %s %s" % (case, dtype))
    # ... and the image the kernel reads: tap (uy, ux) of the zero-stuffed form is K[2 - uy][2 - ux]
    img = F.convt3_image(k)
    assert torch.equal(img[0], k[2, 2]) and torch.equal(img[2], k[2, 0]) and torch.equal(img[4], k[1, 1]) and torch.equal(img[7], k[0, 1])


def _tie_k6(case, dtype):
    """Mode 6: the data gradient of the oracle's 3x3 / stride-2 transposed conv (autograd), input channels [n0, n0 + n), from the output
    gradient rearranged by parity and the block-sparse image -- with the mode's own epilogue composed in plain torch."""
    cp, n, n0, (B, H, W), flags, nbias, use_mask, _ = case
    dy, k, bias, mask, old, filler = F.k6_inputs(case, dtype)
    z = torch.zeros(B, H, W, n0 + n, dtype=F64, requires_grad=True)
    (tf_ops.conv2d_transpose_s2(z, k) * dy).sum().backward()
    y = z.grad[..., n0:]
    if nbias is not None:
        y = y + F.bias_vector(bias, nbias, n0 + n, 0)[n0:]
    y = torch.relu(y) if flags & F.DD_OUT_RELU else y
    y = y * (mask > 0) if use_mask else y
    y = y + old if flags & F.DD_ACCUM else y
    ref = F.k6_reference(case, dtype)
    _close(ref["y"], y, "conv_ks6 %s %s" % (case, dtype))
    assert ref["n"] == 9 * cp + (nbias is not None)
    # the blocks the GEMM route skips are zero: tap (dy, dx) meets plane (py, px) only for py <= 1 - dy and px <= 1 - dx
    img = F.mode6_image(k, filler)
    for t in range(4):
        for pl in range(4):
            if not ((pl >> 1) <= 1 - (t >> 1) and (pl & 1) <= 1 - (t & 1)):
                assert not bool(img[(1 + (t >> 1)) * 3 + 1 + (t & 1)][:, pl * cp:(pl + 1) * cp].any())
    assert bool((img[0] >= 3).all()) and bool((img[6] >= 3).all())      # the unread taps hold the filler


def _tie_wgrad(c, dtype):
    p, q = F.wgrad_inputs(c.id, dtype)
    ref = F.wgrad_reference(c.id, dtype)
    pin = torch.relu(p) if c.flags & F.DD_IN_RELU else p
    if c.flags & F.DD_GATHER2X2:      # conv2d_transpose: the layer input is Q, the fine-grid output gradient P; dK[a][b][co = m][ci = n]
        k = torch.zeros(2, 2, c.m, c.n, dtype=F64, requires_grad=True)
        b = torch.zeros(c.m, dtype=F64, requires_grad=True)
        (tf_ops.conv2d_transpose_s2(q, k, b) * pin).sum().backward()
        _close(ref["out"], k.grad.reshape(4, c.m, c.n), "wgrad %s %s" % (c.name, dtype))
        _close(ref["bias"], b.grad, "wgrad bias of P %s %s" % (c.name, dtype))
    else:
        side = 3 if c.taps == 9 else 1
        k = torch.zeros(side, side, c.m, c.n, dtype=F64, requires_grad=True)
        b = torch.zeros(c.n, dtype=F64, requires_grad=True)
        (tf_ops.conv2d_same(pin, k, b) * q).sum().backward()
        _close(ref["out"], k.grad.reshape(c.taps, c.m, c.n), "wgrad %s %s" % (c.name, dtype))
        if c.bias_mode == 1:
            _close(ref["bias"], b.grad, "wgrad bias %s %s" % (c.name, dtype))
    if c.stack:      # block j of the stacked form is the gradient of conv j alone: input = the prefix, output gradient = its own columns
        m0, width, blocks = c.stack
        for j in range(blocks):
            rows = m0 + j * width
            alone = F.wgrad(p[..., :rows], q[..., j * width:(j + 1) * width], 9, c.flags, c.bias_mode)
            _close(F.stacked_block(ref["out"], j, m0, width), alone["out"], "stacked block %d of %s" % (j, c.name))
            assert alone["out"].shape == (9, rows, width)


def test_reference_equals_the_oracle():
    """Every input set of every GPU case (the inputs are seeded per case and set)."""
    for c in ALL_IGEMM:
        for dtype in c.dtypes:
            _tie_igemm(c, dtype)
    # oracle/np_ops.py (literal loops) on the small grids: a 3x3, a 1x1 and the pixel shuffle
    for name in ("ws 3x3 16->16", "ws 1x1 24->4 nbias 1", "pixshuf 64->4x16"):
        c = F.IGEMM_BY_ID[name]
        x, w, bias, _, _, _ = _operands(c, "bf16")
        x, w = x[:1, :5, :7], w
        cc = F.IgemmCase(name, c.taps, c.cin, c.n, (1, 5, 7), c.flags & ~F.DD_OUT_RELU, c.nbias)
        ref = F.conv_fwd(x, w, bias, taps=c.taps, flags=cc.flags, nbias=c.nbias)["y"]
        if c.flags & F.DD_PIXSHUF:
            want = np_ops.conv2d_transpose_s2(x.numpy(), w[0].reshape(2, 2, c.n // 4, c.cin).numpy(), bias[:c.n // 4].numpy())
        else:
            side = 3 if c.taps == 9 else 1
            b = np.zeros(c.n)
            b[:c.nbias] = bias[:c.nbias].numpy()
            want = np_ops.conv2d_same(x.numpy(), w.reshape(side, side, c.n, c.cin).permute(0, 1, 3, 2).numpy(), b)
        _close(ref, torch.from_numpy(want), "np_ops %s" % name)
    for dtype in F.DTYPES2:
        for c in F.KS_CASES:
            _tie_ks(c, dtype)
        for case in F.KST_CASES:
            _tie_kst(case, dtype)
        for case in F.K6_CASES:
            _tie_k6(case, dtype)
    for c in ALL_WGRAD:
        for dtype in c.dtypes:
            _tie_wgrad(c, dtype)


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation
def _sum32(c, x, w, order):
    """The sum over taps and channels in fp32, in one of three orders; float32 [B, H, W, n]."""
    xin = (torch.relu(x) if c.flags & F.DD_IN_RELU else x).float()
    w32 = w.float()
    taps = list(range(c.taps))
    acc = None
    if order == "sequential":      # one product at a time, in tap and channel order
        for t in taps:
            xs = F.tap_input(xin, c.taps, c.flags, t)
            for k in range(c.cin):
                term = xs[..., k:k + 1] * w32[t][:, k]
                acc = term if acc is None else acc + term
        return acc
    step = 64 if order == "slices" else 32
    slices = list(range(0, c.cin, step))
    if order == "slices":          # per 64-channel K-slice, every tap of it, then the next slice
        for k0 in slices:
            for t in taps:
                part = F.tap_input(xin, c.taps, c.flags, t)[..., k0:k0 + step] @ w32[t][:, k0:k0 + step].T
                acc = part if acc is None else acc + part
        return acc
    parts = [F.tap_input(xin, c.taps, c.flags, t)[..., k0:k0 + step] @ w32[t][:, k0:k0 + step].T for t in reversed(taps) for k0 in reversed(slices)]
    while len(parts) > 1:          # 32-channel pieces, taps reversed, combined pairwise (a tree)
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _wgrad32(c, p, q, order, seed=0):
    """out and the Q column sums in fp32: one product ("matmul"), or per 16 x 16 tile partial sums combined in tile order / in a shuffled order
    (what atomics do)."""
    pin = (torch.relu(p) if c.flags & F.DD_IN_RELU else p).float()
    q32 = q.float()
    tiles = [(b, y, x) for b in range(c.B) for y in range(0, c.H, 16) for x in range(0, c.W, 16)]
    if order == "matmul":
        tiles = [None]
    elif order == "shuffled":
        tiles = [tiles[i] for i in torch.randperm(len(tiles), generator=torch.Generator().manual_seed(seed)).tolist()]
    out, bias = torch.zeros(c.taps, c.m, c.n), torch.zeros(c.n)
    for tile in tiles:
        qt = q32
        if tile is not None:
            b, y, x = tile
            qt = torch.zeros_like(q32)
            qt[b, y:y + 16, x:x + 16] = q32[b, y:y + 16, x:x + 16]
        q2 = qt.reshape(-1, c.n)
        part = torch.stack([F.tap_input(pin, c.taps, c.flags, t).reshape(-1, c.m).T @ q2 for t in range(c.taps)])
        out, bias = out + part, bias + q2.sum(0)
    return out, bias


def test_fp32_evaluation_stays_within_the_gate():
    worst = {}

    def note(key, got, ref, gate_t, what):
        w = F.worst_ratio(got, ref, gate_t)
        worst[key] = max(worst.get(key, 0.0), w)
        assert w <= 1.0, "%s: fp32 emulation at %.3f of the gate" % (what, w)

    for c in ALL_IGEMM:
        big = c in F.PW_CASES
        for dtype in c.dtypes:
            x, w, bias, res, mask, old = _operands(c, dtype)
            ref = F.igemm_reference(c.id, dtype)
            g = F.gate_y(ref, dtype, c.route)
            for order in ("slices", "tree") if big else ("sequential", "slices", "tree"):
                v = _sum32(c, x, w, order)
                if bias is not None:
                    v = F.bias_vector(bias, c.nbias, c.n, c.flags).float() + v      # the accumulators start from the bias
                if c.flags & F.DD_PIXSHUF:
                    v = F.pixshuf(v)
                got = F.emulate_y(v, res, mask, old, c.flags, dtype, c.route)
                note("igemm %-7s %s" % (dtype, order), got, ref["y"], g, "%s %s %s" % (c.name, dtype, order))
    for c in F.KS_CASES:
        for dtype in c.dtypes:
            x, w, bias, mask, old = F.ks_inputs(c.id, dtype)
            ref = F.ks_reference(c.id, dtype)
            g = F.gate_y(ref, dtype, "pw")
            for order in ("slices", "tree") if c.cin > 300 or c.n > 128 else ("sequential", "slices", "tree"):
                v = _sum32(c, x, w[:, c.n0:], order)
                if c.nbias is not None and not c.grad:
                    v = F.bias_vector(bias, c.nbias, c.n0 + c.n, 0)[c.n0:].float() + v
                got = F.emulate_y(v, None, mask if c.mask else None, old if c.accum else None, c.flags, dtype, "pw")
                note("ks %-7s %s" % (dtype, order), got, ref["y"], g, "ks %s %s %s" % (c.name, dtype, order))
    for case in F.K6_CASES:      # mode 6: the four taps in both orders, whole and in 64-channel slices (the GEMM route's units)
        cp, n, n0, grid, flags, nbias, use_mask, route = case
        for dtype in F.DTYPES2:
            dy, k, bias, mask, old, filler = F.k6_inputs(case, dtype)
            ref = F.k6_reference(case, dtype)
            x32, w32 = F.space_to_depth(dy).float(), F.mode6_image(k, filler).float()
            for taps, step in ((range(4), 4 * cp), (reversed(range(4)), 64), (range(4), 32)):
                v = torch.zeros(ref["y"].shape)
                for t in taps:
                    for k0 in range(0, 4 * cp, step):
                        v = v + F.shifted(x32, t >> 1, t & 1)[..., k0:k0 + step] @ w32[(1 + (t >> 1)) * 3 + 1 + (t & 1)][n0:n0 + n, k0:k0 + step].T
                if nbias is not None:
                    v = F.bias_vector(bias, nbias, n0 + n, 0)[n0:].float() + v
                got = F.emulate_y(v, None, mask if use_mask else None, old if flags & F.DD_ACCUM else None, flags, dtype, "pw")
                note("ks mode 6 %s" % dtype, got, ref["y"], F.gate_y(ref, dtype, "pw"), "ks6 %s %s" % (case, dtype))
    for case in F.KST_CASES:
        cin, n, n0, grid, relu, nbias = case
        for dtype in F.DTYPES2:
            x, k, bias = F.kst_inputs(case, dtype)
            ref, budget = F.kst_reference(case, dtype)
            x32, k32 = x.float(), k.float()
            for order in (range(9), reversed(range(9))):
                v = torch.zeros(ref.shape)
                for t in order:
                    a, b = t // 3, t % 3
                    v[:, a % 2::2, b % 2::2] += F.shifted(x32, -(a // 2), -(b // 2)) @ k32[a, b, n0:n0 + n].T
                v = F.bias_vector(bias, nbias, n0 + n, 0)[n0:].float() + v
                got = F.to_storage(torch.relu(v) if relu else v, dtype)
                note("ks modes 1-5 %s" % dtype, got, ref, F.gate_storage(ref, budget, dtype), "ks_t %s %s" % (case, dtype))
    for c in ALL_WGRAD:
        for dtype in c.dtypes:
            if c in F.WGRAD_PW_CASES and dtype != "bf16":
                continue
            p, q = F.wgrad_inputs(c.id, dtype)
            ref = F.wgrad_reference(c.id, dtype)
            for order in ("matmul", "tiles", "shuffled"):
                out, bias = _wgrad32(c, p, q, order)
                note("wgrad %-7s %s" % (dtype, order), out.double(), ref["out"], F.gate_f32(ref["out_budget"]), "%s %s %s" % (c.name, dtype, order))
                if c.bias_mode == 1:
                    note("wgrad bias %-7s %s" % (dtype, order), bias.double(), ref["bias"], F.gate_f32(ref["bias_budget"]), "%s %s bias" % (c.name, dtype))
            if c.bias_mode == 2:
                b32 = p.float().reshape(-1, c.m).sum(0)
                note("wgrad bias of P %s" % dtype, b32.double(), ref["bias"], F.gate_f32(ref["bias_budget"]), "%s %s bias of P" % (c.name, dtype))
    for key in sorted(worst):
        print("fp32 emulation, worst error / gate: %-32s %.3f" % (key, worst[key]))
    assert worst and max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- mutants
def _at(t, b, y, x):
    """t restricted to one pixel (zero elsewhere)."""
    o = torch.zeros_like(t)
    o[b, y, x] = t[b, y, x]
    return o


def _column(t, x):
    o = torch.zeros_like(t)
    o[:, :, x] = t[:, :, x]
    return o


def _row(t, y):
    o = torch.zeros_like(t)
    o[:, y] = t[:, y]
    return o


def test_the_gates_flag_every_mutant():
    tally = Tally()
    equivalent = {}

    def judge(mutant, c, dtype, mut, ref, g, rounder):
        if not tally.judge(mutant, "%s %s" % (c.name, dtype), mut, ref, g, rounder):
            equivalent.setdefault(mutant, []).append("%s %s" % (c.name, dtype))

    for c in SMALL:
        for dtype in c.dtypes:
            x, w, bias, res, mask, old = _operands(c, dtype)
            ref = F.igemm_reference(c.id, dtype)
            g = F.gate_y(ref, dtype)
            if F.is_f32(dtype):
                rounder = _f32
            else:
                rounder = lambda t, dtype=dtype: F.to_storage(t, dtype)      # noqa: E731
                rounder.dtype = dtype
            shuf = bool(c.flags & F.DD_PIXSHUF)
            nterms = ref["n"] - (1 if res is not None else 0)
            s0 = ref["S"] - (res.abs() if res is not None else 0)

            def finish(v, **kw):      # the sum v (GEMM-row grid, bias included) through the (possibly mutated) epilogue
                return F.epilogue(F.pixshuf(v) if shuf else v, s0, nterms, kw.pop("res", res), kw.pop("mask", mask), old, c.flags, **kw)["y"]

            b = F.bias_vector(bias, c.nbias, c.n, c.flags) if bias is not None else 0
            full = F.conv_sum(x, w, c.taps, c.flags)[0] + b

            def without(delta, where=None):
                return finish(full - (delta if where is None else where(delta)))

            B, H, W = c.B, c.H, c.W
            last = lambda t: _at(t, B - 1, H - 1, W - 1)      # noqa: E731
            # ---- taps, halos, channel groups
            if c.taps > 1:
                t = c.taps // 2 + 1
                judge("one tap dropped (at one pixel)", c, dtype, without(F.conv_sum(x, w, c.taps, c.flags, [t])[0], lambda d: _at(d, 0, 0, 0)), ref["y"], g, rounder)
            if c.taps == 9:
                left = F.conv_sum(x, w, 9, c.flags, [0, 3, 6])[0]      # the taps that read column x - 1
                up = F.conv_sum(x, w, 9, c.flags, [0, 1, 2])[0]
                if W > 1:
                    judge("halo column dropped at the image border", c, dtype, without(F.conv_sum(x, w, 9, c.flags, [2, 5, 8])[0], lambda d: _column(d, W - 2)), ref["y"], g, rounder)
                if H > 1:
                    judge("halo row dropped at the image border", c, dtype, without(up, lambda d: _row(d, 1)), ref["y"], g, rounder)
                if W > 16:
                    judge("halo column dropped at the tile border x = 16", c, dtype, without(left, lambda d: _column(d, 16)), ref["y"], g, rounder)
                if H > 16:
                    judge("halo row dropped at the tile border y = 16", c, dtype, without(up, lambda d: _row(d, 16)), ref["y"], g, rounder)
                # the last column / row computed from CLAMPED instead of zero input: the taps that look past the border see the border pixel
                xin = torch.relu(x) if c.flags & F.DD_IN_RELU else x
                extra_c = sum(xin @ w[t].T for t in (5,))      # (centre row, x + 1 -> the pixel itself)
                judge("last column from clamped instead of zero input", c, dtype, finish(full + _column(extra_c, W - 1)), ref["y"], g, rounder)
                extra_r = sum(xin @ w[t].T for t in (7,))
                judge("last row from clamped instead of zero input", c, dtype, finish(full + _row(extra_r, H - 1)), ref["y"], g, rounder)
            for width in (8, 16, 32, 64):
                if c.cin >= 2 * width or (c.cin > width and width >= 32):
                    k0 = (c.cin - 1) // width * width
                    judge("%d-channel K group dropped (at one pixel)" % width, c, dtype, without(F.conv_sum(x, w, c.taps, c.flags, None, k0, k0 + width)[0], last), ref["y"], g, rounder)
            if c.cin == 96 and c.taps == 9:
                judge("odd half-slab (channels 64..95) of one tap dropped (at one pixel)", c, dtype, without(F.conv_sum(x, w, 9, c.flags, [4], 64, 96)[0], last), ref["y"], g, rounder)
            # ---- bias
            if bias is not None:
                co = c.n // 4 if shuf else c.n
                shifted_b = torch.cat([bias[1:], bias[:1]])
                judge("bias shifted by one channel", c, dtype, finish(full - b + F.bias_vector(shifted_b, c.nbias, c.n, c.flags)), ref["y"], g, rounder)
                judge("bias applied for c >= nbias", c, dtype, finish(full - b + F.bias_vector(bias, co, c.n, c.flags)), ref["y"], g, rounder)
                if shuf:      # bias[n mod (n_pad / 4)] instead of bias[n mod cout]
                    idx = torch.arange(c.n) % (c.n_pad // 4)
                    bp = torch.where(idx < c.nbias, bias[idx.clamp_max(c.n - 1)], torch.zeros(c.n, dtype=F64))
                    judge("bias indexed over n_pad", c, dtype, finish(full - b + bp), ref["y"], g, rounder)
                elif c.n_pad > c.n:      # rows of the bias laid out with the padded count: channel n reads bias[n * n / n_pad] -- any wrong index will do
                    idx = (torch.arange(c.n) * c.n_pad // c.n).clamp_max(c.n - 1)
                    bp = torch.where(torch.arange(c.n) < c.nbias, bias[idx], torch.zeros(c.n, dtype=F64))
                    judge("bias indexed over n_pad", c, dtype, finish(full - b + bp), ref["y"], g, rounder)
            # ---- epilogue
            if res is not None and c.flags & F.DD_OUT_RELU:
                judge("residual added after the ReLU", c, dtype, finish(full, res_after_relu=True), ref["y"], g, rounder)
            if mask is not None:
                judge("mask >= 0 instead of > 0", c, dtype, finish(full, mask_ge=True), ref["y"], g, rounder)
                judge("mask taken from the neighbouring channel", c, dtype, finish(full, mask=torch.roll(mask, 1, 3)), ref["y"], g, rounder)
            if c.accum:
                judge("DD_ACCUM overwriting", c, dtype, finish(full, overwrite=True), ref["y"], g, rounder)
            if shuf:
                y = F.epilogue(F.pixshuf(full, swap=True), s0, nterms, res, mask, old, c.flags)["y"]
                judge("DD_PIXSHUF parities (a, b) swapped", c, dtype, y, ref["y"], g, rounder)
            if c.flags & F.DD_GATHER2X2:
                judge("DD_GATHER2X2 a / b swapped", c, dtype, finish(F.conv_sum(x, w[[0, 2, 1, 3]], 4, c.flags)[0] + b), ref["y"], g, rounder)

    for c in F.KS_CASES:
        if c.nbias is None or c.grad:
            continue
        for dtype in c.dtypes:
            x, w, bias, mask, old = F.ks_inputs(c.id, dtype)
            ref = F.ks_reference(c.id, dtype)
            rounder = lambda t, dtype=dtype: F.to_storage(t, dtype)      # noqa: E731
            rounder.dtype = dtype
            mut = F.conv_ks(x, w, bias, None, None, c.n0, c.n, c.flags, c.nbias, bias_from_zero=True)["y"]
            judge("ks: n0 ignored for the bias", c, dtype, mut, ref["y"], F.gate_y(ref, dtype, "pw"), rounder)

    class _Named:
        def __init__(self, name):
            self.name = name

    for case in F.KST_CASES:      # parity modes 2 <-> 3 swapped: plane (0, 1) from the taps of parity (1, 0) -- a = 1, b in {0, 2} -- and the other way round
        cin, n, n0, grid, relu, nbias = case
        for dtype in F.DTYPES2:
            ref, budget = F.kst_reference(case, dtype)
            x, k, bias = F.kst_inputs(case, dtype)
            bv = F.bias_vector(bias, nbias, n0 + n, 0)[n0:]
            p01 = sum(F.shifted(x, 0, -(b // 2)) @ k[1, b, n0:n0 + n].T for b in (0, 2)) + bv
            p10 = sum(F.shifted(x, -(a // 2), 0) @ k[a, 1, n0:n0 + n].T for a in (0, 2)) + bv
            mut = ref.clone()
            mut[:, 0::2, 1::2], mut[:, 1::2, 0::2] = (torch.relu(p01), torch.relu(p10)) if relu else (p01, p10)
            rounder = lambda t, dtype=dtype: F.to_storage(t, dtype)      # noqa: E731
            rounder.dtype = dtype
            judge("ks: parity modes 2 <-> 3 swapped", _Named("ks_t %s" % (case,)), dtype, mut, ref, F.gate_storage(ref, budget, dtype), rounder)

    for case in F.K6_CASES:      # mode 6: the row and column offsets exchanged; an unread image tap read in place of tap (0, 0)
        cp, n, n0, grid, flags, nbias, use_mask, route = case
        for dtype in F.DTYPES2:
            dy, k, bias, mask, old, filler = F.k6_inputs(case, dtype)
            ref = F.k6_reference(case, dtype)
            rounder = lambda t, dtype=dtype: F.to_storage(t, dtype)      # noqa: E731
            rounder.dtype = dtype
            args = (bias if nbias is not None else None, mask if use_mask else None, old if flags & F.DD_ACCUM else None, n0, n, flags, nbias)
            x, w = F.space_to_depth(dy), F.mode6_image(k, filler)
            judge("ks mode 6: row / column offsets exchanged", _Named("ks6 %s" % (case,)), dtype, F.conv_ks6(x, w, *args, swap_offsets=True)["y"], ref["y"],
                  F.gate_y(ref, dtype, "pw"), rounder)
            w0 = w.clone()
            w0[4] = w[0]
            judge("ks mode 6: image tap 0 read for tap 4", _Named("ks6 %s" % (case,)), dtype, F.conv_ks6(x, w0, *args)["y"], ref["y"], F.gate_y(ref, dtype, "pw"), rounder)

    for c in F.WGRAD_CASES:
        for dtype in c.dtypes:
            p, q = F.wgrad_inputs(c.id, dtype)
            ref = F.wgrad_reference(c.id, dtype)
            gw = F.gate_f32(ref["out_budget"])
            keep = torch.ones(c.B, c.H, c.W, 1, dtype=F64)
            keep[c.B - 1, c.H - 16 if c.H > 16 else 0:, c.W - 16 if c.W > 16 else 0:] = 0      # the last (ragged) 16 x 16 tile
            mut = F.wgrad(p, q, c.taps, c.flags, c.bias_mode, pixels=keep)
            judge("wgrad: one tile of pixels dropped", c, dtype, mut["out"], ref["out"], gw, _f32)
            if c.bias_mode == 1:
                judge("wgrad bias: one tile of pixels dropped", c, dtype, mut["bias"], ref["bias"], F.gate_f32(ref["bias_budget"]), _f32)
            if c.taps == 9:
                judge("wgrad: P and Q shifted by the opposite tap sign", c, dtype, ref["out"].flip(0), ref["out"], gw, _f32)
            if c.bias_mode and c.m == c.n:
                other = F.wgrad(p, q, c.taps, c.flags, 3 - c.bias_mode)
                judge("wgrad: bias_mode 1 <-> 2", c, dtype, other["bias"], ref["bias"], F.gate_f32(ref["bias_budget"]), _f32)
            if c.stack:
                m0, width, blocks = c.stack
                for j in range(1, blocks):
                    blk = F.stacked_block(ref["out"], j, m0, width)
                    bud = ref["out_budget"][:, :m0 + j * width, j * width:(j + 1) * width]
                    judge("stacked block j takes the prefix of block j - 1", c, dtype, F.stacked_block(ref["out"], j, m0, width, shift=1), blk, F.gate_f32(bud), _f32)

    for name in sorted(tally.applied):
        n, frac = tally.applied[name]
        print("mutant flagged in %3d cases (at least %.3f of the changed elements): %s" % (n, frac, name))
    for name in sorted(equivalent):
        print("mutant changes NO value (asserted equivalent) on %d cases: %s -- %s" % (len(equivalent[name]), name, "; ".join(equivalent[name][:4])))
    for name in sorted(tally.gaps):
        print("KNOWN GAP (rel-L2 only) in %d cases: %s" % (tally.gaps[name], name))
    print("elements moved by more than twice the gate whose stored value passes it (the mutant's own rounding): %d" % tally.in_band)
    expected = {"one tap dropped (at one pixel)", "halo column dropped at the image border", "halo row dropped at the image border",
                "halo column dropped at the tile border x = 16", "halo row dropped at the tile border y = 16",
                "last column from clamped instead of zero input", "last row from clamped instead of zero input",
                "8-channel K group dropped (at one pixel)", "16-channel K group dropped (at one pixel)", "32-channel K group dropped (at one pixel)",
                "64-channel K group dropped (at one pixel)", "odd half-slab (channels 64..95) of one tap dropped (at one pixel)",
                "bias shifted by one channel", "bias applied for c >= nbias", "bias indexed over n_pad", "residual added after the ReLU",
                "mask >= 0 instead of > 0", "mask taken from the neighbouring channel", "DD_ACCUM overwriting", "DD_PIXSHUF parities (a, b) swapped",
                "DD_GATHER2X2 a / b swapped", "wgrad: one tile of pixels dropped", "wgrad: P and Q shifted by the opposite tap sign",
                "stacked block j takes the prefix of block j - 1", "wgrad bias: one tile of pixels dropped", "ks: n0 ignored for the bias", "ks: parity modes 2 <-> 3 swapped", "wgrad: bias_mode 1 <-> 2",
                "ks mode 6: row / column offsets exchanged", "ks mode 6: image tap 0 read for tap 4"}
    assert expected <= set(tally.applied), expected - set(tally.applied)
