"""-m gpu: dd_conv_igemm, dd_conv_wgrad and dd_conv3x3_ks (modes 0 - 6) op by op through the C-ABI -- every kernel they route a call to (conv_igemm_kernel resident and
streamed, conv_igemm_ws_kernel, the register-weight family of csrc/dd_conv_rw.hip, conv_pw_kernel; wgrad_dma_kernel plain and stacked,
wgrad_kernel, wgrad_pw_kernel; conv_ks_kernel and its nine-tap GEMM route) -- against the float64 reference and error budget of tests/conv_fwd_ref.py.  No Graph is built: every argument
struct is filled by hand.

WHICH KERNEL RAN is asserted, not assumed: every case computes the route it must take from the dispatch rules restated in conv_fwd_ref.py
(under the switches of THIS process: tests/test_gpu_fallbacks.py runs the file again with routes switched off) and checks that exactly that
dd_conv_route_count counter moved, by one.

THE GATE is elementwise on every element of every output: 2 * n * u * S for fp32 outputs, plus half a storage ulp per rounding of the path for
storage-type outputs (conv_fwd_ref.py lists the roundings per route).  The worst error / gate is printed and recorded (gpu_util.gate, bound
1); the rel-L2 gates of gpu_util (ROUND / ACC32) stay next to it.  tests/test_conv_fwd_ref.py shows on the CPU, for these very inputs, that
an fp32 evaluation stays within the gate and that dropped taps, halos, channel groups, wrong bias indices, epilogue slips and swapped
parities do not.

Every operand is a channel view at a non-zero, legally aligned channel offset inside a wider buffer whose other channels hold a sentinel; fp32
outputs sit between guard words.  Inputs, residuals, masks, biases and weight images must be bit-unchanged after the launch, neighbours and
guards intact.  Pad channels of y: the 2-byte implicit-GEMM kernels store whole 8-channel vectors that START below n, so channels n .. the next
multiple of 8 are written -- with the epilogue of a zero sum (0, or what was there under DD_ACCUM); every other kernel stores 4-channel groups
below n and nothing else."""
import ctypes as C
import os

import pytest
import torch

import conv_fwd_ref as F
import conv_ops_util as U
from deepdenoiser_amd import _lib as L
from gpu_util import ACC32, ROUND, check

pytestmark = pytest.mark.gpu
SENTINEL, G, View, Guarded = U.SENTINEL, U.G, U.View, U.Guarded
PAD_OLD = 0.5
SWITCHES = ("DD_CONV_WS", "DD_CONV_RW", "DD_CONV_RW8", "DD_CONV_RW8_MASK", "DD_CONV_RW12", "DD_CONV_RW12_MASK", "DD_CONV_PW", "DD_WGRAD_DMA", "DD_WGRAD_PW_MID")
ENV = {k: os.environ[k] for k in SWITCHES if k in os.environ}      # libdd_hip.so reads each switch once per process, from the same environment
TOLKEY = {"bf16": "bf16", "f16": "f16", "f32": "f32", "f32full": "f32"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _params(cases):
    return [pytest.param(c, d, id="%s-%s" % (c.name.replace(" ", "_"), d)) for c in cases for d in c.dtypes]


class Routes:
    """with Routes(route): ... -- exactly that counter moves, by one (route None: none moves)."""

    def __init__(self, route, what):
        self.route, self.what = route, what

    def __enter__(self):
        self.before = L.route_counts()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            after = L.route_counts()
            moved = {k: after[k] - self.before[k] for k in after if after[k] != self.before[k]}
            assert moved == ({self.route: 1} if self.route else {}), "%s: expected route %s, counters moved: %s" % (self.what, self.route, moved)
        return False


# ---------------------------------------------------------------------------------------------------------------- dd_conv_igemm
def _igemm(lib, c, dtype):
    x, w, bias, res, mask, old = F.igemm_inputs(c.id, dtype)
    ref = F.igemm_reference(c.id, dtype)
    route = F.igemm_route(c, dtype, ENV)
    name = "conv_igemm [%s] %s %s" % (route, c.name, dtype)
    two = not F.is_f32(dtype)
    a8 = 8 if two else 4                                    # elements of a 16-byte step
    co = c.out_channels()
    wide_store = two and route.startswith("igemm") and not c.flags & F.DD_PIXSHUF
    cv = F.round_up(co, 8) if wide_store else co
    xv = View(c.in_grid(), c.cin, c.cin, F.round_up(c.cin, 8) + 16, 8, dtype, x)
    yv = View(c.out_grid(), co, cv, F.round_up(cv, 8) + 24, 16, dtype, old if c.accum else None, PAD_OLD if c.accum else SENTINEL)
    if not c.accum:
        yv.buf[..., yv.off:yv.off + co] = SENTINEL          # every element must be written
    resv = View(c.out_grid(), co, cv, F.round_up(cv, 8) + 8, a8, dtype, res) if c.res else None
    maskv = View(c.out_grid(), co, cv, F.round_up(cv, 8) + 16, (4 if two else 2) if c.mask_off8 else a8, dtype, mask) if c.mask else None
    k_pad = c.k_pad(dtype)
    wp = U.pack_image(lib, name, w.reshape(-1), dtype, c.taps, c.n, c.cin, c.n_pad, k_pad, c.n * c.cin, c.cin, 1, 0)
    wp_before = wp.clone()
    bv = Guarded(c.nbias, bias[:c.nbias]) if c.nbias is not None else None
    a = L.ConvArgs()
    a.x, a.ldx, a.cin, a.wp, a.k_pad, a.n_pad = xv.ptr, xv.ld, c.cin, wp.data_ptr(), k_pad, c.n_pad
    if bv:
        a.bias, a.nbias = bv.ptr, c.nbias
    if resv:
        a.res, a.ldres = resv.ptr, resv.ld
    if maskv:
        a.mask, a.ldmask = maskv.ptr, maskv.ld
    a.y, a.ldy, a.n, a.B, a.H, a.W, a.taps, a.flags, a.dtype = yv.ptr, yv.ld, c.n, c.B, c.H, c.W, c.taps, c.flags, U.DT[dtype][0]
    with Routes(route, name):
        L.check(lib.dd_conv_igemm(C.byref(a), U.stream()))
        torch.cuda.synchronize()
    assert xv.unchanged() and (not resv or resv.unchanged()) and (not maskv or maskv.unchanged()), name + ": an input buffer was written"
    assert torch.equal(wp.view(torch.uint8), wp_before.view(torch.uint8)), name + ": the weight image was written"
    assert not bv or (bv.guards_intact() and torch.equal(bv.values(), bias[:c.nbias])), name + ": the bias was written"
    U.gated(name + " y", yv.values(), ref["y"], F.gate_y(ref, dtype, route))
    check(name + " y rel-L2", yv.values(), ref["y"], ROUND[TOLKEY[dtype]])
    assert yv.neighbours_intact(), name + ": a channel outside the view was written"
    if cv > co:
        assert bool((yv.pads() == (PAD_OLD if c.accum else 0.0)).all()), name + ": pad channels n .. n rounded up to 8"
    return route


@pytest.mark.parametrize("c,dtype", _params(F.IGEMM_CASES))
def test_conv_igemm(c, dtype):
    _need_gpu()
    _igemm(L.load(), c, dtype)


@pytest.mark.parametrize("c,dtype", _params(F.PW_CASES))
def test_conv_igemm_wide_1x1(c, dtype):
    """2 x 128 x 128 pixels: conv_pw_kernel (or, with DD_CONV_PW=0, the implicit-GEMM kernels)."""
    _need_gpu()
    _igemm(L.load(), c, dtype)


# ---------------------------------------------------------------------------------------------------------------- dd_conv_wgrad
def _wgrad(lib, c, dtype):
    p, q = F.wgrad_inputs(c.id, dtype)
    ref = F.wgrad_reference(c.id, dtype)
    route = F.wgrad_route(c, dtype, ENV)
    name = "conv_wgrad [%s] %s %s" % (route, c.name, dtype)
    a8 = 8 if not F.is_f32(dtype) else 4
    mv, nv = F.round_up(c.m, a8), F.round_up(c.n, a8)
    pv = View(c.p_grid(), c.m, mv, F.round_up(mv, 8) + 16, 8, dtype, p)
    qv = View((c.B, c.H, c.W), c.n, nv, F.round_up(nv, 8) + 24, 16, dtype, q)
    npix = c.B * c.H * c.W
    fill = torch.full((1,), F.PREFILL) if c.prefill else None
    a = L.WgradArgs()
    a.p, a.ldp, a.m, a.q, a.ldq, a.n = pv.ptr, pv.ld, c.m, qv.ptr, qv.ld, c.n
    a.B, a.H, a.W, a.taps, a.flags, a.dtype, a.ksplit, a.bias_mode = c.B, c.H, c.W, c.taps, c.flags, U.DT[dtype][0], c.ksplit, c.bias_mode
    outs = []      # (label, Guarded, reference, budget)
    if c.stack:
        m0, width, blocks = c.stack
        a.stack_blocks, a.stack_width, a.stack_m0 = blocks, width, m0
        for j in range(blocks):
            rows = m0 + j * width
            o = Guarded(9 * rows * width, fill.expand(9 * rows * width) if c.prefill else None)
            a.stack_out[j] = o.ptr
            outs.append(("stack_out[%d]" % j, o, F.stacked_block(ref["out"], j, m0, width), ref["out_budget"][:, :rows, j * width:(j + 1) * width]))
            if c.bias_mode:
                b = Guarded(width, fill.expand(width) if c.prefill else None)
                a.stack_bias[j] = b.ptr
                outs.append(("stack_bias[%d]" % j, b, ref["bias"][j * width:(j + 1) * width], ref["bias_budget"][j * width:(j + 1) * width]))
    else:
        o = Guarded(c.taps * c.m * c.n, fill.expand(c.taps * c.m * c.n) if c.prefill else None)
        a.out = o.ptr
        outs.append(("out", o, ref["out"], ref["out_budget"]))
        if c.bias_mode:
            nb = c.n if c.bias_mode == 1 else c.m
            b = Guarded(nb, fill.expand(nb) if c.prefill else None)
            a.bias_out = b.ptr
            outs.append(("bias_out", b, ref["bias"], ref["bias_budget"]))
    if route == "refused":      # the stacked form off the LDS-DMA kernel: the documented error, nothing launched, nothing written
        with Routes(None, name):
            assert lib.dd_conv_wgrad(C.byref(a), U.stream()) == -1 and b"stacked form runs on the LDS-DMA kernel only" in lib.dd_last_error()
            torch.cuda.synchronize()
        for label, arr, _, _ in outs:
            assert arr.guards_intact() and bool((arr.values() == (F.PREFILL if c.prefill else 0.0)).all()), "%s %s: written by a refused call" % (name, label)
        return route
    with Routes(route, name):
        L.check(lib.dd_conv_wgrad(C.byref(a), U.stream()))
        torch.cuda.synchronize()
    assert pv.unchanged() and qv.unchanged(), name + ": an input buffer was written"
    for label, arr, want, budget in outs:
        terms = npix * (4 if label.startswith("bias") and c.bias_mode == 2 else 1)      # (the column sums of P run over the fine grid)
        if c.prefill:
            want, budget = F.prefilled(want, budget, terms)
        U.gated("%s %s" % (name, label), arr.values().reshape(want.shape), want, F.gate_f32(budget))
        check("%s %s rel-L2" % (name, label), arr.values().reshape(want.shape), want, ACC32[TOLKEY[dtype]])
        assert arr.guards_intact(), "%s %s: a guard word was written (the array ends where conv j's own input width ends)" % (name, label)
    return route


@pytest.mark.parametrize("c,dtype", _params(F.WGRAD_CASES))
def test_conv_wgrad(c, dtype):
    _need_gpu()
    _wgrad(L.load(), c, dtype)


@pytest.mark.parametrize("c,dtype", _params(F.WGRAD_PW_CASES))
def test_conv_wgrad_wide_1x1(c, dtype):
    """2 x 128 x 128 pixels: wgrad_pw_kernel above 256 channels on a side; 129 .. 256 (without DD_WGRAD_PW_MID) and 64 x 64 stay on the LDS-DMA kernel."""
    _need_gpu()
    _wgrad(L.load(), c, dtype)


# ---------------------------------------------------------------------------------------------------------------- dd_conv3x3_ks, mode 0
def _ks(lib, c, dtype):
    """Input and output are ONE allocation, as in a dense block: channels [0, cin) of the buffer are x, the launch writes channels
    [cin, cin + n) -- through y = buffer + (cin - n0) channels, so that y[p][n0 + c] lands there -- and everything behind stays the sentinel."""
    x, w, bias, mask, old = F.ks_inputs(c.id, dtype)
    ref = F.ks_reference(c.id, dtype)
    route = F.ks_route(c, ENV)
    name = "conv3x3_ks [%s] %s %s" % (route, c.name, dtype)
    tdt = U.DT[dtype][1]
    ld = c.cin + c.n + 16
    buf = torch.full((c.B, c.H, c.W, ld), SENTINEL, dtype=tdt, device="cuda")
    buf[..., :c.cin] = x.to(tdt).cuda()
    if c.accum:
        buf[..., c.cin:c.cin + c.n] = old.to(tdt).cuda()
    before = buf.clone()
    maskv = View((c.B, c.H, c.W), c.n, c.n, c.n + 24, 4 if c.mask_off8 else 8, dtype, mask) if c.mask else None
    k_pad = c.k_pad(dtype)
    rows = c.n0 + c.n
    wp = U.pack_image(lib, name, w.reshape(-1), dtype, 9, rows, c.cin, c.n_pad, k_pad, rows * c.cin, c.cin, 1, 0)
    wp_before = wp.clone()
    use_bias = c.nbias is not None and not c.grad
    bv = Guarded(c.nbias, bias[:c.nbias]) if use_bias else None
    a = L.ConvKsArgs()
    a.x, a.ldx, a.cin, a.wp, a.n_pad, a.k_pad = buf.data_ptr(), ld, c.cin, wp.data_ptr(), c.n_pad, k_pad
    if bv:
        a.bias, a.nbias = bv.ptr, c.nbias
    a.y, a.ldy, a.n0, a.n = buf.data_ptr() + 2 * (c.cin - c.n0), ld, c.n0, c.n
    a.B, a.H, a.W, a.mode, a.flags, a.dtype = c.B, c.H, c.W, 0, c.flags, U.DT[dtype][0]
    if maskv:
        a.mask, a.ldmask = maskv.ptr - 2 * c.n0, maskv.ld      # mask[p][n0 + c]
    with Routes(route, name):
        L.check(lib.dd_conv3x3_ks(C.byref(a), U.stream()))
        torch.cuda.synchronize()
    assert torch.equal(buf[..., :c.cin].contiguous().view(torch.int16), before[..., :c.cin].contiguous().view(torch.int16)), name + ": the input channels were written"
    assert bool((buf[..., c.cin + c.n:] == SENTINEL).all()), name + ": a channel behind the output range was written"
    assert (not maskv or maskv.unchanged()) and torch.equal(wp.view(torch.int16), wp_before.view(torch.int16)), name + ": mask or weight image written"
    assert not bv or (bv.guards_intact() and torch.equal(bv.values(), bias[:c.nbias])), name + ": the bias was written"
    got = buf[..., c.cin:c.cin + c.n].double().cpu()
    U.gated(name + " y", got, ref["y"], F.gate_y(ref, dtype, "pw"))      # ("pw": the gate of a path that rounds once)
    check(name + " y rel-L2", got, ref["y"], ROUND[dtype])


@pytest.mark.parametrize("c,dtype", _params(F.KS_CASES))
def test_conv3x3_ks_mode0(c, dtype):
    _need_gpu()
    _ks(L.load(), c, dtype)


@pytest.mark.parametrize("dtype", list(F.DTYPES2))
@pytest.mark.parametrize("case", F.KST_CASES, ids=["%dx%d_at_%d_%s" % (c[0], c[1], c[2], "x".join(map(str, c[3]))) for c in F.KST_CASES])
def test_conv3x3_ks_transposed_parities(case, dtype):
    """Modes 1 .. 4, each into its own parity of one buffer (the other three parities untouched by that launch), and mode 5 into another: both
    gated against the float64 transposed conv, and bit-identical to each other."""
    _need_gpu()
    lib = L.load()
    cin, n, n0, (B, H, W), relu, nbias = case
    x, k, bias = F.kst_inputs(case, dtype)
    ref, budget = F.kst_reference(case, dtype)
    name = "conv3x3_ks [ks] modes 1-5 %dx%d at %d on %dx%dx%d %s" % (cin, n, n0, B, H, W, dtype)
    rows = n0 + n
    n_pad, k_pad = F.round_up(rows, 16), F.round_up(cin, 32)
    xv = View((B, H, W), cin, cin, cin + 16, 8, dtype, x)
    wp = U.pack_image(lib, name, F.convt3_image(k).reshape(-1), dtype, 9, rows, cin, n_pad, k_pad, rows * cin, cin, 1, 0)
    bv = Guarded(nbias, bias[:nbias])

    def launch(mode, yv):
        a = L.ConvKsArgs()
        a.x, a.ldx, a.cin, a.wp, a.n_pad, a.k_pad, a.bias, a.nbias = xv.ptr, xv.ld, cin, wp.data_ptr(), n_pad, k_pad, bv.ptr, nbias
        a.y, a.ldy, a.n0, a.n = yv.ptr - 2 * n0, yv.ld, n0, n
        a.B, a.H, a.W, a.mode, a.flags, a.dtype = B, H, W, mode, F.DD_OUT_RELU if relu else 0, U.DT[dtype][0]
        with Routes("ks", "%s mode %d" % (name, mode)):
            L.check(lib.dd_conv3x3_ks(C.byref(a), U.stream()))
            torch.cuda.synchronize()

    def fresh():
        v = View((B, 2 * H, 2 * W), n, n, n + 24, 8, dtype)
        v.buf[..., v.off:v.off + n] = SENTINEL
        return v

    single, whole = fresh(), fresh()
    for mode in (1, 2, 3, 4):
        py, px = (mode - 1) // 2, (mode - 1) % 2
        before = single.buf.clone()
        launch(mode, single)
        changed = (single.buf != before)
        changed[:, py::2, px::2] = False
        assert not bool(changed.any()), "%s mode %d wrote outside its parity" % (name, mode)
        assert not bool((single.values()[:, py::2, px::2] == SENTINEL).any()), "%s mode %d left elements of its parity unwritten" % (name, mode)
    launch(5, whole)
    gate_t = F.gate_storage(ref, budget, dtype)
    for label, v in (("singly", single), ("mode 5", whole)):
        U.gated("%s %s y" % (name, label), v.values(), ref, gate_t)
        check("%s %s y rel-L2" % (name, label), v.values(), ref, ROUND[dtype])
        assert v.neighbours_intact(), "%s %s: a channel outside the view was written" % (name, label)
    assert torch.equal(single.buf.view(torch.int16), whole.buf.view(torch.int16)), name + ": the four single-parity launches differ from mode 5"
    assert xv.unchanged() and bv.guards_intact(), name + ": an input was written"


@pytest.mark.parametrize("dtype", list(F.DTYPES2))
@pytest.mark.parametrize("case", F.K6_CASES, ids=["cp%d_%d_at_%d_%s_%s" % (c[0], c[1], c[2], "x".join(map(str, c[3])), c[7]) for c in F.K6_CASES])
def test_conv3x3_ks_mode6(case, dtype):
    """Mode 6 -- the 2 x 2-tap conv over the parity-rearranged output gradient that is the data gradient of the 3x3 / stride-2 transposed conv --
    on conv_ks_kernel and, with more than 128 channels on 2 048 pixels, on the tap form of conv_pw_kernel (which skips the K-slices the
    block-sparse image leaves empty).  The image taps the mode never reads hold values of 3 and more."""
    _need_gpu()
    lib = L.load()
    cp, n, n0, (B, H, W), flags, nbias, use_mask, _ = case
    cin, rows = 4 * cp, n0 + n
    dy, k, bias, mask, old, filler = F.k6_inputs(case, dtype)
    ref = F.k6_reference(case, dtype)
    route = F.ks6_route(case, ENV)
    name = "conv3x3_ks [%s] mode 6 cp %d -> %d at %d on %dx%dx%d flags %d %s" % (route, cp, n, n0, B, H, W, flags, dtype)
    accum = bool(flags & F.DD_ACCUM)
    xv = View((B, H, W), cin, cin, cin + 16, 8, dtype, F.space_to_depth(dy))
    yv = View((B, H, W), n, n, n + 24, 8, dtype, old if accum else None)
    if not accum:
        yv.buf[..., yv.off:yv.off + n] = SENTINEL
    maskv = View((B, H, W), n, n, n + 16, 8, dtype, mask) if use_mask else None
    n_pad, k_pad = F.round_up(rows, 16), F.round_up(cin, 32)
    wp = U.pack_image(lib, name, F.mode6_image(k, filler).reshape(-1), dtype, 9, rows, cin, n_pad, k_pad, rows * cin, cin, 1, 0)
    wp_before = wp.clone()
    bv = Guarded(nbias, bias[:nbias]) if nbias is not None else None
    a = L.ConvKsArgs()
    a.x, a.ldx, a.cin, a.wp, a.n_pad, a.k_pad = xv.ptr, xv.ld, cin, wp.data_ptr(), n_pad, k_pad
    if bv:
        a.bias, a.nbias = bv.ptr, nbias
    a.y, a.ldy, a.n0, a.n = yv.ptr - 2 * n0, yv.ld, n0, n
    a.B, a.H, a.W, a.mode, a.flags, a.dtype = B, H, W, 6, flags, U.DT[dtype][0]
    if maskv:
        a.mask, a.ldmask = maskv.ptr - 2 * n0, maskv.ld
    with Routes(route, name):
        L.check(lib.dd_conv3x3_ks(C.byref(a), U.stream()))
        torch.cuda.synchronize()
    assert xv.unchanged() and (not maskv or maskv.unchanged()) and torch.equal(wp.view(torch.int16), wp_before.view(torch.int16)), name + ": an input was written"
    assert not bv or (bv.guards_intact() and torch.equal(bv.values(), bias[:nbias])), name + ": the bias was written"
    U.gated(name + " y", yv.values(), ref["y"], F.gate_y(ref, dtype, "pw"))      # (one rounding on both routes)
    check(name + " y rel-L2", yv.values(), ref["y"], ROUND[dtype])
    assert yv.neighbours_intact(), name + ": a channel outside the view was written"


def test_conv3x3_ks_refusals_launch_nothing():
    _need_gpu()
    lib = L.load()
    B, H, W = 1, 4, 4

    def args(**over):
        tdt = torch.bfloat16
        t = dict(x=torch.zeros(B, H, W, 64, dtype=tdt, device="cuda"), wp=torch.zeros(9 * 64 * 64, dtype=tdt, device="cuda"),
                 y=torch.full((B, 2 * H, 2 * W, 64), SENTINEL, dtype=tdt, device="cuda"), aux=torch.zeros(B, H, W, 64, dtype=tdt, device="cuda"))
        a = L.ConvKsArgs()
        a.x, a.ldx, a.cin, a.wp, a.n_pad, a.k_pad = t["x"].data_ptr(), 64, 16, t["wp"].data_ptr(), 32, 32
        a.y, a.ldy, a.n0, a.n, a.B, a.H, a.W, a.mode, a.flags, a.dtype = t["y"].data_ptr(), 64, 16, 16, B, H, W, 0, 0, L.DD_BF16
        for key, v in over.items():
            setattr(a, key, v(a, t) if callable(v) else v)
        return a, t

    aux = lambda a, t: t["aux"].data_ptr()      # noqa: E731
    cases = [("null x", dict(x=None)), ("null wp", dict(wp=None)), ("null y", dict(y=None)), ("f32 storage", dict(dtype=L.DD_F32)),
             ("B 0", dict(B=0)), ("cin 0", dict(cin=0)), ("n 0", dict(n=0)), ("n0 -16", dict(n0=-16)), ("mode 7", dict(mode=7)), ("mode -1", dict(mode=-1)),
             ("DD_IN_RELU with mode 1", dict(mode=1, flags=F.DD_IN_RELU)), ("DD_PIXSHUF", dict(flags=F.DD_PIXSHUF)),
             ("DD_ACCUM with mode 1", dict(mode=1, flags=F.DD_ACCUM)), ("mask with mode 5", dict(mode=5, mask=aux, ldmask=64)),
             ("DD_ACCUM with DD_OUT_RELU", dict(flags=F.DD_ACCUM | F.DD_OUT_RELU)), ("mask with DD_IN_RELU", dict(flags=F.DD_IN_RELU, mask=aux, ldmask=64)),
             ("ldmask 62", dict(mask=aux, ldmask=62)), ("mask 4 bytes off", dict(mask=lambda a, t: t["aux"].data_ptr() + 4, ldmask=64)),
             ("ldx 60", dict(ldx=60)), ("ldy 62", dict(ldy=62)), ("k_pad 48", dict(k_pad=48)), ("n_pad 24", dict(n_pad=24)), ("n0 8", dict(n0=8)),
             ("n 6", dict(n=6)), ("n0 + n > n_pad", dict(n=32)), ("cin > k_pad", dict(cin=40)),
             ("x 8 bytes off", dict(x=lambda a, t: a.x + 8)), ("wp 8 bytes off", dict(wp=lambda a, t: a.wp + 8)), ("y 4 bytes off", dict(y=lambda a, t: a.y + 4))]
    for what, over in cases:
        a, t = args(**over)
        with Routes(None, what):
            _refused(lib, lib.dd_conv3x3_ks(C.byref(a), U.stream()), dict(y=t["y"]), "dd_conv3x3_ks " + what)
    for over in (dict(), dict(flags=F.DD_ACCUM, mask=aux, ldmask=64), dict(mode=5)):      # controls
        a, t = args(**over)
        with Routes("ks", str(over)):
            assert lib.dd_conv3x3_ks(C.byref(a), U.stream()) == 0, (over, lib.dd_last_error())
            torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(lib, rc, outs, what):
    torch.cuda.synchronize()
    assert rc == -1 and lib.dd_last_error(), what + ": accepted (status %d)" % rc
    for key, t in outs.items():
        assert bool((t == SENTINEL).all()), "%s: %s was written" % (what, key)


def test_conv_igemm_refusals_launch_nothing():
    """One case per DD_REQUIRE of dd_conv_igemm: DD_ERR_INVALID, a message, no counter moved, y untouched.  The un-tampered descriptor is
    accepted, so each refusal is due to the one field changed."""
    _need_gpu()
    lib = L.load()
    B, H, W = 1, 4, 4

    def args(dtype="bf16", **over):
        tdt = U.DT[dtype][1]
        t = dict(x=torch.zeros(B, 2 * H, 2 * W, 32, dtype=tdt, device="cuda"), wp=torch.zeros(9 * 32 * 64, dtype=tdt, device="cuda"),
                 y=torch.full((B, 2 * H, 2 * W, 32), SENTINEL, dtype=tdt, device="cuda"), aux=torch.zeros(B, H, W, 32, dtype=tdt, device="cuda"))
        a = L.ConvArgs()
        a.x, a.ldx, a.cin, a.wp, a.k_pad, a.n_pad = t["x"].data_ptr(), 32, 16, t["wp"].data_ptr(), 32, 32
        a.y, a.ldy, a.n, a.B, a.H, a.W, a.taps, a.flags, a.dtype = t["y"].data_ptr(), 32, 16, B, H, W, 9, 0, U.DT[dtype][0]
        for key, v in over.items():
            setattr(a, "dtype" if key == "raw_dtype" else key, v(a, t) if callable(v) else v)
        return a, t

    cases = [("null x", dict(x=None)), ("null wp", dict(wp=None)), ("null y", dict(y=None)), ("bad dtype", dict(raw_dtype=3)),
             ("taps 2", dict(taps=2)), ("taps 4 without DD_GATHER2X2", dict(taps=4)), ("DD_GATHER2X2 with taps 9", dict(flags=F.DD_GATHER2X2)),
             ("DD_PIXSHUF with taps 9", dict(flags=F.DD_PIXSHUF)), ("cin 6 (not a multiple of 16 bytes)", dict(cin=6)), ("cin 0", dict(cin=0)),
             ("ldx 36", dict(ldx=36)), ("k_pad < cin", dict(cin=48)), ("k_pad 48 (not a multiple of 64 bytes)", dict(k_pad=48)),
             ("n_pad 24", dict(n_pad=24)), ("n 0", dict(n=0)), ("n > n_pad", dict(n=48)), ("n 18", dict(n=18)),
             ("DD_PIXSHUF with n 24", dict(taps=1, flags=F.DD_PIXSHUF, n=24)),
             ("DD_PIXSHUF with cout 4 in 2-byte storage (an 8-channel vector would straddle two parities)", dict(taps=1, flags=F.DD_PIXSHUF, n=16)),
             ("ldy 34", dict(ldy=34)),
             ("ldres 34", dict(res=lambda a, t: t["aux"].data_ptr(), ldres=34)), ("ldmask 34", dict(mask=lambda a, t: t["aux"].data_ptr(), ldmask=34)),
             ("B 0", dict(B=0)), ("H 0", dict(H=0)), ("W -1", dict(W=-1)),
             ("x 8 bytes off", dict(x=lambda a, t: a.x + 8)), ("wp 8 bytes off", dict(wp=lambda a, t: a.wp + 8)), ("y 8 bytes off", dict(y=lambda a, t: a.y + 8))]
    for what, over in cases:
        a, t = args(**over)
        with Routes(None, what):
            _refused(lib, lib.dd_conv_igemm(C.byref(a), U.stream()), dict(y=t["y"]), "dd_conv_igemm " + what)
    a, t = args(dtype="f32", cin=6)      # f32 storage: 16 bytes are 4 channels
    _refused(lib, lib.dd_conv_igemm(C.byref(a), U.stream()), dict(y=t["y"]), "dd_conv_igemm f32 cin 6")
    for over in (dict(), dict(taps=1, flags=F.DD_PIXSHUF, n=32), dict(dtype="f32", taps=1, flags=F.DD_PIXSHUF), dict(taps=4, flags=F.DD_GATHER2X2),
                 dict(res=lambda a, t: t["aux"].data_ptr(), ldres=32, mask=lambda a, t: t["aux"].data_ptr(), ldmask=32)):      # controls
        a, t = args(**over)
        assert lib.dd_conv_igemm(C.byref(a), U.stream()) == 0, (over, lib.dd_last_error())
        torch.cuda.synchronize()
        rows = 4 * B * H * W if over.get("flags", 0) & F.DD_PIXSHUF else B * H * W      # (the kernel's pixel index is linear: the first rows of the buffer)
        assert not bool((t["y"].view(-1, 32)[:rows, :4] == SENTINEL).any()), over


def test_conv_wgrad_refusals_launch_nothing():
    _need_gpu()
    lib = L.load()
    B, H, W = 1, 4, 4

    def args(dtype="bf16", stack=None, **over):
        tdt = U.DT[dtype][1]
        t = dict(p=torch.zeros(B, 2 * H, 2 * W, 1024, dtype=tdt, device="cuda"), q=torch.zeros(B, H, W, 1024, dtype=tdt, device="cuda"),
                 out=torch.full((9 * 32 * 32,), SENTINEL, device="cuda"), bias=torch.full((32,), SENTINEL, device="cuda"))
        a = L.WgradArgs()
        a.p, a.ldp, a.m, a.q, a.ldq, a.n = t["p"].data_ptr(), 1024, 32, t["q"].data_ptr(), 1024, 32
        a.out, a.bias_out, a.bias_mode, a.B, a.H, a.W, a.taps, a.dtype = t["out"].data_ptr(), t["bias"].data_ptr(), 1, B, H, W, 9, U.DT[dtype][0]
        if stack:
            m0, width, blocks = stack
            a.stack_blocks, a.stack_width, a.stack_m0, a.m, a.n = blocks, width, m0, m0 + (blocks - 1) * width, blocks * width
            for j in range(min(blocks, 8)):
                t["so%d" % j] = torch.full((9 * (m0 + j * width) * width,), SENTINEL, device="cuda")
                t["sb%d" % j] = torch.full((width,), SENTINEL, device="cuda")
                a.stack_out[j], a.stack_bias[j] = t["so%d" % j].data_ptr(), t["sb%d" % j].data_ptr()
        for key, v in over.items():
            if key == "drop_stack_out":
                a.stack_out[v] = None
            else:
                setattr(a, "dtype" if key == "raw_dtype" else key, v(a, t) if callable(v) else v)
        return a, t

    cases = [("null p", dict(p=None)), ("null q", dict(q=None)), ("null out", dict(out=None)), ("bad dtype", dict(raw_dtype=7)),
             ("taps 3", dict(taps=3)), ("taps 4 without DD_GATHER2X2", dict(taps=4)), ("DD_GATHER2X2 with taps 9", dict(flags=F.DD_GATHER2X2)),
             ("m 0", dict(m=0)), ("ldp 1020", dict(ldp=1020)), ("ldq below the rounded n", dict(ldq=24)), ("B 0", dict(B=0)), ("H 0", dict(H=0)),
             ("p 8 bytes off", dict(p=lambda a, t: a.p + 8)), ("q 8 bytes off", dict(q=lambda a, t: a.q + 8)),
             ("bias_mode 3", dict(bias_mode=3)), ("bias_mode 1 without bias_out", dict(bias_out=None)),
             ("stacked: 9 blocks", dict(stack=(8, 8, 9))), ("stacked: taps 1", dict(stack=(16, 16, 2), taps=1)),
             ("stacked: f32 storage", dict(stack=(16, 16, 2), dtype="f32")), ("stacked: n mismatch", dict(stack=(16, 16, 2), n=16)),
             ("stacked: m mismatch", dict(stack=(16, 16, 2), m=16)), ("stacked: bias_mode 2", dict(stack=(16, 16, 2), bias_mode=2)),
             ("stacked: a block without output", dict(stack=(16, 16, 3), drop_stack_out=1)),
             ("stacked: 15 x 16 slice pairs, more than the LDS-DMA kernel's table holds", dict(stack=(8, 128, 8)))]
    for what, over in cases:
        a, t = args(**over)
        with Routes(None, what):
            _refused(lib, lib.dd_conv_wgrad(C.byref(a), U.stream()), {k: v for k, v in t.items() if k not in ("p", "q")}, "dd_conv_wgrad " + what)
    for over in (dict(), dict(stack=(16, 16, 2))) if F._on(ENV, "DD_WGRAD_DMA") else (dict(),):      # controls
        a, t = args(**over)
        assert lib.dd_conv_wgrad(C.byref(a), U.stream()) == 0, (over, lib.dd_last_error())
        torch.cuda.synchronize()
