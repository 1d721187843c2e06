"""-m gpu: the fused backward launches op by op through the C-ABI -- dd_conv3x3_bwd (cout <= 64, the 65..96 kernel of csrc/dd_conv_bwd96.hip,
the per-64 launches of wider layers, dx = NULL), dd_conv3x3_bwd_multi, dd_convt2x2_fwd / dd_convt2x2_bwd and dd_pack_weights(_batched) --
against the float64 reference and error budget of tests/conv_bwd_ref.py.  No Graph is built: every argument struct is filled by hand.

THE GATE is elementwise on every element of every output (conv_bwd_ref.py): 2 * n * u * S for the fp32 outputs, plus half a storage ulp per
rounding of the path for dx / y.  The worst error / gate of every output is printed and recorded (gpu_util.gate, bound 1); the rel-L2 gates
of gpu_util (ROUND / ACC32) stay next to it.  tests/test_conv_bwd_ref.py shows on the CPU, for these very inputs, that an fp32 evaluation
stays within the gate and that dropped taps, halos, channel groups, blocks, masks and swapped parities do not.

Every operand is a channel view at a non-zero, legally aligned channel offset inside a wider buffer whose other channels hold a sentinel; dw / db
sit between guard words.  All of them must be bit-unchanged after the launch; pad channels up to the next multiple of 8 are zero in the inputs
and, in dx, come back 0 (or, with accumulate, as they were: the kernels store whole 4-channel groups below cinv)."""
import ctypes as C
import os

import pytest
import torch

import conv_bwd_ref as R
import conv_ops_util as U
from deepdenoiser_amd import _lib as L
from gpu_util import ACC32, ROUND, check

pytestmark = pytest.mark.gpu
PAD_OLD = 0.5           # what the pad channels cin..cinv-1 of an accumulated-into dx hold before the launch
DT = {k: U.DT[k] for k in ("bf16", "f16")}
SENTINEL, G, View, Guarded = U.SENTINEL, U.G, U.View, U.Guarded      # shared with tests/test_gpu_conv_fwd_ops.py (tests/conv_ops_util.py)
_stream, _bits, _pack, _gated = U.stream, U.bits, U.pack, U.gated
# libdd_hip.so reads the switch once per process: `e && e[0] == '0'` turns the 65..96 kernel off and those layers run one launch per 64 channels
BWD96_OFF = os.environ.get("DD_CONV_BWD96", "1")[:1] == "0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count      # the attribute dd_device_cus() reads


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def _r8(c):
    return R.round_up(c, 8)


def _check_fp32(name, arr, ref, budget, dtype):
    _gated(name, arr.values().reshape(ref.shape), ref, R.gate_f32(budget))
    check(name + " rel-L2", arr.values().reshape(ref.shape), ref, ACC32[dtype])
    assert arr.guards_intact(), name + ": a guard word was written"


def _check_dx(name, dxv, ref, dtype, accumulate):
    pts = ref["dx_points"]
    _gated(name, dxv.values(), ref["dx"], R.gate_storage(ref["dx"], ref["dx_budget"], dtype, pts))
    check(name + " rel-L2", dxv.values(), ref["dx"], ROUND[dtype])
    assert dxv.neighbours_intact(), name + ": a channel outside the view was written"
    if dxv.cv > dxv.C:      # the 4-channel groups below cinv are stored whole: the sum over zero weights, i.e. 0, added to what was there
        assert bool((dxv.pads() == (PAD_OLD if accumulate else 0.0)).all()), name + ": pad channels cin..cinv-1 of dx"


# ---------------------------------------------------------------------------------------------------------------- dd_conv3x3_bwd
def _conv_bwd(lib, shape, dtype, mask, acc, per64=False, want_dx=True, db_null=False, other_ld=False, tag=""):
    cin, cout, B, H, W = shape
    cinv, coutv = _r8(cin), _r8(cout)
    x, dy, k, old = R.conv_inputs(shape, dtype)
    ref = R.conv_reference(shape, dtype, mask, acc, per64)
    name = "conv3x3_bwd%s %s %s mask%d acc%d" % (tag, "x".join(map(str, shape)), dtype, mask, acc)
    dyv = View((B, H, W), cout, coutv, coutv + 16, 8, dtype, dy)
    xv = View((B, H, W), cin, cinv, cinv + 24, 16, dtype, x)
    a = L.ConvBwdArgs()
    a.dy, a.ld_dy, a.cout, a.x, a.ld_x, a.cin = dyv.ptr, dyv.ld, cout, xv.ptr, xv.ld, cin
    dxv = None
    if want_dx:
        # ld_dx == ld_x at channel offset 16, or (other_ld) a row of its own length at the 8-byte-aligned offset 4
        dxv = View((B, H, W), cin, cinv, cinv + 12 if other_ld else xv.ld, 4 if other_ld else 16, dtype, old if acc else None, PAD_OLD if acc else SENTINEL)
        if not acc:
            dxv.buf[..., dxv.off:dxv.off + cin] = SENTINEL      # every element must be written
        wd, a.n_pad, a.k_pad = _pack(lib, "conv", "dgrad", k, cin, cout, dtype)
        a.wd, a.dx, a.ld_dx = wd.data_ptr(), dxv.ptr, dxv.ld
    dw, db = Guarded(9 * cin * cout), Guarded(cout)
    a.dw, a.db = dw.ptr, None if db_null else db.ptr
    a.B, a.H, a.W, a.use_mask, a.accumulate, a.dtype = B, H, W, mask, acc, DT[dtype][0]
    L.check(lib.dd_conv3x3_bwd(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert dyv.unchanged() and xv.unchanged(), name + ": an input buffer was written"
    if want_dx:
        _check_dx(name + " dx", dxv, ref, dtype, acc)
    _check_fp32(name + " dw", dw, ref["dw"], ref["dw_budget"], dtype)
    if db_null:
        assert bool((db.buf[G:G + cout] == 0).all()) and db.guards_intact()
    else:
        _check_fp32(name + " db", db, ref["db"], ref["db_budget"], dtype)
    return dxv.values() if want_dx else None


def _assert_launches(name, got, shape, dtype, per64):
    """Which path stored this dx (mask 0, accumulate 0)?  One launch rounds the fp32 sum over all output channels once; per-64 launches round each
    block's sum, then the sum of the rounded values.  The order of an fp32 sum moves a stored value only where it sits within ~2^-22 of a
    rounding boundary (under 1 element in 1 000 even in fp16), the second rounding moves one in every few -- so dx is all but bit-equal to the
    fp32 emulation of the path that ran, and visibly further from the other one."""
    x, dy, k, _ = R.conv_inputs(shape, dtype)
    parts32 = [R.conv3_dx_part(dy.float(), k.float(), c0, c1, magnitudes=False)[0] for c0, c1 in R.co_blocks(shape[1])]
    same = {True: float((got == R.emulate_dx(parts32, x, 0, None, dtype)).double().mean()),
            False: float((got == R.to_storage(sum(parts32), dtype)).double().mean())}
    print("%-84s bit-equal to the per-64 emulation %.4f, to the one-launch emulation %.4f" % (name, same[True], same[False]))
    assert same[per64] >= 0.98 and same[not per64] < same[per64] - 0.02, (name, "expected per-64 launches" if per64 else "expected one launch", same)


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONV_LE64, ids=_ids(R.CONV_LE64))
def test_conv3x3_bwd_up_to_64(shape, dtype):
    _need_gpu()
    lib = L.load()
    for mask, acc in R.FLAGS:
        _conv_bwd(lib, shape, dtype, mask, acc)
    _conv_bwd(lib, shape, dtype, 0, 0, db_null=True, tag=" db=NULL")
    _conv_bwd(lib, shape, dtype, 1, 1, other_ld=True, tag=" ld_dx!=ld_x")
    _conv_bwd(lib, shape, dtype, 1, 0, other_ld=True, tag=" ld_dx!=ld_x")


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONV_96, ids=_ids(R.CONV_96))
def test_conv3x3_bwd_65_to_96(shape, dtype):
    """One launch of csrc/dd_conv_bwd96.hip -- or, in a process started with DD_CONV_BWD96=0 (tests/test_gpu_fallbacks.py), one launch per 64
    output channels of csrc/dd_conv_bwd.hip: the same reference, gated with one rounding per launch.  Which of the two ran is read off dx."""
    _need_gpu()
    lib = L.load()
    for mask, acc in R.FLAGS:
        got = _conv_bwd(lib, shape, dtype, mask, acc, per64=BWD96_OFF, tag=" per-64" if BWD96_OFF else " bwd96")
        if not mask and not acc:
            _assert_launches("conv3x3_bwd %s %s" % ("x".join(map(str, shape)), dtype), got, shape, dtype, BWD96_OFF)


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONV_WIDE, ids=_ids(R.CONV_WIDE))
def test_conv3x3_bwd_wider_than_96_with_dx(shape, dtype):
    """cout > 96 with a data gradient: one launch per 64 output channels, the later ones accumulating into dx (a path the engine never takes)."""
    _need_gpu()
    lib = L.load()
    for mask, acc in R.FLAGS:
        _conv_bwd(lib, shape, dtype, mask, acc, per64=True, tag=" per-64")


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONV_WONLY, ids=_ids(R.CONV_WONLY))
def test_conv3x3_bwd_weights_only(shape, dtype):
    _need_gpu()
    _conv_bwd(L.load(), shape, dtype, 0, 0, want_dx=False, tag=" dx=NULL")


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("route", ["le64", "bwd96", "wide", "wonly"])
def test_conv3x3_bwd_uneven_tile_dealing(route, dtype):
    """Tiles that are no multiple of ksplit: workgroup ks walks tiles tile0(ks), + ksplit, ...; some walk one more than others, and the last
    round prefetches past the end (conv_bwd_ref.uneven_cases states the arithmetic; asserted here for the device at hand)."""
    _need_gpu()
    cus = _cus()
    cases = R.uneven_cases(cus)
    shape = cases[route]
    if route == "bwd96" and BWD96_OFF:      # a process with DD_CONV_BWD96=0 runs 65..96 channels on the cout <= 64 kernel: 64-channel columns
        shape = cases["le64"][:1] + shape[1:]
    cin, cout, B, H, W = shape
    tiles = B * (-(-H // 16)) * (-(-W // 16))
    columns = {"le64": -(-cin // 64), "wide": -(-cin // 64), "bwd96": -(-cin // (64 if BWD96_OFF else 32)), "wonly": -(-cin // 64) * -(-cout // 64)}[route]
    ksplit = min(max(1, cus // columns), tiles)
    assert ksplit < tiles and tiles % ksplit, (cus, shape, tiles, ksplit)
    if route == "wonly":
        _conv_bwd(L.load(), shape, dtype, 0, 0, want_dx=False, tag=" uneven dx=NULL")
    else:
        _conv_bwd(L.load(), shape, dtype, 1, 1, per64=route == "wide" or (route == "bwd96" and BWD96_OFF), tag=" uneven " + route)


# ---------------------------------------------------------------------------------------------------------------- dd_conv3x3_bwd_multi
def _multi(lib, probs, grid, dtype, tag=""):
    B, H, W = grid
    n = len(probs)
    args = (L.ConvBwdArgs * n)()
    keep = []
    for i, (cin, cout) in enumerate(probs):
        x, dy, _, _ = R.conv_inputs((cin, cout, B, H, W), dtype)
        dyv = View(grid, cout, _r8(cout), _r8(cout) + 16, 8, dtype, dy)
        xv = View(grid, cin, _r8(cin), _r8(cin) + 24, 16, dtype, x)
        dw, db = Guarded(9 * cin * cout), Guarded(cout)
        a = args[i]
        a.dy, a.ld_dy, a.cout, a.x, a.ld_x, a.cin = dyv.ptr, dyv.ld, cout, xv.ptr, xv.ld, cin
        a.dw, a.db, a.B, a.H, a.W, a.dtype = dw.ptr, db.ptr, B, H, W, DT[dtype][0]
        keep.append((dyv, xv, dw, db))
    L.check(lib.dd_conv3x3_bwd_multi(args, n, _stream()))
    torch.cuda.synchronize()
    for i, (cin, cout) in enumerate(probs):
        dyv, xv, dw, db = keep[i]
        ref = R.conv_reference((cin, cout, B, H, W), dtype, 0, 0, False)      # float64, not the single launches
        name = "conv3x3_bwd_multi%s %dof%d %dx%d on %s %s" % (tag, i, n, cin, cout, "x".join(map(str, grid)), dtype)
        assert dyv.unchanged() and xv.unchanged(), name
        _check_fp32(name + " dw", dw, ref["dw"], ref["dw_budget"], dtype)
        _check_fp32(name + " db", db, ref["db"], ref["db_budget"], dtype)


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("grid", R.MULTI_GRIDS, ids=_ids(R.MULTI_GRIDS))
def test_conv3x3_bwd_multi(grid, n, dtype):
    _need_gpu()
    _multi(L.load(), R.MULTI_CHANNELS[:n], grid, dtype)


@pytest.mark.parametrize("dtype", list(DT))
def test_conv3x3_bwd_multi_uneven_tile_dealing(dtype):
    _need_gpu()
    cus = _cus()
    probs, grid = R.uneven_multi(cus)
    tiles = grid[0] * (-(-grid[1] // 16)) * (-(-grid[2] // 16))
    for cin, cout in probs:      # ksplit of dd_conv3x3_bwd_multi: cus / (n * nblk * nblk_co)
        ks = max(1, cus // (len(probs) * -(-cin // 64) * -(-cout // 64)))
        assert ks < tiles and tiles % ks, (cus, cin, cout, tiles, ks)
    _multi(L.load(), probs, grid, dtype, " uneven")


# ---------------------------------------------------------------------------------------------------------------- dd_convt2x2_fwd / _bwd
def _convt_fwd(lib, shape, dtype, relu, tag=""):
    cin, cout, B, H, W = shape
    x, _, k, bias, _ = R.convt_inputs(shape, dtype)
    ref, budget = R.convt_fwd_reference(shape, dtype, relu)
    name = "convt2x2_fwd%s %s %s relu%d" % (tag, "x".join(map(str, shape)), dtype, relu)
    xv = View((B, H, W), cin, _r8(cin), _r8(cin) + 16, 8, dtype, x)
    yv = View((B, 2 * H, 2 * W), cout, cout, 2 * cout, cout, dtype)      # the upper half of a 2 * cout concat buffer; the lower half is sentinel
    w, n_pad, k_pad = _pack(lib, "convT2", "fwd", k, cin, cout, dtype)
    bv = Guarded(cout, bias)
    a = L.ConvTArgs()
    a.x, a.ld_x, a.cin, a.y, a.ld_y, a.cout = xv.ptr, xv.ld, cin, yv.ptr, yv.ld, cout
    a.w, a.n_pad, a.k_pad, a.bias, a.relu = w.data_ptr(), n_pad, k_pad, bv.ptr, relu
    a.B, a.H, a.W, a.dtype = B, H, W, DT[dtype][0]
    L.check(lib.dd_convt2x2_fwd(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert xv.unchanged() and bv.guards_intact() and torch.equal(bv.values(), bias), name + ": an input was written"
    _gated(name + " y", yv.values(), ref, R.gate_storage(ref, budget, dtype))
    check(name + " y rel-L2", yv.values(), ref, ROUND[dtype])
    assert yv.neighbours_intact(), name + ": the lower half of the concat buffer was written"


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONVT_FWD, ids=_ids(R.CONVT_FWD))
def test_convt2x2_fwd(shape, dtype):
    _need_gpu()
    for relu in (0, 1):
        _convt_fwd(L.load(), shape, dtype, relu)


def _convt_bwd(lib, shape, dtype, mask, acc, tag=""):
    cin, cout, B, H, W = shape
    cinv = _r8(cin)
    x, dy, k, _, old = R.convt_inputs(shape, dtype)
    ref = R.convt_bwd_reference(shape, dtype, mask, acc)
    name = "convt2x2_bwd%s %s %s mask%d acc%d" % (tag, "x".join(map(str, shape)), dtype, mask, acc)
    xv = View((B, H, W), cin, cinv, cinv + 16, 8, dtype, x)
    dyv = View((B, 2 * H, 2 * W), cout, cout, cout + 24, 16, dtype, dy)
    dxv = View((B, H, W), cin, cinv, cinv + 12, 4, dtype, old if acc else None, PAD_OLD if acc else SENTINEL)
    if not acc:
        dxv.buf[..., dxv.off:dxv.off + cin] = SENTINEL
    w, n_pad, k_pad = _pack(lib, "convT2", "dgrad", k, cin, cout, dtype)
    dw, db = Guarded(4 * cout * cin), Guarded(cout)
    a = L.ConvTArgs()
    a.x, a.ld_x, a.cin, a.y, a.ld_y, a.cout = xv.ptr, xv.ld, cin, dyv.ptr, dyv.ld, cout
    a.w, a.n_pad, a.k_pad = w.data_ptr(), n_pad, k_pad
    a.dx, a.ld_dx, a.dw, a.db, a.use_mask, a.accumulate = dxv.ptr, dxv.ld, dw.ptr, db.ptr, mask, acc
    a.B, a.H, a.W, a.dtype = B, H, W, DT[dtype][0]
    L.check(lib.dd_convt2x2_bwd(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert xv.unchanged() and dyv.unchanged(), name + ": an input buffer was written"
    _check_dx(name + " dx", dxv, ref, dtype, acc)
    _check_fp32(name + " dw", dw, ref["dw"], ref["dw_budget"], dtype)
    _check_fp32(name + " db", db, ref["db"], ref["db_budget"], dtype)


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("shape", R.CONVT_BWD, ids=_ids(R.CONVT_BWD))
def test_convt2x2_bwd(shape, dtype):
    _need_gpu()
    for mask, acc in R.FLAGS:
        _convt_bwd(L.load(), shape, dtype, mask, acc)


@pytest.mark.parametrize("dtype", list(DT))
def test_convt2x2_uneven_tile_dealing(dtype):
    """More 8 x 8-pixel tiles than workgroups (min(tiles, cus)) and no multiple of them: some workgroups walk two tiles, the rest one."""
    _need_gpu()
    cus = _cus()
    cases = R.uneven_cases(cus)
    for key in ("convt_fwd", "convt_bwd"):
        _, _, B, H, W = cases[key]
        tiles = B * (-(-H // 8)) * (-(-W // 8))
        assert cus < tiles and tiles % cus, (cus, tiles)
    _convt_fwd(L.load(), cases["convt_fwd"], dtype, 1, " uneven")
    _convt_bwd(L.load(), cases["convt_bwd"], dtype, 1, 1, " uneven")


# ---------------------------------------------------------------------------------------------------------------- dd_pack_weights(_batched)
PACKS = [("conv", "dgrad", 20, 70), ("conv", "fwd", 20, 70), ("conv", "dgrad", 72, 100), ("convT2", "fwd", 100, 32), ("convT2", "dgrad", 40, 80),
         ("conv", "dgrad", 8, 16)]


@pytest.mark.parametrize("dtype", list(DT))
def test_pack_weights_rounds_to_nearest_even(dtype):
    """fp32 masters that are NOT representable (and exact ties, and values below the smallest normal of fp16): the image is torch's
    round-to-nearest-even conversion of the restatement, bit for bit, padding exactly zero."""
    _need_gpu()
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    for kind, role, cin, cout in PACKS:
        taps = 9 if kind == "conv" else 4
        m = torch.randn(taps * cin * cout, generator=g, dtype=torch.float64) * torch.pow(2.0, torch.randint(-20, 4, (taps * cin * cout,), generator=g).double())
        m[::7] = (1.0 + 2.0 ** -(8 if dtype == "bf16" else 11)) * m[::7].to(DT[dtype][1]).double()      # half-way between two neighbours (mostly)
        _pack(lib, kind, role, m, cin, cout, dtype)


@pytest.mark.parametrize("dtype", list(DT))
def test_pack_weights_batched_side_by_side(dtype):
    """One table: the packs of the cases above as dense images, and three records that stack their [n_pad][k_pad] corners side by side in ONE
    wider image [9][n_pad][dst_ld] (dst_ld, dst_tap_stride; the gather-form data gradient of dd_conv3x3_ks) whose remaining columns nobody writes."""
    _need_gpu()
    lib = L.load()
    code, tdt = DT[dtype]
    g = torch.Generator().manual_seed(6)
    recs, wants, images, keep = [], [], [], []
    for kind, role, cin, cout in PACKS:
        taps, n, k, st, sn, sk, flip = R.pack_params(kind, role, cin, cout)
        n_pad, k_pad = R.pack_dims(n, k)
        src = torch.randn((9 if kind == "conv" else 4) * cin * cout, generator=g).cuda()
        dst = torch.full((taps * n_pad * k_pad + 8,), SENTINEL, dtype=tdt, device="cuda")
        want = torch.full((taps * n_pad * k_pad + 8,), SENTINEL, dtype=tdt)
        R.pack_weights(src.cpu().numpy(), dtype, taps, n, k, n_pad, k_pad, st, sn, sk, flip, dst=want)
        recs.append(L.PackDesc(src.data_ptr(), dst.data_ptr(), taps, n, k, n_pad, k_pad, flip, st, sn, sk, 0, 0))
        wants.append(want)
        images.append(dst)
        keep.append(src)
    # three dgrad records (cin = 24; cout = 16, 40, 8 -> k_pad 32, 64, 32) at columns 0, 32, 96 of a [9][32][160] image; columns 128.. stay
    cin, n_pad, ld = 24, 32, 160
    wide = torch.full((9 * n_pad * ld + 8,), SENTINEL, dtype=tdt, device="cuda")
    want = torch.full((9 * n_pad * ld + 8,), SENTINEL, dtype=tdt)
    col = 0
    for cout in (16, 40, 8):
        taps, n, k, st, sn, sk, flip = R.pack_params("conv", "dgrad", cin, cout)
        k_pad = R.pack_dims(n, k)[1]
        src = torch.randn(9 * cin * cout, generator=g).cuda()
        R.pack_weights(src.cpu().numpy(), dtype, taps, n, k, n_pad, k_pad, st, sn, sk, flip, dst=want, dst_off=col, dst_ld=ld, dst_tap_stride=n_pad * ld)
        recs.append(L.PackDesc(src.data_ptr(), wide.data_ptr() + col * 2, taps, n, k, n_pad, k_pad, flip, st, sn, sk, ld, n_pad * ld))
        keep.append(src)
        col += k_pad
    assert col == 128
    wants.append(want)
    images.append(wide)
    arr = (L.PackDesc * len(recs))(*recs)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    L.check(lib.dd_pack_weights_batched(table.data_ptr(), len(recs), code, _stream()))
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(zip(images, wants)):
        assert torch.equal(_bits(got.cpu()), _bits(want)), "record / image %d differs from the restatement" % i


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    _need_gpu()
    lib = L.load()
    dtype, (code, tdt) = "bf16", DT["bf16"]
    B, H, W = 1, 4, 4

    def conv_args(cin=16, cout=16, **over):
        t = dict(dy=torch.zeros(B, H, W, 32, dtype=tdt, device="cuda"), x=torch.zeros(B, H, W, 32, dtype=tdt, device="cuda"),
                 wd=torch.zeros(9 * 32 * 128, dtype=tdt, device="cuda"), dx=torch.full((B, H, W, 32), SENTINEL, dtype=tdt, device="cuda"),
                 dw=torch.full((9 * 128 * 136,), SENTINEL, device="cuda"), db=torch.full((136,), SENTINEL, device="cuda"))
        a = L.ConvBwdArgs()
        a.dy, a.ld_dy, a.cout, a.x, a.ld_x, a.cin = t["dy"].data_ptr(), 32, cout, t["x"].data_ptr(), 32, cin
        a.wd, a.n_pad, a.k_pad, a.dx, a.ld_dx = t["wd"].data_ptr(), 32, 32, t["dx"].data_ptr(), 32
        a.dw, a.db, a.B, a.H, a.W, a.dtype = t["dw"].data_ptr(), t["db"].data_ptr(), B, H, W, code
        for key, v in over.items():
            setattr(a, key, v(a) if callable(v) else v)
        return a, t

    def refused(rc, t, what):
        torch.cuda.synchronize()
        assert rc != 0 and lib.dd_last_error(), what + ": accepted"
        for key in ("dx", "dw", "db", "y"):
            if key in t:
                assert bool((t[key] == SENTINEL).all()), "%s: %s was written" % (what, key)

    for what, over in (("ld_dy not a multiple of 8", dict(ld_dy=20)),
                       ("misaligned dx", dict(dx=lambda a: a.dx + 2)),
                       ("k_pad < cout with dx", dict(cout=24, k_pad=16))):
        a, t = conv_args(**over)
        refused(lib.dd_conv3x3_bwd(C.byref(a), _stream()), t, what)
    a, t = conv_args()      # sanity: the un-tampered descriptor is accepted, so each refusal above is due to the one field changed
    assert lib.dd_conv3x3_bwd(C.byref(a), _stream()) == 0
    torch.cuda.synchronize()

    args = (L.ConvBwdArgs * 2)()
    a0, t0 = conv_args(dx=None, wd=None)
    a1, t1 = conv_args()      # carries dx
    for dst, src in ((args[0], a0), (args[1], a1)):
        C.memmove(C.byref(dst), C.byref(src), C.sizeof(L.ConvBwdArgs))
    rc = lib.dd_conv3x3_bwd_multi(args, 2, _stream())
    refused(rc, dict(dx=t1["dx"], dw=t1["dw"], db=t1["db"]), "dd_conv3x3_bwd_multi with a problem that carries dx")
    refused(rc, dict(dw=t0["dw"], db=t0["db"]), "dd_conv3x3_bwd_multi with a problem that carries dx (problem 0)")

    def convt_args(cin, cout):
        t = dict(x=torch.zeros(B, H, W, 144, dtype=tdt, device="cuda"), y=torch.full((B, 2 * H, 2 * W, 128), SENTINEL, dtype=tdt, device="cuda"),
                 w=torch.zeros(4 * 144 * 512, dtype=tdt, device="cuda"), dx=torch.full((B, H, W, 144), SENTINEL, dtype=tdt, device="cuda"),
                 dw=torch.full((4 * 128 * 144,), SENTINEL, device="cuda"), db=torch.full((128,), SENTINEL, device="cuda"))
        a = L.ConvTArgs()
        a.x, a.ld_x, a.cin, a.y, a.ld_y, a.cout = t["x"].data_ptr(), 144, cin, t["y"].data_ptr(), 128, cout
        a.w, a.dx, a.ld_dx, a.dw, a.db = t["w"].data_ptr(), t["dx"].data_ptr(), 144, t["dw"].data_ptr(), t["db"].data_ptr()
        a.B, a.H, a.W, a.dtype = B, H, W, code
        return a, t

    for what, cin, cout, fwd in (("convT cout % 16 != 0", 32, 24, True), ("convT cout % 16 != 0", 32, 24, False), ("convT forward cout > 96", 32, 112, True),
                                 ("convT cin > 128", 136, 32, True), ("convT cin > 128", 136, 32, False)):
        a, t = convt_args(cin, cout)
        if fwd:
            a.n_pad, a.k_pad = 4 * 112, 128
            refused(lib.dd_convt2x2_fwd(C.byref(a), _stream()), t, what + " (forward)")
        else:
            a.n_pad, a.k_pad = 144, 128
            refused(lib.dd_convt2x2_bwd(C.byref(a), _stream()), t, what + " (backward)")
    # controls: the nearest legal channel counts with the very same buffers, strides and pack dimensions are accepted and write their outputs,
    # so each refusal above is due to the channel count its label names (a forward with cin > 128 has no legal k_pad at all: k_pad <= 128)
    for cin, cout, fwd in ((32, 32, True), (32, 96, True), (128, 32, True), (32, 32, False), (128, 32, False)):
        a, t = convt_args(cin, cout)
        if fwd:
            a.n_pad, a.k_pad = 4 * 112, 128
            assert lib.dd_convt2x2_fwd(C.byref(a), _stream()) == 0, (cin, cout, lib.dd_last_error())
            torch.cuda.synchronize()
            assert bool((t["y"][..., :cout] == 0).all()) and bool((t["y"][..., cout:] == SENTINEL).all())
        else:
            a.n_pad, a.k_pad = 144, 128
            assert lib.dd_convt2x2_bwd(C.byref(a), _stream()) == 0, (cin, cout, lib.dd_last_error())
            torch.cuda.synchronize()
            assert bool((t["dx"][..., :cin] == 0).all()) and bool((t["dw"][:4 * cout * cin] == SENTINEL).all())      # (dw += 0: atomics onto the fill)
