"""-m gpu: the launches whose channel count is not the one their kernel was laid out for, op by op through the C-ABI, against the float64
references and elementwise gates of tests/conv_fwd_ref.py (no new tolerance).

conv_rw8_kernel with ONE K chunk (csrc/dd_conv_rw.hip): a plain 3x3 forward with 17..32 input channels in a 32-channel weight image.  Which
instantiation ran is asserted: the route counter rw8_kc2 moves by one for every call the family takes, and its sub-count rw8_k32
(deepdenoiser_amd._lib.subroute_counts) moves with it exactly when the one-chunk kernel ran -- 16 and 40 input channels, either side of the
border, must not move it.  dd_conv_igemm takes input channels in 16-byte groups (cin % 8 == 0 in 2-byte storage, a refusal otherwise), so a
17-channel layer reaches it the way the engine stages it: cin = 24, seven zero channels in x, a weight image packed from 17 columns.  The raw
cin = 17 is shown to be refused.  The one-chunk output must equal, bit for bit, what the two-chunk kernel stores for the same call
(DD_CONV_RW8_K32=0 is read once per process: a child process computes it)."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":      # the child of the bit-identity test
    sys.path.insert(0, ROOT)

import conv_bwd_ref as R      # noqa: E402
import conv_fwd_ref as F      # noqa: E402
import conv_ops_util as U      # noqa: E402
from deepdenoiser_amd import _lib as L      # noqa: E402
from gpu_util import ACC32, ROUND, check      # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL, View, Guarded = U.SENTINEL, U.View, U.Guarded
K32_ON = F._on(os.environ, "DD_CONV_RW8_K32") and F._on(os.environ, "DD_CONV_RW8") and F._on(os.environ, "DD_CONV_RW")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------------------------- conv_rw8_kernel<KC = 1>
GRIDS = {"one_tile": (2, 16, 16), "ragged_18x20": (2, 18, 20), "ragged_33x17": (2, 33, 17)}
MANY_TILES = (3, 150, 157)      # 3 x 10 x 10 tiles of 16 x 16: more than the workgroups of the launch (one per CU), so both LDS buffers turn over


@functools.lru_cache(maxsize=None)
def fwd_case(cin, n, grid, epi, dtype):
    """Inputs (values of the storage type) and the float64 reference of one plain forward call; epi: bias and ReLU, or neither."""
    g = F._gen("ragged fwd", cin, n, grid, dtype)      # (not of epi: both epilogues see the same operands)
    x = F.values_of(F._signed(grid + (cin,), g), dtype)
    w = F.values_of(torch.randn(9, n, cin, generator=g, dtype=F.F64) / math.sqrt(9 * cin), dtype)
    bias = torch.randn(n, generator=g, dtype=F.F64).float().to(F.F64)
    ref = F.conv_fwd(x, w, bias if epi else None, taps=9, flags=F.DD_OUT_RELU if epi else 0, nbias=n)
    return x, w, bias, ref


def run_fwd(lib, cin, n, grid, epi, dtype, expect_k32):
    """One dd_conv_igemm call laid out as tests/test_gpu_conv_fwd_ops.py lays its calls out.  Returns the output view."""
    x, w, bias, ref = fwd_case(cin, n, grid, epi, dtype)
    cs = F.round_up(cin, 8)      # staged channels: what the call names as cin
    name = "conv_igemm [rw8 one K chunk] %d->%d %s %s %s" % (cin, n, "x".join(map(str, grid)), "bias relu" if epi else "plain", dtype)
    xv = View(grid, cin, cs, cs + 16, 8, dtype, x)
    yv = View(grid, n, n, F.round_up(n, 8) + 24, 16, dtype, None, SENTINEL)
    yv.buf[..., yv.off:yv.off + n] = SENTINEL      # every element must be written
    n_pad, k_pad = F.round_up(n, 16), F.round_up(cs, 32)
    wp = U.pack_image(lib, name, w.reshape(-1), dtype, 9, n, cin, n_pad, k_pad, n * cin, cin, 1, 0)
    wp_before = wp.clone()
    bv = Guarded(n, bias) if epi else None
    a = L.ConvArgs()
    a.x, a.ldx, a.cin, a.wp, a.k_pad, a.n_pad = xv.ptr, xv.ld, cs, wp.data_ptr(), k_pad, n_pad
    if bv:
        a.bias, a.nbias = bv.ptr, n
    a.y, a.ldy, a.n, a.B, a.H, a.W, a.taps, a.flags, a.dtype = yv.ptr, yv.ld, n, grid[0], grid[1], grid[2], 9, F.DD_OUT_RELU if epi else 0, U.DT[dtype][0]
    route = F.igemm_route(F.IgemmCase(name, 9, cs, n, grid, a.flags, nbias=n if epi else None), dtype, os.environ)      # the restated dispatch
    before, sub_before = L.route_counts(), L.subroute_counts()
    L.check(lib.dd_conv_igemm(C.byref(a), U.stream()))
    torch.cuda.synchronize()
    after, sub_after = L.route_counts(), L.subroute_counts()
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert moved == {route: 1}, "%s: expected route %s, counters moved: %s" % (name, route, moved)
    assert route == "rw8_kc2" or not expect_k32, name + ": the case was meant for conv_rw8_kernel"
    assert sub_after["rw8_k32"] - sub_before["rw8_k32"] == (1 if expect_k32 else 0), "%s: one-chunk launches %d" % (name, sub_after["rw8_k32"] - sub_before["rw8_k32"])
    assert xv.unchanged(), name + ": the input buffer was written"
    assert torch.equal(wp.view(torch.uint8), wp_before.view(torch.uint8)), name + ": the weight image was written"
    assert not bv or (bv.guards_intact() and torch.equal(bv.values(), bias)), name + ": the bias was written"
    U.gated(name + " y", yv.values(), ref["y"], F.gate_y(ref, dtype, route))
    check(name + " y rel-L2", yv.values(), ref["y"], ROUND[dtype])
    assert yv.neighbours_intact(), name + ": a channel outside the view was written"
    return yv


@pytest.mark.parametrize("dtype", F.DTYPES2)
@pytest.mark.parametrize("epi", (True, False), ids=("bias_relu", "plain"))
@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("n", (48, 64, 96))
@pytest.mark.parametrize("cin", (17, 24, 32))
def test_first_conv_on_one_k_chunk(cin, n, grid, epi, dtype):
    _need_gpu()
    run_fwd(L.load(), cin, n, GRIDS[grid], epi, dtype, expect_k32=K32_ON)


@pytest.mark.parametrize("dtype", F.DTYPES2)
@pytest.mark.parametrize("cin", (16, 40))
def test_the_borders_stay_off_the_one_chunk_kernel(cin, dtype):
    """16 input channels: not a register-weight layer at all; 40: conv_rw8_kernel<KC = 2> (a 64-channel weight image)."""
    _need_gpu()
    run_fwd(L.load(), cin, 64, GRIDS["ragged_18x20"], True, dtype, expect_k32=False)


@pytest.mark.parametrize("dtype", F.DTYPES2)
def test_one_k_chunk_with_more_tiles_than_workgroups(dtype):
    _need_gpu()
    run_fwd(L.load(), 32, 64, MANY_TILES, True, dtype, expect_k32=K32_ON)


def test_seventeen_raw_input_channels_are_refused():
    """What `cin 17` cannot mean: dd_conv_igemm takes 16-byte channel groups; nothing is launched, nothing written."""
    _need_gpu()
    lib = L.load()
    t = dict(x=torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16, device="cuda"), wp=torch.zeros(9 * 48 * 32, dtype=torch.bfloat16, device="cuda"),
             y=torch.full((1, 4, 4, 48), SENTINEL, dtype=torch.bfloat16, device="cuda"))
    a = L.ConvArgs()
    a.x, a.ldx, a.cin, a.wp, a.k_pad, a.n_pad = t["x"].data_ptr(), 32, 17, t["wp"].data_ptr(), 32, 48
    a.y, a.ldy, a.n, a.B, a.H, a.W, a.taps, a.flags, a.dtype = t["y"].data_ptr(), 48, 48, 1, 4, 4, 9, 0, L.DD_BF16
    before = (L.route_counts(), L.subroute_counts())
    assert lib.dd_conv_igemm(C.byref(a), U.stream()) == -1 and b"cin=17" in lib.dd_last_error()
    torch.cuda.synchronize()
    assert (L.route_counts(), L.subroute_counts()) == before and bool((t["y"] == SENTINEL).all())


BIT_CASE = (24, 96, (2, 33, 17), True)      # two output-channel blocks, ragged edges, bias and ReLU


@pytest.mark.parametrize("dtype", F.DTYPES2)
def test_one_k_chunk_is_bit_identical_to_two(dtype, tmp_path):
    """The same call in a child process with DD_CONV_RW8_K32=0 (there: conv_rw8_kernel<KC = 2>, asserted by the sub-count) and here: the whole
    output buffers -- values, pad channels, sentinels -- are equal bit for bit."""
    _need_gpu()
    if not K32_ON:
        pytest.skip("the one-chunk kernel is switched off in this process")
    out = str(tmp_path / "kc2.pt")
    env = dict(os.environ, DD_CONV_RW8_K32="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), dtype, out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child failed\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:])
    yv = run_fwd(L.load(), *BIT_CASE, dtype, expect_k32=True)
    two = torch.load(out)
    assert torch.equal(yv.buf.cpu().view(torch.int16), two.view(torch.int16)), "KC = 1 and KC = 2 outputs differ in %d elements" % int(
        (yv.buf.cpu().view(torch.int16) != two.view(torch.int16)).sum())


# ---------------------------------------------------------------------------------------------------------------- convt_bwd_kernel<NSD = 2>
# dd_convt2x2_bwd with 65..96 output channels: one launch of the two-slice geometry (tiles of 8 x 4 input pixels) -- or, in a process started
# with DD_CONVT_BWD_WIDE=0, one launch per 64 output channels, the second accumulating into dx.  Reference, budget and gate are those of
# tests/test_gpu_conv_bwd_ops.py for this call (conv_bwd_ref.convt_bwd: half a storage ulp per per-64 rounding point), for both paths.  The
# one launch rounds dx where the two round it -- a single rounding of the whole sum leaves that gate (fp32 emulation on the CPU: up to 1.2 of
# it in bf16 with accumulate) -- so dx cannot tell the paths apart: dd_convt_bwd_wide_count does, and the two paths' dx are compared bit for bit.
WIDE_ON = F._on(os.environ, "DD_CONVT_BWD_WIDE")
PAD_OLD = 0.5
CONVT_GRIDS = {"8x8": (1, 8, 8), "ragged_5x9": (1, 5, 9)}
CONVT_LOOP = (128, 96, 5, 64, 64)      # 320 tiles of 8 x 8 (640 of 8 x 4): more than the workgroups, every workgroup loops


def run_convt_bwd(lib, shape, dtype, mask, acc):
    cin, cout, B, H, W = shape
    cinv = R.round_up(cin, 8)
    x, dy, k, _, old = R.convt_inputs(shape, dtype)
    ref = R.convt_bwd_reference(shape, dtype, mask, acc)
    name = "convt2x2_bwd [%s] %s %s mask%d acc%d" % ("one launch" if WIDE_ON else "per-64", "x".join(map(str, shape)), dtype, mask, acc)
    xv = View((B, H, W), cin, cinv, cinv + 16, 8, dtype, x)
    dyv = View((B, 2 * H, 2 * W), cout, cout, cout + 24, 16, dtype, dy)
    dxv = View((B, H, W), cin, cinv, cinv + 12, 4, dtype, old if acc else None, PAD_OLD if acc else SENTINEL)
    if not acc:
        dxv.buf[..., dxv.off:dxv.off + cin] = SENTINEL      # every element must be written
    w, n_pad, k_pad = U.pack(lib, "convT2", "dgrad", k, cin, cout, dtype)
    w_before = w.clone()
    dw, db = Guarded(4 * cout * cin), Guarded(cout)
    a = L.ConvTArgs()
    a.x, a.ld_x, a.cin, a.y, a.ld_y, a.cout = xv.ptr, xv.ld, cin, dyv.ptr, dyv.ld, cout
    a.w, a.n_pad, a.k_pad = w.data_ptr(), n_pad, k_pad
    a.dx, a.ld_dx, a.dw, a.db, a.use_mask, a.accumulate = dxv.ptr, dxv.ld, dw.ptr, db.ptr, mask, acc
    a.B, a.H, a.W, a.dtype = B, H, W, U.DT[dtype][0]
    wide_before = lib.dd_convt_bwd_wide_count()
    L.check(lib.dd_convt2x2_bwd(C.byref(a), U.stream()))
    torch.cuda.synchronize()
    assert lib.dd_convt_bwd_wide_count() - wide_before == (1 if WIDE_ON else 0), name + ": one-launch calls %d" % (lib.dd_convt_bwd_wide_count() - wide_before)
    assert xv.unchanged() and dyv.unchanged() and torch.equal(U.bits(w), U.bits(w_before)), name + ": an input buffer was written"
    U.gated(name + " dx", dxv.values(), ref["dx"], R.gate_storage(ref["dx"], ref["dx_budget"], dtype, ref["dx_points"]))
    check(name + " dx rel-L2", dxv.values(), ref["dx"], ROUND[dtype])
    assert dxv.neighbours_intact(), name + ": a channel outside the dx view was written"
    if cinv > cin:
        assert bool((dxv.pads() == (PAD_OLD if acc else 0.0)).all()), name + ": pad channels cin..cinv-1 of dx"
    for key, arr in (("dw", dw), ("db", db)):
        U.gated("%s %s" % (name, key), arr.values().reshape(ref[key].shape), ref[key], R.gate_f32(ref[key + "_budget"]))
        check("%s %s rel-L2" % (name, key), arr.values().reshape(ref[key].shape), ref[key], ACC32[dtype])
        assert arr.guards_intact(), "%s %s: a guard word was written" % (name, key)
    return dxv


@pytest.mark.parametrize("dtype", F.DTYPES2)
@pytest.mark.parametrize("flags", R.FLAGS, ids=["mask%d_acc%d" % f for f in R.FLAGS])
@pytest.mark.parametrize("grid", sorted(CONVT_GRIDS))
@pytest.mark.parametrize("cin", (72, 96, 128))
@pytest.mark.parametrize("cout", (80, 96))
def test_convt2x2_bwd_65_to_96_output_channels(cout, cin, grid, flags, dtype):
    _need_gpu()
    run_convt_bwd(L.load(), (cin, cout) + CONVT_GRIDS[grid], dtype, *flags)


@pytest.mark.parametrize("dtype", F.DTYPES2)
def test_convt2x2_bwd_65_to_96_every_workgroup_loops(dtype):
    _need_gpu()
    cin, cout, B, H, W = CONVT_LOOP
    assert B * (H // 8) * (W // 8) == 320 > torch.cuda.get_device_properties(0).multi_processor_count
    for mask, acc in ((0, 0), (1, 1)):
        run_convt_bwd(L.load(), CONVT_LOOP, dtype, mask, acc)


CONVT_CHILD = (96, 80, 1, 5, 9)


def test_convt2x2_bwd_65_to_96_as_two_launches(tmp_path):
    """DD_CONVT_BWD_WIDE=0 (read once per process: a child): the loop over blocks of 64 output channels passes the same gate, all four
    epilogues, both storage types (that the loop ran: the counter stays); the one launch here stores the same dx buffers bit for bit."""
    _need_gpu()
    if not WIDE_ON:
        pytest.skip("the one-launch kernel is switched off in this process")
    out = str(tmp_path / "two_launches.pt")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "convt", out], env=dict(os.environ, DD_CONVT_BWD_WIDE="0"), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, "child failed\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.count("[per-64]") >= 8 * 3, p.stdout[-2000:]
    two = torch.load(out)
    for dtype in F.DTYPES2:
        for mask, acc in R.FLAGS:
            one = run_convt_bwd(L.load(), CONVT_CHILD, dtype, mask, acc).buf.cpu()
            assert torch.equal(one.view(torch.int16), two[(dtype, mask, acc)].view(torch.int16)), "dx of one launch and of two differ: %s mask%d acc%d" % (dtype, mask, acc)


if __name__ == "__main__":
    if sys.argv[1] == "convt":
        assert not WIDE_ON, "the child runs with DD_CONVT_BWD_WIDE=0"
        torch.save({(child_dtype, child_mask, child_acc): run_convt_bwd(L.load(), CONVT_CHILD, child_dtype, child_mask, child_acc).buf.cpu()
                    for child_dtype in F.DTYPES2 for child_mask, child_acc in R.FLAGS}, sys.argv[2])
    else:
        assert not K32_ON, "the child runs with DD_CONV_RW8_K32=0"
        view = run_fwd(L.load(), *BIT_CASE, sys.argv[1], expect_k32=False)
        torch.save(view.buf.cpu(), sys.argv[2])
