"""-m gpu: the fused kernel-prediction head launches op by op through the C-ABI -- dd_kpcn_head_fwd, dd_kpcn_head_bwd, dd_kpcn_head_bwd_multi
(csrc/dd_head.hip) -- against the float64 reference and the per-element error budget of tests/head_ref.py.  No Graph is built: every argument
struct is filled by hand.

THE GATE is elementwise on every element of every output (head_ref.py): a few fp32 ulps where no intermediate rounding of the kernel can fall the
other way, ZERO for dx there (the stored bits must be the reference's), and one storage ulp's worth, carried through the weights, exactly where it
can.  The worst error / gate of every output is printed and recorded (gpu_util.gate, bound 1) and asserted to be < 1.  tests/test_head_ref.py shows
on the CPU, for these very inputs, that an fp32 evaluation stays within the gates and that 19 plausible mistakes of the kernel do not.

Every device buffer sits between sentinels: x is a channel window of a wider row (ldx = C + 8 or C + 24) whose other channels hold NaN, src and
dout carry a NaN in their fourth channel (ldsrc = ld_dout = 4), out has ld_out = 4 and dx ld_dx = C + 4 with sentinel channels that must stay,
the fp32 weights, biases and gradients lie between guard words.  Inputs, guards and unused channels must be bit-unchanged after every launch."""
import ctypes as C

import pytest
import torch

import conv_ops_util as U
import head_ref as R
from deepdenoiser_amd import _lib as L

pytestmark = pytest.mark.gpu
SENTINEL, G, View, Guarded = U.SENTINEL, U.G, U.View, U.Guarded
DT = {k: U.DT[k] for k in R.DTYPES}
GRADS = ("dwa", "dba", "dwb", "dbb")
WORST = {}      # (output, storage type) -> worst error / gate of the session, printed by the last test of the file


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _gated(name, key, got, ref, gate):
    w = U.gated(name, got, ref, gate)
    assert w < 1.0, "%s: worst error / gate %.4f" % (name, w)
    WORST[key] = max(WORST.get(key, 0.0), w)
    return w


class Problem:
    """The device buffers of one head problem (a row of head_ref.CASES, a storage type, an input kind)."""

    def __init__(self, case, dtype, kind, wide=False):
        self.case, self.dtype, self.kind = case, dtype, kind
        self.ks, self.C, self.N, self.H, self.W, _ = case
        self.K = self.ks * self.ks
        self.inp = inp = R.head_inputs(case, dtype, kind)
        tdt = DT[dtype][1]
        shape, Cc = (self.N, self.H, self.W), self.C
        # x: channels [off, off + C) of a row of C + 8 (off 8) or C + 24 (off 16) channels; every other channel a NaN of the storage type
        self.x = View(shape, Cc, Cc, Cc + (24 if wide else 8), 16 if wide else 8, dtype, inp["x"])
        self.x.buf[..., :self.x.off] = float("nan")
        self.x.buf[..., self.x.off + Cc:] = float("nan")
        self.x.before = self.x.buf.clone()
        self.npix = self.N * self.H * self.W
        nan4 = lambda v: torch.cat([v, torch.full(v.shape[:-1] + (1,), float("nan"), dtype=v.dtype)], -1)      # noqa: E731
        self.src, self.dout = Guarded(self.npix * 4, nan4(inp["src"])), Guarded(self.npix * 4, nan4(inp["dout"]))
        self.w = {k: Guarded(inp[k].numel(), inp[k]) for k in ("wa", "ba", "wb", "bb")}
        self.inputs = [self.src, self.dout] + list(self.w.values())
        self.inputs_before = [_bits32(t.buf).clone() for t in self.inputs]
        self.name = "%s %s %s" % (R.case_id(case), dtype, kind)

    def args(self, a=None):
        a = a if a is not None else L.HeadArgs()
        a.x, a.ldx, a.C, a.src, a.ldsrc = self.x.ptr, self.x.ld, self.C, self.src.ptr, 4
        a.wa, a.ba, a.wb, a.bb = self.w["wa"].ptr, self.w["ba"].ptr, self.w["wb"].ptr, self.w["bb"].ptr
        a.N, a.H, a.W, a.ksize, a.dtype = self.N, self.H, self.W, self.ks, DT[self.dtype][0]
        return a

    def forward_buffers(self, a):
        self.out = Guarded(self.npix * 4, torch.full((self.npix * 4,), SENTINEL))
        a.out, a.ld_out = self.out.ptr, 4
        return a

    def backward_buffers(self, a, accumulate, prefilled):
        inp = self.inp
        self.dx = View((self.N, self.H, self.W), self.C, self.C, self.C + 4, 0, self.dtype, inp["dx_old"] if accumulate else None)
        if not accumulate:
            self.dx.buf[..., :self.C] = SENTINEL      # every element must be written
        self.g = {k: Guarded(inp["w_old_" + k].numel(), inp["w_old_" + k] if prefilled else None) for k in GRADS}
        a.dout, a.ld_dout, a.dx, a.ld_dx, a.accumulate_dx = self.dout.ptr, 4, self.dx.ptr, self.dx.ld, int(accumulate)
        a.dwa, a.dba, a.dwb, a.dbb = (self.g[k].ptr for k in GRADS)
        return a

    def reference(self, accumulate=False, prefilled=False):
        return R.head_reference(self.case, self.dtype, self.kind, accumulate, prefilled)

    def inputs_intact(self):
        ok = self.x.unchanged() and all(t.guards_intact() for t in self.inputs)
        return ok and all(torch.equal(_bits32(t.buf), b) for t, b in zip(self.inputs, self.inputs_before))

    def check_forward(self, tag=""):
        ref = self.reference()
        name = "head_fwd%s %s" % (tag, self.name)
        assert self.inputs_intact(), name + ": an input or a guard word was written"
        o = self.out.values().reshape(self.N, self.H, self.W, 4)
        assert self.out.guards_intact() and bool((o[..., 3] == SENTINEL).all()), name + ": the fourth channel of out or a guard word was written"
        _gated(name + " out", ("out", self.dtype), o[..., :3], ref["out"], ref["gate_out"])      # (finite despite the NaN neighbours: U.gated asserts it)

    def check_backward(self, accumulate, prefilled, tag=""):
        ref = self.reference(accumulate, prefilled)
        name = "head_bwd%s %s acc%d pre%d" % (tag, self.name, accumulate, prefilled)
        assert self.inputs_intact(), name + ": an input or a guard word was written"
        assert self.dx.neighbours_intact(), name + ": channels >= C of the ld_dx row were written"
        got = self.dx.values()
        _gated(name + " dx", ("dx", self.dtype), got, ref["dx"], ref["gate_dx"])
        if not accumulate:      # masked positions: exactly +0 (all 16 bits clear)
            masked = ~R.positive16(self.inp["x"])
            raw = U.bits(self.dx.buf[..., :self.C].cpu())
            assert bool((raw[masked] == 0).all()), name + ": a masked dx is not +0"
        for k in GRADS:
            assert self.g[k].guards_intact(), "%s %s: a guard word was written" % (name, k)
            _gated("%s %s" % (name, k), (k, self.dtype), self.g[k].values().reshape(ref[k].shape), ref[k], ref["gate_" + k])
        return self.dx.buf.clone()


def _run_case(lib, case, dtype, kind, wide):
    p = Problem(case, dtype, kind, wide)
    L.check(lib.dd_kpcn_head_fwd(C.byref(p.forward_buffers(p.args())), U.stream()))
    torch.cuda.synchronize()
    p.check_forward()
    for accumulate, prefilled in ((False, False), (True, True)):
        L.check(lib.dd_kpcn_head_bwd(C.byref(p.backward_buffers(p.args(), accumulate, prefilled)), U.stream()))
        torch.cuda.synchronize()
        p.check_backward(accumulate, prefilled)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_head_forward_and_backward(lib, case, dtype):
    """Every row of head_ref.CASES in every input kind it runs: forward; backward into zeroed gradient buffers with dx overwritten; backward into
    buffers that hold a known pattern with dx accumulated (the twice-rounded reference).  The grid-exact kind runs under gates of a few fp32 ulps."""
    _need_gpu()
    for i, kind in enumerate(R.kinds_of(case)):
        _run_case(lib, case, dtype, kind, wide=(R.CASES.index(case) + i) % 2 == 1)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("cases", R.MULTI, ids=["+".join(R.case_id(c) for c in m) for m in R.MULTI])
def test_head_backward_multi(lib, cases, dtype):
    """dd_kpcn_head_bwd_multi with 2 and 3 problems of one kernel size -- a 4- or 2-pixel problem next to one of several workgroups, the second
    problem accumulating into dx -- each against the float64 reference; and dx bit-identical to the problems' own launches."""
    _need_gpu()
    n = len(cases)
    kinds = ["grid-exact" if c in R.EXACT_CASES and i != 1 else "real" if i == 1 else "grid" for i, c in enumerate(cases)]
    probs = [Problem(c, dtype, k, wide=i % 2 == 0) for i, (c, k) in enumerate(zip(cases, kinds))]
    arr = (L.HeadArgs * n)()
    for i, p in enumerate(probs):
        p.backward_buffers(p.args(arr[i]), accumulate=i == 1, prefilled=i == 1)
    L.check(lib.dd_kpcn_head_bwd_multi(arr, n, U.stream()))
    torch.cuda.synchronize()
    multi_dx = [p.check_backward(i == 1, i == 1, " multi %dof%d" % (i, n)) for i, p in enumerate(probs)]
    for i, p in enumerate(probs):
        L.check(lib.dd_kpcn_head_bwd(C.byref(p.backward_buffers(p.args(), i == 1, i == 1)), U.stream()))
        torch.cuda.synchronize()
        assert torch.equal(U.bits(p.dx.buf), U.bits(multi_dx[i])), "problem %d: dx of the multi launch differs from the single launch" % i


# ---------------------------------------------------------------------------------------------------------------- the fast exponential
@pytest.mark.parametrize("ks", [5, 3])
def test_fast_exponential_stays_within_its_allowance(lib, ks):
    """head_ref.EXP_REL is an assumption about __expf.  dd_kpcn_fwd runs the same intrinsic in the same softmax (csrc/dd_pointwise.hip) and has its
    own test; here its source is a comb of ones -- every ks x ks window of an interior pixel holds exactly one 1 per channel -- so out[y, x, c] IS
    one probability of that pixel, and its relative error against float64 is compared with the softmax allowance of head_ref.evaluate WITHOUT its
    factor 2: EXP_REL(arg_t) + max_u EXP_REL(arg_u) + u |arg_t| + SOFTMAX_F32_TERMS u.  The logits are storage-representable (both types).
    MEASURED 2026-10-20 on an MI355X (worst relative error of a probability; worst error / allowance): ks 5 bf16 1.085e-6 = 18.2 u at argument
    -12.06, 0.174; ks 5 f16 1.052e-6, 0.149; ks 3 bf16 9.72e-7, 0.158; ks 3 f16 8.76e-7, 0.141 -- the assumed allowance stands."""
    _need_gpu()
    B, H, W, K, P = 1, 45, 50, ks * ks, (ks - 1) // 2
    gen = torch.Generator().manual_seed(ks)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    src = torch.zeros(B, H, W, 4)
    for c, (a, b) in enumerate(((0, 0), (1, ks - 1), (ks - 1, 2))):
        src[0, :, :, c] = ((yy % ks == a) & (xx % ks == b)).float()
    for dtype in R.DTYPES:
        code, tdt = DT[dtype]
        lg = R.representable(torch.randn(B, H, W, 32, generator=gen, dtype=torch.float64) * 3.0, dtype)
        out, src_d, lg_d = torch.zeros(B, H, W, 3, device="cuda"), src.cuda(), lg.to(tdt).cuda()
        L.check(lib.dd_kpcn_fwd(src_d.data_ptr(), 4, lg_d.data_ptr(), 32, out.data_ptr(), 3, B, H, W, ks, code, U.stream()))
        torch.cuda.synchronize()
        arg = lg[..., :K] - lg[..., :K].max(-1, keepdim=True).values
        p = torch.softmax(lg[..., :K], -1)
        tp = R.gather_taps(src[..., :3].double(), ks)                      # [B, H, W, K, 3]: one 1 per channel in the interior
        inner = (slice(None), slice(P, H - P), slice(P, W - P))
        assert bool((tp[inner].sum(-2) == 1).all())
        want = (p[..., None] * tp).sum(-2)[inner]
        a_t = (arg[..., None] * tp).sum(-2)[inner]                         # the argument of the probability each output shows
        er_max = R.EXP_REL(arg).max(-1, keepdim=True).values.expand(B, H, W, 3)[inner]
        allowed = R.EXP_REL(a_t) + er_max + R.U * a_t.abs() + R.SOFTMAX_F32_TERMS * R.U
        rel = (out.double().cpu()[inner] - want).abs() / want
        worst = float((rel / allowed).max())
        print("__expf through dd_kpcn_fwd, ks %d %s: worst relative error of a probability %.3e (%.2f u) at argument %.2f; worst error / allowance %.3f over %d values, arguments down to %.1f"
              % (ks, dtype, float(rel.max()), float(rel.max()) / R.U, float(a_t.reshape(-1)[rel.reshape(-1).argmax()]), worst, rel.numel(), float(a_t.min())))
        U.gate("EXP_REL allowance ks %d %s" % (ks, dtype), worst, 1.0)
        assert worst < 1.0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(lib):
    _need_gpu()
    case = (5, 16, 1, 4, 4, "")
    kept = []

    def problem(n=1, **over):
        arr = (L.HeadArgs * n)()
        ps = []
        for i in range(n):
            p = Problem(case, "bf16", "grid")
            p.backward_buffers(p.forward_buffers(p.args(arr[i])), False, False)
            for t in p.g.values():
                t.buf[:] = SENTINEL
            ps.append(p)
        for key, v in over.items():
            setattr(arr[0], key, v(arr[0]) if callable(v) else v)
        kept.append(ps)
        return arr, ps

    def untouched(ps, what):
        torch.cuda.synchronize()
        for p in ps:
            assert bool((p.out.buf == SENTINEL).all()) and bool((p.dx.buf == SENTINEL).all()), what + ": out or dx was written"
            assert all(bool((t.buf == SENTINEL).all()) for t in p.g.values()), what + ": a gradient buffer was written"
            assert p.inputs_intact(), what

    def refused(rc, ps, what):
        assert rc != 0 and lib.dd_last_error(), what + ": accepted"
        untouched(ps, what)

    both = (("f32 storage", dict(dtype=L.DD_F32)), ("ks = 7", dict(ksize=7)), ("C = 12", dict(C=12)), ("C = 136", dict(C=136, ldx=136, ld_dx=136)),
            ("ldx < C", dict(ldx=8)), ("ldx % 8 != 0", dict(ldx=28)), ("x misaligned by 8 bytes", dict(x=lambda a: a.x + 8)), ("H < P", dict(H=1)),
            ("N H W = 2^31", dict(N=65536, H=256, W=128)), ("H W ldsrc = 2^32", dict(N=1, H=32768, W=32768)))
    for what, over in both:
        arr, ps = problem(**over)
        refused(lib.dd_kpcn_head_fwd(arr, U.stream()), ps, "forward, " + what)
        refused(lib.dd_kpcn_head_bwd(arr, U.stream()), ps, "backward, " + what)
        arr2, ps2 = problem(2, **over)
        refused(lib.dd_kpcn_head_bwd_multi(arr2, 2, U.stream()), ps2, "multi, " + what)
    arr, ps = problem(out=None)
    refused(lib.dd_kpcn_head_fwd(arr, U.stream()), ps, "forward, null out")
    for what, over in (("ld_dx % 4 != 0", dict(ld_dx=22)), ("null dwa", dict(dwa=None)), ("dx misaligned by 4 bytes", dict(dx=lambda a: a.dx + 4))):
        arr, ps = problem(**over)
        refused(lib.dd_kpcn_head_bwd(arr, U.stream()), ps, "backward, " + what)
        arr2, ps2 = problem(2, **over)
        refused(lib.dd_kpcn_head_bwd_multi(arr2, 2, U.stream()), ps2, "multi, " + what)
    arr, ps = problem(4)
    refused(lib.dd_kpcn_head_bwd_multi(arr, 4, U.stream()), ps, "multi, n = 4")
    arr, ps = problem(2, ksize=3)
    refused(lib.dd_kpcn_head_bwd_multi(arr, 2, U.stream()), ps, "multi, mixed kernel sizes")
    arr, ps = problem(2, dtype=L.DD_F16)
    refused(lib.dd_kpcn_head_bwd_multi(arr, 2, U.stream()), ps, "multi, mixed storage types")
    # control: the untampered descriptors are accepted, so each refusal above is due to the one field changed
    arr, ps = problem()
    assert lib.dd_kpcn_head_fwd(arr, U.stream()) == 0 and lib.dd_kpcn_head_bwd(arr, U.stream()) == 0, lib.dd_last_error()
    arr2, ps2 = problem(2)
    assert lib.dd_kpcn_head_bwd_multi(arr2, 2, U.stream()) == 0, lib.dd_last_error()
    torch.cuda.synchronize()
    assert not bool((ps[0].out.values().reshape(-1, 4)[:, :3] == SENTINEL).any()) and not bool((ps2[1].dx.values() == SENTINEL).any())


def test_worst_ratios_of_the_session():
    """Prints the worst error / gate per output and storage type over the tests of this file that ran before it (the figures of the change's description)."""
    _need_gpu()
    for key in sorted(WORST):
        print("head ops, worst error / gate: %-4s %-5s %.3f" % (key + (WORST[key],)))
    assert all(v < 1.0 for v in WORST.values())
