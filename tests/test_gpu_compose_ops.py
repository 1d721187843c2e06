"""-m gpu: the fused compose net op by op through the C-ABI -- dd_compose_net_fwd (the row-streaming kernel of csrc/dd_compose_stream.hip and
the 16x16-tile kernel of csrc/dd_compose.hip) and dd_compose_net_bwd (the two streaming launches of csrc/dd_compose_stream_bwd.hip and the tile
kernel) -- with hand-filled ComposeArgs / ComposeBwdArgs, no Graph.

FORWARD: the kernel stores every intermediate (save_netin, save_act[0..4], save_wl), so each stage is gated from the kernel's OWN stored input of
that stage against the float64 reference and the per-element gate of tests/compose_ref.py: one rounding to the storage type plus a derived fp32
accumulation error.  tests/test_compose_ref.py shows on the CPU that an fp32 evaluation in any order stays within these gates and that seventeen
plausible mistakes do not.  Per shape and storage type: (a) everything saved; (b) nothing saved, the inference variant, its out gated with the wl
of (a) and required to be bit-equal to (a)'s (SAVE only guards stores in cs_role / compose_fwd_kernel: both variants share every arithmetic
instruction of the source); (c) on three shapes two partial launches (only save_wl; only save_act[2] plus save_netin -- a tensor is requested
by its pointer, so the others are NULL and there is no buffer of theirs to touch), whose requested tensors and out must be bit-equal to (a)'s.
The tile forward runs the same test functions under ids containing `tile_forward`; the library reads DD_COMPOSE_STREAM once per process, so they
run in the child process of tests/test_gpu_fallbacks.py ("compose_ops_tile_forward") and skip elsewhere, and the streaming ids skip there.

BACKWARD: compose_ref.backward_reference (the storage-emulating oracle under autograd, the kernel fed the oracle's activations) at the gate of
tests/test_gpu_ops.py: rel-L2 2e-4 (a flipped rounding of one parked gradient element moves a 24 x 216 gradient by ~1e-5 of its norm; a dropped
halo column, tap or strip seam shows at >= 1e-3).  The ABI as read in dd_compose_stream_wgrad_launch / compose_bwd_kernel (atomicAdd into dw* /
db*) and deepdenoiser_amd/prediction_head.py (the six layers' gradient slots are shared by every scale transition): weight and bias gradients are
ADDED to what the buffers hold, d_fine is overwritten, d_small is overwritten or accumulated (accumulate_small).

Every buffer sits between sentinels: small, fine, out, dout, d_small, d_fine with ld = 4 (NaN in the fourth channel of inputs, the sentinel in that
of outputs) or ld = 3; saved activations as a 24-channel window of a 32-channel row or plain 24; ld_netin 8 / 16, ld_wl 1 / 2; weights, biases,
gradients and the scratch between guard words.  After every launch inputs, guards and neighbour channels are bit-unchanged and every element of
every requested output has been written."""
import ctypes as C
import os

import pytest
import torch

import compose_ref as R
import conv_ops_util as U
from deepdenoiser_amd import _lib as L
from gpu_util import check, gate

pytestmark = pytest.mark.gpu
SENTINEL, G, View, Guarded = U.SENTINEL, U.G, U.View, U.Guarded
DT = {k: U.DT[k] for k in R.DTYPES}
TILE_PROCESS = os.environ.get("DD_COMPOSE_STREAM", "1")[:1] == "0"      # the library's own reading of the switch (csrc/dd_compose.hip)
WORST = {}      # (stage, storage type, kernel) -> worst error / gate of the session
BWD_TOL = 2e-4
FWD_CASES = [("stream", s) for s in R.FWD_SHAPES] + [("tile_forward", s) for s in R.TILE_FWD_SHAPES]
PARTIAL_SHAPES = {"stream": [(1, 18, 30), (1, 16, 130), (24, 22, 140)], "tile_forward": [(1, 16, 16), (2, 20, 28), (1, 34, 18)]}
TINY_SHAPES = {"stream": [(2, 10, 50), (1, 20, 72), (1, 6, 260)], "tile_forward": [(2, 20, 28)]}


def _need(which):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if which == "tile_forward" and not TILE_PROCESS:
        pytest.skip("DD_COMPOSE_STREAM is not 0 in this process: the tile forward runs in the child process of tests/test_gpu_fallbacks.py")
    if which != "tile_forward" and TILE_PROCESS:
        pytest.skip("DD_COMPOSE_STREAM=0 in this process: the streaming forward does not run here")


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _image(v, ld, fill):
    """[.., 3] fp32 values as rows of ld channels (the fourth: `fill`), flat."""
    v = v.float()
    if ld == 4:
        v = torch.cat([v, torch.full(v.shape[:-1] + (1,), fill, dtype=torch.float32)], -1)
    return v.reshape(-1)


class Images:
    """An fp32 [.., 3] tensor of row length ld between guard words; inputs carry NaN in the fourth channel, outputs the sentinel."""

    def __init__(self, shape, ld, values=None, output=False):
        self.shape, self.ld = tuple(shape), ld
        v = torch.full(self.shape + (3,), SENTINEL) if values is None else values
        self.g = Guarded(v[..., 0].numel() * ld, _image(v, ld, SENTINEL if output else float("nan")))
        self.before = _bits32(self.g.buf).clone()
        self.ptr = self.g.ptr

    def values(self):
        return self.g.values().reshape(self.shape + (self.ld,))[..., :3]

    def raw(self):
        return self.g.buf[G:G + self.g.n].reshape(self.shape + (self.ld,))[..., :3].contiguous().cpu()

    def unchanged(self):
        return torch.equal(_bits32(self.g.buf), self.before)

    def frame_intact(self):
        v = self.g.values().reshape(self.shape + (self.ld,))
        return self.g.guards_intact() and (self.ld == 3 or bool((v[..., 3] == SENTINEL).all()))

    def all_written(self):
        return not bool((self.values() == SENTINEL).any())


class Weights:
    """The twelve fp32 masters between guard words."""

    def __init__(self, tensors):
        self.t = {k: Guarded(v.numel(), v) for k, v in tensors.items()}
        self.before = {k: _bits32(g.buf).clone() for k, g in self.t.items()}

    def unchanged(self):
        return all(torch.equal(_bits32(g.buf), self.before[k]) for k, g in self.t.items())


def _worst(stage, dtype, kernel, name, ratio):
    w = float(ratio.max())
    print("%-72s worst error / gate %.3f over %d elements" % (name, w, ratio.numel()))
    gate(name, w, 1.0)
    assert (w <= 1.0) if stage == "netin" else (w < 1.0), "%s: worst error / gate %.4f" % (name, w)      # (netin: compose_ref.within)
    key = (stage, dtype, kernel)
    WORST[key] = max(WORST.get(key, 0.0), w)


# ---------------------------------------------------------------------------------------------------------------- forward
class Forward:
    def __init__(self, shape, dtype, kind, ld3, wide):
        self.shape, self.dtype, self.ld3 = shape, dtype, ld3
        self.inp = inp = R.compose_inputs(shape, dtype, 0, kind)
        N, H, W = shape
        self.small, self.fine = Images((N, H // 2, W // 2), ld3, inp["small"]), Images((N, H, W), ld3, inp["fine"])
        named = {"w_in": inp["w_in"], "b_in": inp["b_in"], "w_out": inp["w_out"], "b_out": inp["b_out"]}
        for i in range(4):
            named["w_res%d" % i], named["b_res%d" % i] = inp["w_res"][i], inp["b_res"][i]
        self.w = Weights(named)
        self.ld_act, self.off_act = (32, 8) if wide else (24, 0)
        self.ld_netin, self.off_netin = (16, 8) if wide else (8, 0)
        self.ld_wl = 2 if wide else 1
        self.name = "%s %s %s ld3=%d ld_act=%d" % (R.shape_id(shape), dtype, kind, ld3, self.ld_act)

    def launch(self, lib, save=("netin", "a1", "r1", "a2", "r3", "a3", "wl"), mutate=None):
        """One dd_compose_net_fwd into fresh sentinel-filled outputs; returns the status."""
        N, H, W = self.shape
        self.out = Images((N, H, W), self.ld3, None, output=True)
        self.saved = {}
        a = L.ComposeArgs()
        C.memset(C.byref(a), 0, C.sizeof(a))
        a.small, a.ld_small, a.fine, a.ld_fine, a.out, a.ld_out = self.small.ptr, self.ld3, self.fine.ptr, self.ld3, self.out.ptr, self.ld3
        t = self.w.t
        a.w_in, a.b_in, a.w_out, a.b_out = t["w_in"].ptr, t["b_in"].ptr, t["w_out"].ptr, t["b_out"].ptr
        for i in range(4):
            a.w_res[i], a.b_res[i] = t["w_res%d" % i].ptr, t["b_res%d" % i].ptr
        for s in save:
            if s == "netin":
                v = self.saved[s] = View((N, H, W), 8, 8, self.ld_netin, self.off_netin, self.dtype)
                a.save_netin, a.ld_netin = v.ptr, v.ld
            elif s == "wl":
                v = self.saved[s] = View((N, H, W), 1, 1, self.ld_wl, 0, self.dtype)
                a.save_wl, a.ld_wl = v.ptr, v.ld
            else:
                v = self.saved[s] = View((N, H, W), 24, 24, self.ld_act, self.off_act, self.dtype)
                a.save_act[R.ACT_OF[s]], a.ld_act[R.ACT_OF[s]] = v.ptr, v.ld
        a.N, a.H, a.W, a.dtype = N, H, W, DT[self.dtype][0]
        if mutate:
            mutate(a)
        self.args = a
        rc = lib.dd_compose_net_fwd(C.byref(a), U.stream())
        torch.cuda.synchronize()
        return rc

    def frame_checks(self, what):
        assert self.small.unchanged() and self.fine.unchanged() and self.w.unchanged(), what + ": an input or one of its guard words was written"
        assert self.out.frame_intact(), what + ": a guard word or the fourth channel of out was written"
        for s, v in self.saved.items():
            assert v.neighbours_intact(), "%s: a neighbour channel of the saved %s was written" % (what, s)

    def all_written(self, what):
        assert self.out.all_written(), what + ": an element of out was not written"
        for s, v in self.saved.items():
            assert not bool((v.values() == SENTINEL).any()), "%s: an element of the saved %s was not written" % (what, s)

    def got(self):
        g = {s: v.values() for s, v in self.saved.items()}
        g["out"] = self.out.values()
        return g


def _forward_case(lib, which, shape, dtype, kind, ld3, wide):
    kernel = "tile" if which == "tile_forward" else "stream"
    p = Forward(shape, dtype, kind, ld3, wide)
    # (a) everything saved: every stage from the kernel's own stored input
    L.check(p.launch(lib))
    what = "compose_fwd %s %s" % (kernel, p.name)
    p.frame_checks(what)
    p.all_written(what)
    got = p.got()
    ref = R.stage_reference(p.inp, got, kernel)
    for s in R.STAGES:
        _worst(s, dtype, kernel, "%s %s" % (what, s), R.stage_ratio(ref[s], got[s]))
    assert bool((U.bits(p.saved["netin"].buf[..., p.off_netin + 6:p.off_netin + 8].cpu()) == 0).all()), what + ": channels 6, 7 of netin are not +0"
    full = {s: v.buf.clone() for s, v in p.saved.items()}
    out_a = p.out.raw()
    # (b) nothing saved: the inference variant
    L.check(p.launch(lib, save=()))
    p.frame_checks(what + " (no save)")
    p.all_written(what + " (no save)")
    _worst("out", dtype, kernel + " no save", what + " out (no save)", R.stage_ratio(ref["out"], p.out.values()))
    same = torch.equal(_bits32(p.out.raw()), _bits32(out_a))
    print("%s: out of the no-save variant bit-equal to the saving variant's: %s" % (what, same))
    assert same, what + ": the no-save variant's out differs from the saving variant's"
    # (c) partial saves: the requested tensors bit-equal to (a)'s
    if kind == "normal" and shape in PARTIAL_SHAPES[which]:
        for save in (("wl",), ("a2", "netin")):
            L.check(p.launch(lib, save=save))
            p.frame_checks(what + " (partial)")
            assert sorted(p.saved) == sorted(save)
            for s in save:
                assert torch.equal(U.bits(p.saved[s].buf), U.bits(full[s])), "%s: %s of a launch saving %s differs from the full launch's" % (what, s, save)
            assert torch.equal(_bits32(p.out.raw()), _bits32(out_a)), what + ": out of a partial launch differs"


@pytest.mark.parametrize("ld3", [3, 4])
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("which,shape", FWD_CASES, ids=["%s-%s" % (w, R.shape_id(s)) for w, s in FWD_CASES])
def test_compose_forward_stage_by_stage(lib, which, shape, dtype, ld3):
    _need(which)
    wide = (FWD_CASES.index((which, shape)) + ld3) % 2 == 1
    _forward_case(lib, which, shape, dtype, "normal", ld3, wide)
    if shape in TINY_SHAPES[which] and ld3 == 4:      # the small-magnitude kind: f16 activations in the subnormal range
        _forward_case(lib, which, shape, dtype, "tiny", ld3, not wide)


def test_streaming_forward_shapes_cover_the_geometry_on_this_device(lib):
    """The plan of every streaming forward shape with the device's own compute-unit count: the list must still hold every frame width, rows per
    step, strip count, a narrow last strip, ragged bands, a band higher than 4 rows and two shapes with more units than workgroups."""
    _need("stream")
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    rows = {s: dict(zip(R.PLAN_KEYS, R.plan(lib, s, cus))) for s in R.FWD_SHAPES}
    lost = R.coverage_lost(rows, cus)
    for s, p in rows.items():
        print(cus, "CUs", s, p)
    assert not lost, "with %d compute units the forward shapes no longer cover: %s\n%s" % (cus, lost, rows)


# ---------------------------------------------------------------------------------------------------------------- backward
class Backward:
    def __init__(self, shape, dtype, ld3, ld_act):
        self.shape, self.dtype, self.ld3 = shape, dtype, ld3
        self.ref = ref = R.backward_reference(shape, dtype)
        N, H, W = shape
        self.small, self.fine = Images((N, H // 2, W // 2), ld3, ref["small"]), Images((N, H, W), ld3, ref["fine"])
        self.dout = Images((N, H, W), ld3, ref["gout"])
        off = 8 if ld_act == 32 else 0
        self.acts = [View((N, H, W), 24, 24, ld_act, off, dtype, t) for t in ref["acts"]]
        self.wl = View((N, H, W), 1, 1, 2 if ld_act == 32 else 1, 0, dtype, ref["wl"])
        self.w = Weights({n: ref["vars"][n] for n in ref["names"] if n.endswith("/kernel")})
        self.name = "%s %s ld3=%d ld_act=%d" % (R.shape_id(shape), dtype, ld3, ld_act)
        g = torch.Generator().manual_seed(3)
        self.old_small = torch.randn(N, H // 2, W // 2, 3, generator=g).float()
        self.old_w = {n: (torch.randn(ref["vars"][n].shape, generator=g) * 0.5).float() for n in ref["names"]}

    def launch(self, lib, scratch, accumulate, prefilled, mutate=None, scratch_short=0):
        ref = self.ref
        N, H, W = self.shape
        self.d_small = Images((N, H // 2, W // 2), self.ld3, self.old_small if accumulate else None, output=True)
        self.d_fine = Images((N, H, W), self.ld3, None, output=True)
        self.dw = {n: Guarded(ref["vars"][n].numel(), self.old_w[n] if prefilled else None) for n in ref["names"]}
        cb = L.ComposeBwdArgs()
        C.memset(C.byref(cb), 0, C.sizeof(cb))
        cb.small, cb.ld_small, cb.fine, cb.ld_fine, cb.dout, cb.ld_dout = self.small.ptr, self.ld3, self.fine.ptr, self.ld3, self.dout.ptr, self.ld3
        for i, v in enumerate(self.acts):
            cb.act[i], cb.ld_act[i] = v.ptr, v.ld
        cb.wl, cb.ld_wl = self.wl.ptr, self.wl.ld
        lay, wt, dw = R.LAYERS, self.w.t, self.dw
        cb.w_in, cb.dw_in, cb.db_in = wt[lay[0] + "/kernel"].ptr, dw[lay[0] + "/kernel"].ptr, dw[lay[0] + "/bias"].ptr
        for i in range(4):
            cb.w_res[i], cb.dw_res[i], cb.db_res[i] = wt[lay[1 + i] + "/kernel"].ptr, dw[lay[1 + i] + "/kernel"].ptr, dw[lay[1 + i] + "/bias"].ptr
        cb.w_out, cb.dw_out, cb.db_out = wt[lay[5] + "/kernel"].ptr, dw[lay[5] + "/kernel"].ptr, dw[lay[5] + "/bias"].ptr
        cb.d_small, cb.ld_dsmall, cb.accumulate_small, cb.d_fine, cb.ld_dfine = self.d_small.ptr, self.ld3, int(accumulate), self.d_fine.ptr, self.ld3
        cb.N, cb.H, cb.W, cb.dtype = N, H, W, DT[self.dtype][0]
        self.scratch = None
        if scratch:      # exactly dd_compose_bwd_scratch_bytes between two 16-byte guards
            need = int(lib.dd_compose_bwd_scratch_bytes(N, H, W))
            self.scratch = torch.full((need + 32,), 0xFF, dtype=torch.uint8, device="cuda")      # (NaN in either storage type: a read of scratch nobody wrote shows)
            cb.scratch, cb.scratch_bytes = self.scratch.data_ptr() + 16, need - scratch_short
        if mutate:
            mutate(cb)
        rc = lib.dd_compose_net_bwd(C.byref(cb), U.stream())
        torch.cuda.synchronize()
        return rc

    def frame_checks(self, what):
        ok = self.small.unchanged() and self.fine.unchanged() and self.dout.unchanged() and self.w.unchanged()
        ok = ok and all(v.unchanged() for v in self.acts) and self.wl.unchanged()
        assert ok, what + ": an input or one of its guard words / neighbour channels was written"
        assert self.d_small.frame_intact() and self.d_fine.frame_intact(), what + ": a guard word or fourth channel of d_small / d_fine was written"
        assert all(g.guards_intact() for g in self.dw.values()), what + ": a guard word of a weight gradient was written"
        if self.scratch is not None:
            assert bool((self.scratch[:16] == 0xFF).all()) and bool((self.scratch[-16:] == 0xFF).all()), what + ": written outside the scratch"

    def check(self, what, accumulate, prefilled):
        ref = self.ref
        self.frame_checks(what)
        assert self.d_fine.all_written() and self.d_small.all_written(), what + ": an element of d_fine / d_small was not written"
        check(what + " d_fine", self.d_fine.values(), ref["grads"][1], BWD_TOL)
        if accumulate:
            _accumulated(what + " d_small (accumulated)", self.d_small.values(), self.old_small.double(), ref["grads"][0])
        else:
            check(what + " d_small", self.d_small.values(), ref["grads"][0], BWD_TOL)
        for n, gr in zip(ref["names"], ref["grads"][2:]):
            got = self.dw[n].values().reshape(gr.shape)
            if prefilled:      # the ABI ADDS weight and bias gradients to what the buffer holds
                _accumulated("%s d %s (added to a non-zero buffer)" % (what, n), got, self.old_w[n].double(), gr)
            else:
                check("%s d %s" % (what, n), got, gr, BWD_TOL)


def _accumulated(name, got, old, want):
    """got - old against the reference at the same rel-L2 gate, each element first given one fp32 ulp of |old| + |new| (the one addition)."""
    assert bool(torch.isfinite(got).all()), name + ": non-finite values"
    slack = 2.0 ** -23 * (old.abs() + got.abs())
    resid = ((got - old - want).abs() - slack).clamp_min(0.0)
    e = float(resid.norm() / want.norm().clamp_min(1e-30))
    print("%-84s rel-L2 beyond one ulp of the addition %.3e" % (name, e))
    gate(name, e, BWD_TOL)


def _backward_case(lib, shape, dtype, scratch, ld_act, ld3=4):
    p = Backward(shape, dtype, ld3, ld_act)
    path = "stream" if scratch and ld_act == 24 else ("tile, no scratch" if not scratch else "tile, ld_act 32")
    for accumulate, prefilled in ((False, False), (True, True)):
        what = "compose_bwd %s %s acc%d pre%d" % (path, p.name, accumulate, prefilled)
        L.check(p.launch(lib, scratch, accumulate, prefilled))
        p.check(what, accumulate, prefilled)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("shape", R.BWD_SHAPES + R.BWD_NEW_SHAPES, ids=R.shape_id)
def test_compose_backward_streaming(lib, shape, dtype):
    """The two streaming launches (scratch given, ld_act = 24): ld = 4 with sentinels, d_small overwritten over a sentinel-filled buffer and
    accumulated over a non-zero one, weight gradients into zeroed and into non-zero buffers, the scratch exactly as large as asked for."""
    _need("backward")
    _backward_case(lib, shape, dtype, scratch=True, ld_act=24)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("path", ["no_scratch", "ld_act_32"])
@pytest.mark.parametrize("shape", R.TILE_BWD_SHAPES, ids=R.shape_id)
def test_compose_backward_tile(lib, shape, path, dtype):
    """compose_bwd_kernel, the path of scratch == NULL and of ld_act != 24, in the same process."""
    _need("backward")
    _backward_case(lib, shape, dtype, scratch=path == "ld_act_32", ld_act=32 if path == "ld_act_32" else 24)


def test_compose_backward_scratch_one_byte_short_is_refused(lib):
    _need("backward")
    p = Backward((2, 16, 32), "bf16", 4, 24)
    rc = p.launch(lib, True, False, False, scratch_short=1)
    err = lib.dd_last_error().decode()
    assert rc != 0 and "scratch" in err, (rc, err)
    p.frame_checks("scratch one byte short")
    assert p.d_small.unchanged() and p.d_fine.unchanged() and all(bool((g.values() == 0).all()) for g in p.dw.values()), "something was launched"
    assert bool((p.scratch == 0xFF).all()), "the scratch was written"


# ---------------------------------------------------------------------------------------------------------------- argument checks (host code)
def _set(**kw):
    def mutate(a):
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
    return mutate


def test_compose_argument_checks_refuse_and_launch_nothing(lib):
    """Every DD_REQUIRE of the two entry points: the documented status, an error text, outputs untouched."""
    _need("argument checks")
    f = Forward((1, 4, 8), "bf16", "normal", 4, False)
    b = Backward((2, 16, 32), "bf16", 4, 24)
    fwd = [("odd H", _set(H=3)), ("odd W", _set(W=7)), ("ld_small < 3", _set(ld_small=2)), ("ld_fine < 3", _set(ld_fine=2)), ("ld_out < 3", _set(ld_out=2)),
           ("ld_act = 20", _set(ld_act=(2, 20))), ("f32 storage", _set(dtype=L.DD_F32)), ("null w_in", _set(w_in=None)), ("null b_out", _set(b_out=None)),
           ("null w_res[2]", _set(w_res=(2, None))), ("null small", _set(small=None)), ("N = 0", _set(N=0)), ("ld_netin = 4", _set(ld_netin=4)),
           ("ld_wl = 0", _set(ld_wl=0))]
    for what, m in fwd:
        rc = f.launch(lib, mutate=m)
        assert rc != 0 and lib.dd_last_error(), "dd_compose_net_fwd accepted " + what
        f.frame_checks(what)
        assert f.out.unchanged() and all(v.unchanged() for v in f.saved.values()), "dd_compose_net_fwd wrote something with " + what

    def misaligned(a):
        a.save_act[1] = a.save_act[1] + 8
    rc = f.launch(lib, mutate=misaligned)
    assert rc != 0 and lib.dd_last_error() and f.out.unchanged() and all(v.unchanged() for v in f.saved.values()), "misaligned save_act"
    bwd = [("odd H", _set(H=15)), ("odd W", _set(W=31)), ("ld_small < 3", _set(ld_small=2)), ("ld_dout < 3", _set(ld_dout=2)), ("ld_dfine < 3", _set(ld_dfine=2)),
           ("ld_dsmall < 3", _set(ld_dsmall=2)), ("ld_wl = 0", _set(ld_wl=0)), ("ld_act = 20", _set(ld_act=(3, 20))), ("f32 storage", _set(dtype=L.DD_F32)),
           ("null w_out", _set(w_out=None)), ("null dw_in", _set(dw_in=None)), ("null db_res[1]", _set(db_res=(1, None))), ("null act[4]", _set(act=(4, None))),
           ("null wl", _set(wl=None)), ("null d_fine", _set(d_fine=None))]

    def misaligned_b(a):
        a.act[0] = a.act[0] + 8
    for what, m in bwd + [("misaligned act", misaligned_b)]:
        for scratch in (True, False):
            rc = b.launch(lib, scratch, False, False, mutate=m)
            assert rc != 0 and lib.dd_last_error(), "dd_compose_net_bwd accepted " + what
            b.frame_checks(what)
            assert b.d_small.unchanged() and b.d_fine.unchanged() and all(bool((g.values() == 0).all()) for g in b.dw.values()), "dd_compose_net_bwd wrote something with " + what


def test_worst_error_over_gate_table_stream_and_tile_forward():
    """Last of the file: the worst error / gate per (stage, storage type, kernel) of this process."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    for key in sorted(WORST):
        print("compose ops, worst error / gate: %-6s %-5s %-16s %.3f" % (key + (WORST[key],)))
        gate("compose ops worst error / gate %s %s %s" % key, WORST[key], 1.0)
    assert WORST, "no forward case ran in this process"
