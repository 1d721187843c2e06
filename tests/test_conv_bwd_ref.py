"""CPU checks of tests/conv_bwd_ref.py, the float64 reference and gates of tests/test_gpu_conv_bwd_ops.py, on every input those tests use:
  * the shifted-slice sums equal autograd of the oracle's conv2d_same / conv2d_transpose_s2 to 1e-12;
  * an fp32 evaluation of the same operation, rounded where the kernels round (once per launch, per-64 launches emulated one by one), stays
    within 1x the gate for every output -- the worst ratio is printed;
  * the gate catches mutants: a tap dropped at a corner pixel or along a border, a dy channel group dropped at a tile seam, the last block of
    output channels dropped, the mask or `accumulate` ignored, `accumulate` applied twice, taps not flipped, the transposed conv's parities
    swapped, a pixel dropped from dw / db, dw laid out over coutv instead of cout.
  TWO GAPS REMAIN and are printed as such: on the transposed conv's uneven-dealing shape (9 243 pixels) the worst-case budget of dw / db
  exceeds one pixel's term, so a dropped pixel is caught there by the ACC32 rel-L2 bound only; and "db summed over coutv" changes no value at
  all, because the pad channels are zero.
No element of any output is left out of any comparison."""
import torch

import conv_bwd_ref as R
from gpu_util import ACC32
from oracle import tf_ops

F64 = torch.float64
DTYPES = ("bf16", "f16")
UNEVEN = R.uneven_cases(256)                 # the shapes the GPU tests build on a 256-CU device (MI355X)
MULTI_UNEVEN = R.uneven_multi(256)


def conv_cases():
    """(shape, per64, want_dx) of every dd_conv3x3_bwd / _multi launch of the GPU tests (the 65..96 rows on both of their paths)."""
    out = [(s, False, True) for s in R.CONV_LE64 + R.CONV_96 + [UNEVEN["le64"], UNEVEN["bwd96"]]]
    out += [(s, True, True) for s in R.CONV_96 + R.CONV_WIDE + [UNEVEN["wide"], UNEVEN["bwd96"]]]
    out += [(s, False, False) for s in R.CONV_WONLY + [UNEVEN["wonly"]]]
    out += [((ci, co) + g, False, False) for g in R.MULTI_GRIDS for ci, co in R.MULTI_CHANNELS]
    out += [((ci, co) + MULTI_UNEVEN[1], False, False) for ci, co in MULTI_UNEVEN[0]]
    return out


CONV_CASES = conv_cases()
CONVT_FWD_CASES = R.CONVT_FWD + [UNEVEN["convt_fwd"]]
CONVT_BWD_CASES = R.CONVT_BWD + [UNEVEN["convt_bwd"]]
LARGE = 2.0e8      # multiply-adds above which a shape is an uneven-dealing one, which the GPU tests run with mask + accumulate only


def _cost(shape):
    cin, cout, B, H, W = shape
    return 9.0 * cin * cout * B * H * W


def _flags(shape, want_dx):
    if not want_dx:
        return [(0, 0)]
    return R.FLAGS if _cost(shape) < LARGE else [(1, 1)]


def _close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-12 * scale, "%s: %.3e" % (what, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- tie to the oracle
def test_reference_equals_autograd_of_the_oracle():
    seen = set()
    for shape, _, _ in CONV_CASES:
        if shape in seen:
            continue
        seen.add(shape)
        x, dy, k, old = R.conv_inputs(shape, "bf16")
        ref = R.conv3_bwd(x, dy, k, True, old, per64=True)
        z, kk, b = x.clone().requires_grad_(), k.clone().requires_grad_(), torch.zeros(shape[1], dtype=F64, requires_grad=True)
        (tf_ops.conv2d_same(z, kk, b) * dy).sum().backward()
        _close(sum(ref["dx_parts"]), z.grad, "conv dx %s" % (shape,))
        _close(ref["dx"], old + z.grad * (x > 0), "conv masked accumulated dx %s" % (shape,))
        _close(ref["dw"], kk.grad, "conv dw %s" % (shape,))
        _close(ref["db"], b.grad, "conv db %s" % (shape,))
        # the mask is the ReLU the producer applied: the gradient of conv(relu(z)) at z = x, where x > 0 is exact
        z2 = x.clone().requires_grad_()
        (tf_ops.conv2d_same(torch.relu(z2), k) * dy).sum().backward()
        _close(R.conv3_bwd(x, dy, k, True)["dx"], z2.grad, "conv masked dx %s" % (shape,))
    for shape in dict.fromkeys(CONVT_FWD_CASES + CONVT_BWD_CASES):
        x, dy, k, bias, old = R.convt_inputs(shape, "f16")
        z, kk, b = x.clone().requires_grad_(), k.clone().requires_grad_(), bias.clone().requires_grad_()
        y = tf_ops.conv2d_transpose_s2(z, kk, b)
        (y * dy).sum().backward()
        _close(R.convt_fwd(x, k, bias, False)[0], y.detach(), "convT y %s" % (shape,))
        _close(R.convt_fwd(x, k, bias, True)[0], torch.relu(y.detach()), "convT relu y %s" % (shape,))
        ref = R.convt_bwd(x, dy, k, True, old)
        _close(sum(ref["dx_parts"]), z.grad, "convT dx %s" % (shape,))
        _close(ref["dx"], old + z.grad * (x > 0), "convT masked accumulated dx %s" % (shape,))
        _close(ref["dw"], kk.grad, "convT dw %s" % (shape,))
        _close(ref["db"], b.grad, "convT db %s" % (shape,))


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation
def _launches(parts, per64):
    return parts if per64 else [sum(parts)]


def test_fp32_evaluation_stays_within_the_gate():
    worst = {}

    def note(key, got, ref, gate_t, what):
        w = R.worst_ratio(got, ref, gate_t)
        worst[key] = max(worst.get(key, 0.0), w)
        assert w <= 1.0, "%s: fp32 emulation at %.3f of the gate" % (what, w)

    for dtype in DTYPES:
        for shape, per64, want_dx in CONV_CASES:
            x, dy, k, old = R.conv_inputs(shape, dtype)
            x32, dy32, k32 = x.float(), dy.float(), k.float()
            if want_dx:
                parts32 = [R.conv3_dx_part(dy32, k32, c0, c1)[0] for c0, c1 in R.co_blocks(shape[1])]
                for mask, acc in _flags(shape, True):
                    ref = R.conv_reference(shape, dtype, mask, acc, per64)
                    got = R.emulate_dx(_launches(parts32, per64), x, mask, old if acc else None, dtype)
                    note("conv dx" + (" per-64" if per64 else ""), got, ref["dx"], R.gate_storage(ref["dx"], ref["dx_budget"], dtype, ref["dx_points"]),
                         "conv dx %s %s mask%d acc%d per64=%d" % (shape, dtype, mask, acc, per64))
            ref = R.conv_reference(shape, dtype, 0, 0, per64)
            dw32, _, db32, _ = R.conv3_dw(x32, dy32)
            note("conv dw", dw32.double(), ref["dw"], R.gate_f32(ref["dw_budget"]), "conv dw %s %s" % (shape, dtype))
            note("conv db", db32.double(), ref["db"], R.gate_f32(ref["db_budget"]), "conv db %s %s" % (shape, dtype))
        for shape in CONVT_FWD_CASES:
            x, _, k, bias, _ = R.convt_inputs(shape, dtype)
            for relu in (0, 1):
                ref, budget = R.convt_fwd_reference(shape, dtype, relu)
                got = R.to_storage(R.convt_fwd(x.float(), k.float(), bias.float(), bool(relu))[0], dtype)
                note("convT y", got, ref, R.gate_storage(ref, budget, dtype), "convT y %s %s relu%d" % (shape, dtype, relu))
        for shape in CONVT_BWD_CASES:
            x, dy, k, _, old = R.convt_inputs(shape, dtype)
            e32 = R.convt_bwd(x.float(), dy.float(), k.float())
            for mask, acc in R.FLAGS:
                ref = R.convt_bwd_reference(shape, dtype, mask, acc)
                got = R.emulate_dx(e32["dx_parts"], x, mask, old if acc else None, dtype)
                note("convT dx", got, ref["dx"], R.gate_storage(ref["dx"], ref["dx_budget"], dtype, ref["dx_points"]),
                     "convT dx %s %s mask%d acc%d" % (shape, dtype, mask, acc))
            note("convT dw", e32["dw"].double(), ref["dw"], R.gate_f32(ref["dw_budget"]), "convT dw %s %s" % (shape, dtype))
            note("convT db", e32["db"].double(), ref["db"], R.gate_f32(ref["db_budget"]), "convT db %s %s" % (shape, dtype))
    for key in sorted(worst):
        print("fp32 emulation, worst error / gate: %-16s %.3f" % (key, worst[key]))
    assert worst and max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- mutants
class Tally:
    def __init__(self):
        self.applied = {}
        self.gaps = {}        # mutant -> cases in which NO element flags it (only the whole-tensor rel-L2 bound does)
        self.in_band = 0      # elements moved by more than twice the gate whose STORED value passes it (the mutant's own rounding, see judge)

    def judge(self, mutant, case, mut, ref, gate_t, rounder, rel=None):
        """`mut`: the mutant applied to the reference output (float64).  Where it differs from the reference by more than twice the gate it must be
        flagged, and what the mutant would STORE (its own roundings on top) must be flagged somewhere.  Returns False where the mutant changes nothing (it does not apply to the case).
        rel (the uneven-dealing shapes only, whose reductions run over thousands of pixels: there the worst-case budget n u S of dw / db exceeds
        one pixel's term): the rel-L2 bound the GPU tests keep next to the elementwise gate; a mutant no element flags must break that one."""
        change = (mut - ref).abs()
        if not bool((change > 0).any()):
            return False
        flagged = R.ratio(rounder(mut), ref, gate_t) > 1.0      # as the mutant would store it
        big = change > 2 * gate_t
        # The stored value is off by the mutant's OWN store rounding as well, half an ulp at |mut|.  Where |mut| sits in the binade above |ref| that
        # is twice the half-ulp the gate holds, and a change just over two gates can be stored inside the gate: the reference 1.9963 (bf16
        # neighbours 1.9922 and 2.0, gate 0.0041) and a mutant at 2.0056 (2.3 gates away; neighbours 2.0 and 2.0156) both store 2.0 -- the
        # very bits of a right answer, which no check can flag.  So the stored value must be flagged wherever the change exceeds twice the gate
        # plus that excess (then |stored - ref| >= change - hu(mut) > 2 gate - hu(ref) >= gate); the elements in between are counted.
        dt = getattr(rounder, "dtype", None)
        excess = (R.half_ulp(mut, dt) - R.half_ulp(ref, dt)).clamp_min(0) if dt else torch.zeros_like(change)
        self.in_band += int((big & ~(change > 2 * gate_t + excess) & ~flagged).sum())
        assert bool(flagged[change > 2 * gate_t + excess].all()), "%s on %s: %d elements changed by more than twice their gate pass it" % (
            mutant, case, int(((change > 2 * gate_t + excess) & ~flagged).sum()))
        if rel is not None and not bool(flagged.any()):
            e = float((rounder(mut) - ref).norm() / ref.norm().clamp_min(1e-30))
            assert e > rel, "%s on %s: neither an element nor the rel-L2 bound (%.3e <= %.1e) flags it" % (mutant, case, e, rel)
            self.gaps[mutant] = self.gaps.get(mutant, 0) + 1      # a gap of the elementwise gate, recorded as one
            return True
        assert bool(flagged.any()), "%s on %s: not flagged (largest change %.3f of its gate)" % (mutant, case, float((change / gate_t.clamp_min(1e-300)).max()))
        n, f = self.applied.get(mutant, (0, 1.0))
        self.applied[mutant] = (n + 1, min(f, float(flagged.sum()) / float((change > 0).sum())))
        return True


def _f32(t):
    return t.float().double()


def _one_pixel(t, b, y, x, c0=None, c1=None):
    o = torch.zeros_like(t)
    o[b, y, x, c0:c1] = t[b, y, x, c0:c1]
    return o


def test_the_gates_flag_every_mutant():
    tally = Tally()
    for dtype in DTYPES:
        store = lambda t, dtype=dtype: R.to_storage(t, dtype)      # noqa: E731
        store.dtype = dtype
        for shape, per64, want_dx in CONV_CASES:
            cin, cout, B, H, W = shape
            x, dy, k, old = R.conv_inputs(shape, dtype)
            blocks = R.co_blocks(cout)
            base = R.conv_reference(shape, dtype, 0, 0, per64)
            case0 = "conv %s %s per64=%d" % (shape, dtype, per64)
            # ---- dw / db
            gw, gb = R.gate_f32(base["dw_budget"]), R.gate_f32(base["db_budget"])
            rel32 = ACC32[dtype] if _cost(shape) >= LARGE else None
            for (pb, py, px), tag in (((B - 1, H - 1, W - 1), "corner"), ((0, H // 2, min(W - 1, 16)), "seam")):
                d1 = _one_pixel(dy, pb, py, px)
                ddw, _, ddb, _ = R.conv3_dw(x, d1)
                assert tally.judge("dw: one pixel dropped (%s)" % tag, case0, base["dw"] - ddw, base["dw"], gw, _f32, rel32)
                assert tally.judge("db: one pixel dropped (%s)" % tag, case0, base["db"] - ddb, base["db"], gb, _f32, rel32)
            if W > 16 and cout >= 16:
                d1 = _one_pixel(dy, 0, H // 2, 16, 8, 16)
                ddw, _, ddb, _ = R.conv3_dw(x, d1)
                assert tally.judge("dw: 8-channel group of dy dropped at the seam pixel", case0, base["dw"] - ddw, base["dw"], gw, _f32, rel32)
                assert tally.judge("db: 8-channel group of dy dropped at the seam pixel", case0, base["db"] - ddb, base["db"], gb, _f32, rel32)
            if cout % 8:      # dw written with rows of coutv instead of cout words (what lands past the array is lost)
                coutv = R.round_up(cout, 8)
                flat = torch.zeros(9 * cin * coutv, dtype=F64)
                flat.view(9 * cin, coutv)[:, :cout] = base["dw"].reshape(9 * cin, cout)
                assert tally.judge("dw laid out over coutv instead of cout", case0, flat[:9 * cin * cout].view(3, 3, cin, cout), base["dw"], gw, _f32)
                dbv = torch.cat([base["db"], torch.zeros(coutv - cout, dtype=F64)])      # db over coutv channels: the extra sums are those of the zero pad channels
                assert not tally.judge("db summed over coutv instead of cout", case0, dbv[:cout], base["db"], gb, _f32) and not bool(dbv[cout:].any())
            if not want_dx:
                continue
            # ---- dx
            parts = base["dx_parts"]
            for mask, acc in _flags(shape, True):
                ref = R.conv_reference(shape, dtype, mask, acc, per64)
                gd = R.gate_storage(ref["dx"], ref["dx_budget"], dtype, ref["dx_points"])
                m = (x > 0).to(F64) if mask else None
                o = old if acc else None
                case = case0 + " mask%d acc%d" % (mask, acc)

                def finish(ps, m=m, o=o):
                    return R.dx_points(_launches(ps, per64), m, o)[-1]

                def minus(delta_fn):      # the parts with a linear piece taken out of each block
                    return [p - delta_fn(c0, c1) for p, (c0, c1) in zip(parts, blocks)]

                assert not tally.judge("nothing", case, finish(parts), ref["dx"], gd, store)
                # centre tap dropped at the far corner pixel (every block), and at the near corner for the first 8 output channels only
                far = _one_pixel(dy, B - 1, H - 1, W - 1)
                assert tally.judge("dx: centre tap dropped at a corner pixel", case,
                                   finish(minus(lambda c0, c1: R.conv3_dx_part(far, k, c0, c1, taps=[4], magnitudes=False)[0])), ref["dx"], gd, store)
                near = _one_pixel(dy, 0, 0, 0, 0, 8)
                assert tally.judge("dx: centre tap of 8 output channels dropped at a corner pixel", case,
                                   finish(minus(lambda c0, c1: R.conv3_dx_part(near, k, c0, c1, taps=[4], magnitudes=False)[0])), ref["dx"], gd, store)
                # one tap dropped along a whole border row / column: the tap that reads the row below (the column to the right)
                if H > 1:
                    def row0(c0, c1):
                        d = R.conv3_dx_part(dy, k, c0, c1, taps=[1], magnitudes=False)[0]
                        d[:, 1:] = 0
                        return d
                    assert tally.judge("dx: one tap dropped along a border row", case, finish(minus(row0)), ref["dx"], gd, store)
                if W > 1:
                    def col_last(c0, c1):
                        d = R.conv3_dx_part(dy, k, c0, c1, taps=[5], magnitudes=False)[0]
                        d[:, :, :-1] = 0
                        return d
                    assert tally.judge("dx: one tap dropped along a border column", case, finish(minus(col_last)), ref["dx"], gd, store)
                if W > 16 and cout >= 16:
                    seam = _one_pixel(dy, 0, H // 2, 16, 8, 16)
                    assert tally.judge("dx: 8-channel group of dy dropped at the seam pixel", case,
                                       finish(minus(lambda c0, c1: R.conv3_dx_part(seam, k, c0, c1, magnitudes=False)[0])), ref["dx"], gd, store)
                if per64 and len(parts) > 1:
                    assert tally.judge("dx: last output-channel block dropped (co_base)", case, R.dx_points(parts[:-1], m, o)[-1], ref["dx"], gd, store)
                if mask:
                    assert tally.judge("dx: mask ignored", case, R.dx_points(_launches(parts, per64), None, o)[-1], ref["dx"], gd, store)
                if acc:
                    assert tally.judge("dx: accumulate ignored", case, R.dx_points(_launches(parts, per64), m, None)[-1], ref["dx"], gd, store)
                    assert tally.judge("dx: accumulate applied twice", case, R.dx_points(_launches(parts, per64), m, 2 * old)[-1], ref["dx"], gd, store)
                if H > 1 or W > 1:
                    unflipped = [R.conv3_dx_part(dy, k, c0, c1, flip=True, magnitudes=False)[0] for c0, c1 in blocks]
                    assert tally.judge("dx: taps not flipped in wd", case, finish(unflipped), ref["dx"], gd, store)

        for shape in CONVT_FWD_CASES:
            x, _, k, bias, _ = R.convt_inputs(shape, dtype)
            for relu in (0, 1) if shape in R.CONVT_FWD else (1,):
                ref, budget = R.convt_fwd_reference(shape, dtype, relu)
                gy = R.gate_storage(ref, budget, dtype)
                case = "convT fwd %s %s relu%d" % (shape, dtype, relu)
                assert tally.judge("convT y: a / b parity swapped", case, R.convt_fwd(x, k, bias, bool(relu), swap_ab=True)[0], ref, gy, store)
                nobias = R.convt_fwd(x, k, None, bool(relu))[0]
                assert tally.judge("convT y: bias dropped", case, nobias, ref, gy, store)
        for shape in CONVT_BWD_CASES:
            cin, cout, B, H, W = shape
            rel32 = None if shape in R.CONVT_BWD else ACC32[dtype]
            x, dy, k, _, old = R.convt_inputs(shape, dtype)
            blocks = R.co_blocks(cout)
            base = R.convt_bwd_reference(shape, dtype, 0, 0)
            case0 = "convT bwd %s %s" % (shape, dtype)
            gw, gb = R.gate_f32(base["dw_budget"]), R.gate_f32(base["db_budget"])
            d1 = _one_pixel(dy, B - 1, 2 * H - 1, 2 * W - 1)
            e1 = R.convt_bwd(x, d1, k)
            assert tally.judge("convT dw: one pixel dropped", case0, base["dw"] - e1["dw"], base["dw"], gw, _f32, rel32)
            assert tally.judge("convT db: one pixel dropped", case0, base["db"] - e1["db"], base["db"], gb, _f32, rel32)
            sw = R.convt_bwd(x, _swap_parity(dy), k)
            assert tally.judge("convT dw: a / b parity swapped", case0, sw["dw"], base["dw"], gw, _f32)
            parts = base["dx_parts"]
            for mask, acc in R.FLAGS if shape in R.CONVT_BWD else [(1, 1)]:
                ref = R.convt_bwd_reference(shape, dtype, mask, acc)
                gd = R.gate_storage(ref["dx"], ref["dx_budget"], dtype, ref["dx_points"])
                m = (x > 0).to(F64) if mask else None
                o = old if acc else None
                case = case0 + " mask%d acc%d" % (mask, acc)
                assert not tally.judge("nothing", case, R.dx_points(parts, m, o)[-1], ref["dx"], gd, store)
                corner = [p - R.convt_dx_part(_one_pixel(dy, B - 1, 2 * H - 1, 2 * W - 1), k, c0, c1)[0] for p, (c0, c1) in zip(parts, blocks)]
                assert tally.judge("convT dx: one tap dropped at a corner pixel", case, R.dx_points(corner, m, o)[-1], ref["dx"], gd, store)
                row = torch.zeros_like(dy)
                row[:, 0] = dy[:, 0]      # the taps a = 0 of the first input row
                border = [p - R.convt_dx_part(row, k, c0, c1)[0] for p, (c0, c1) in zip(parts, blocks)]
                assert tally.judge("convT dx: taps dropped along a border row", case, R.dx_points(border, m, o)[-1], ref["dx"], gd, store)
                if 2 * W > 16:
                    seam = [p - R.convt_dx_part(_one_pixel(dy, 0, H, 16, 8, 16), k, c0, c1)[0] for p, (c0, c1) in zip(parts, blocks)]
                    assert tally.judge("convT dx: 8-channel group of dy dropped at the seam pixel", case, R.dx_points(seam, m, o)[-1], ref["dx"], gd, store)
                if len(parts) > 1:
                    assert tally.judge("convT dx: last output-channel block dropped (co_off)", case, R.dx_points(parts[:-1], m, o)[-1], ref["dx"], gd, store)
                if mask:
                    assert tally.judge("convT dx: mask ignored", case, R.dx_points(parts, None, o)[-1], ref["dx"], gd, store)
                if acc:
                    assert tally.judge("convT dx: accumulate ignored", case, R.dx_points(parts, m, None)[-1], ref["dx"], gd, store)
                    assert tally.judge("convT dx: accumulate applied twice", case, R.dx_points(parts, m, 2 * old)[-1], ref["dx"], gd, store)
                swapped = [R.convt_dx_part(dy, k, c0, c1, swap_ab=True)[0] for c0, c1 in blocks]
                assert tally.judge("convT dx: a / b parity swapped", case, R.dx_points(swapped, m, o)[-1], ref["dx"], gd, store)
    print("elements moved by more than twice their gate that the mutant's own store rounding brought back inside it: %d" % tally.in_band)
    for mutant in sorted(tally.gaps):
        print("GAP  %-61s NOT flagged by the elementwise gate in %d cases (convT uneven-dealing shape, 9 243 pixels: the budget n u S exceeds one "
              "pixel's term); only the ACC32 rel-L2 bound catches it there" % (mutant, tally.gaps[mutant]))
    print("GAP  %-61s changes no value (the extra sums are those of the zero pad channels, and adding 0 leaves a guard word as it is): "
          "neither a gate nor a guard flags it" % "db summed over coutv instead of cout")
    assert set(tally.gaps) <= {"convT dw: one pixel dropped", "convT db: one pixel dropped"}, tally.gaps
    for mutant in sorted(tally.applied):
        n, share = tally.applied[mutant]
        print("%-66s flagged in all %3d cases it applies to; least share of changed elements flagged %.2f" % (mutant, n, share))
    expected = {"dx: centre tap dropped at a corner pixel", "dx: centre tap of 8 output channels dropped at a corner pixel", "dx: one tap dropped along a border row",
                "dx: one tap dropped along a border column", "dx: 8-channel group of dy dropped at the seam pixel", "dx: last output-channel block dropped (co_base)",
                "dx: mask ignored", "dx: accumulate ignored", "dx: accumulate applied twice", "dx: taps not flipped in wd", "dw laid out over coutv instead of cout",
                "dw: one pixel dropped (corner)", "db: one pixel dropped (corner)", "convT y: a / b parity swapped", "convT dx: a / b parity swapped",
                "convT dx: last output-channel block dropped (co_off)", "convT dw: one pixel dropped", "convT db: one pixel dropped"}
    assert expected <= set(tally.applied), expected - set(tally.applied)


def _swap_parity(dy):
    """dy with its (a, b) parity planes exchanged: pixel (2i + a, 2j + b) takes the value of (2i + b, 2j + a)."""
    out = dy.clone()
    out[:, 0::2, 1::2] = dy[:, 1::2, 0::2]
    out[:, 1::2, 0::2] = dy[:, 0::2, 1::2]
    return out


# ---------------------------------------------------------------------------------------------------------------- packing restatement
def test_pack_restatement_layout():
    """The numpy restatement against a literal triple loop: tap_flip, strides, zero padding, dst_ld / dst_tap_stride / offset."""
    import numpy as np
    rng = np.random.default_rng(0)
    for kind, role, cin, cout in (("conv", "dgrad", 5, 3), ("conv", "fwd", 5, 3), ("convT2", "fwd", 3, 16), ("convT2", "dgrad", 3, 16)):
        taps, n, k, st, sn, sk, flip = R.pack_params(kind, role, cin, cout)
        n_pad, k_pad = R.pack_dims(n, k)
        src = rng.standard_normal((9 if kind == "conv" else 4) * cin * cout).astype(np.float32)
        for ld, ts, off in ((0, 0, 0), (k_pad + 32, n_pad * (k_pad + 32) + 64, 32)):
            got = R.pack_weights(src, "bf16", taps, n, k, n_pad, k_pad, st, sn, sk, flip, dst_off=off, dst_ld=ld, dst_tap_stride=ts)
            want = torch.zeros_like(got)
            for t in range(taps):
                for nn in range(n):
                    for kk in range(k):
                        v = src[(taps - 1 - t if flip else t) * st + nn * sn + kk * sk]
                        want[off + t * (ts or n_pad * k_pad) + nn * (ld or k_pad) + kk] = torch.tensor(v).to(torch.bfloat16)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (kind, role, ld)
    # the dgrad image of a conv IS the header's wd: wd[t][ci][co] = K[8 - t][ci][co]
    k = torch.randn(3, 3, 5, 3).to(torch.bfloat16).float()
    taps, n, kk_, st, sn, sk, flip = R.pack_params("conv", "dgrad", 5, 3)
    img = R.pack_weights(k.numpy().reshape(-1), "bf16", taps, n, kk_, 16, 32, st, sn, sk, flip).view(9, 16, 32)
    assert torch.equal(img[:, :5, :3].float(), k.reshape(9, 5, 3).flip(0)) and not bool(img[:, 5:].any()) and not bool(img[:, :, 3:].any())
