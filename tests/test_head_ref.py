"""CPU checks of tests/head_ref.py, the float64 reference, gates, inputs and mutants of tests/test_gpu_head_ops.py, on every input those tests use:
  * with every rounding switched off the reference equals torch float64 autograd of the plain formula (oracle.tf_ops.kernel_prediction behind two
    matmuls and a ReLU) for all six outputs, to 1e-12;
  * an fp32 evaluation with the kernel's rounding points (channels in 32-wide chunks, pixels in 32-pixel steps, both in a scrambled order) stays
    strictly inside every gate; no hidden unit of any committed input is undecided; the median logit spread lies in [2, 8]; GEMM 1 of the grid
    kinds is bit-identical under two summation orders;
  * every mutant of head_ref.MUTANTS exceeds a gate, on at least one case of the table, by the factor asserted in FACTORS below (recorded from
    this test's own printout; "inf": an element whose gate is 0 -- it must be bit-exact -- changed):
        index mutants (>= 10 required)
          inf: taps_transposed, pad_reflect_not_symmetric, pad_clamp, slot_perm_identity, softmax_over_32, x_mask_dropped, x_mask_ge0,
          dlogits_missing_dot, dx_overwrites_when_accumulating, dba_unmasked, image_base_of_first_image (1e3 .. 2e7 where the gate is not 0);
          softmax_no_max_shift inf (NaN, on the "big" row only: elsewhere it is an fp32 softmax and passes, as expected);
          dW_overwrite_not_add 2.8e6, last_segment_dropped 1.7e6
        rounding mutants (> 1 required)
          inf: hid_not_rounded, logits_not_rounded, weights_truncated (1e4 .. 6e4 where the gate is not 0), dx_single_rounding_when_accumulating
          (only elements whose gate is 0 show it); dbb_from_unrounded_dl 2.3e3
        not distinguishable at this budget: none.
        change no value on any admissible input (head_ref.EQUIVALENT_MUTANTS, asserted): dWa_rows_beyond_C_written, relu_mask_on_pre_not_hidT;
  * flip-based gates are monotone in the budget and zero only where the stored value must be exact.
No element of any output is left out of any comparison."""
import math

import pytest
import torch

import head_ref as R
from oracle import tf_ops

F64 = torch.float64
OUTPUTS = R.OUTPUTS_FWD + R.OUTPUTS_BWD
ALL = [(case, dtype, kind) for case in R.CASES for dtype in R.DTYPES for kind in R.kinds_of(case)]
# the least factor by which each mutant must exceed a gate somewhere in the table (measured: see the docstring)
FACTORS = {"taps_transposed": math.inf, "pad_reflect_not_symmetric": math.inf, "pad_clamp": math.inf, "slot_perm_identity": math.inf,
           "softmax_no_max_shift": math.inf, "softmax_over_32": math.inf, "x_mask_dropped": math.inf, "x_mask_ge0": math.inf,
           "dlogits_missing_dot": math.inf, "dx_overwrites_when_accumulating": math.inf, "dba_unmasked": math.inf, "dW_overwrite_not_add": 1e6,
           "last_segment_dropped": 1e6, "image_base_of_first_image": math.inf,
           "hid_not_rounded": math.inf, "logits_not_rounded": math.inf, "weights_truncated": math.inf,
           "dx_single_rounding_when_accumulating": math.inf, "dbb_from_unrounded_dl": 1e3}


def _close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-12 * scale, "%s: %.3e" % (what, float((a - b).abs().max()))


def test_reference_without_roundings_equals_autograd_of_the_plain_formula():
    for case in R.CASES:
        ks = case[0]
        kind = R.kinds_of(case)[-1] if case[5] == "big" else "real"
        inp = R.head_inputs(case, "bf16", kind)
        ref = R.evaluate(inp, ks, "bf16", accumulate=True, prefilled=True, rounding=False, budget=False)
        leaves = {k: inp[k].clone().requires_grad_() for k in ("x", "wa", "ba", "wb", "bb")}
        hid = torch.relu(leaves["x"] @ leaves["wa"] + leaves["ba"])
        out = tf_ops.kernel_prediction(inp["src"], hid @ leaves["wb"] + leaves["bb"], ks)
        (out * inp["dout"]).sum().backward()
        what = R.case_id(case)
        _close(ref["out"], out.detach(), what + " out")
        # x is the backbone's ReLU output: its gradient passes where x is positive (as a 16-bit integer: -0 and negative values drop it)
        _close(ref["dx"], inp["dx_old"] + leaves["x"].grad * R.positive16(inp["x"]), what + " dx")
        for name, leaf in (("dwa", "wa"), ("dba", "ba"), ("dwb", "wb"), ("dbb", "bb")):
            _close(ref[name], inp["w_old_" + name] + leaves[leaf].grad, what + " " + name)
        plain = R.evaluate(inp, ks, "bf16", rounding=False, budget=False)
        _close(plain["dx"], leaves["x"].grad * R.positive16(inp["x"]), what + " dx (no accumulate)")
        _close(plain["dwa"], leaves["wa"].grad, what + " dwa (zeroed buffer)")


def test_symmetric_pad_index_is_the_kernels():
    for n in (1, 2, 3, 7):
        for P in (1, 2):
            if n < P:
                continue
            i = torch.arange(-P, n + P)
            want = torch.tensor([(-v - 1) if v < 0 else (2 * n - 1 - v if v >= n else v) for v in i.tolist()])
            assert torch.equal(R._index(i, n, "symmetric"), want) and int(want.min()) >= 0 and int(want.max()) < n


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_fp32_emulation_inputs_and_scales(dtype):
    worst, worst_flips = {}, 0.0
    for case, dt, kind in ALL:
        if dt != dtype:
            continue
        ks = case[0]
        inp = R.head_inputs(case, dtype, kind)
        what = "%s %s %s" % (R.case_id(case), dtype, kind)
        for acc, pre in ((False, False), (True, True)):
            ref = R.head_reference(case, dtype, kind, acc, pre)
            emu = R.evaluate(inp, ks, dtype, accumulate=acc, prefilled=pre, emulate=True, budget=False, seed=11)
            for name in OUTPUTS:
                w = R.worst_ratio(emu[name].double(), ref[name], ref["gate_" + name])
                worst[(kind, name)] = max(worst.get((kind, name), 0.0), w)
                assert w < 1.0, "%s %s: the fp32 emulation is at %.4f of its gate" % (what, name, w)
        assert ref["undecided"] == 0, "%s: %d hidden units whose ReLU is undecided within 2 n u S" % (what, ref["undecided"])
        assert 2.0 <= ref["spread"] <= 8.0, "%s: median logit spread %.2f" % (what, ref["spread"])
        worst_flips = max(worst_flips, ref["flips"]["logT"] / ref["logT"].numel())
        if kind != "real":      # GEMM 1 exact in fp32: two scrambled chunk orders give the same bits, and they are the float64 value
            x, wa, ba = inp["x"].float(), R.to_storage(inp["wa"], dtype).float(), inp["ba"].float()
            a, b = R.Sums(True, 1).gemm(x, wa, ba), R.Sums(True, 2).gemm(x, wa, ba)
            rev = ba + sum((x[..., c:c + 8] @ wa[c:c + 8] for c in reversed(range(0, case[1], 8))), torch.zeros_like(a))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), rev.view(torch.int32)), what
            assert torch.equal(a.double(), ref["pre"]) and not bool((ref["pre"] == 0).any()), what
        if kind == "grid-exact":      # ... and the logits are exactly representable: nothing can flip before the softmax
            assert ref["flips"]["logT"] == 0 and torch.equal(R.to_storage(ref["logT"], dtype), ref["logT"]), what
            lg = inp["bb"] + ref["hidT"] @ R.to_storage(inp["wb"], dtype)
            assert torch.equal(lg, ref["logT"]), what
    for key in sorted(worst):
        print("fp32 emulation, worst error / gate: %-10s %-4s %.3f" % (key + (worst[key],)))
    print("largest share of logits that may flip: %.3f" % worst_flips)


def test_real_kind_weights_are_not_representable_and_x_is():
    for case, dtype, kind in ALL:
        inp = R.head_inputs(case, dtype, kind)
        assert torch.equal(R.representable(inp["x"], dtype), inp["x"])
        if kind == "real":
            for k in ("wa", "wb", "ba", "bb"):
                assert float((R.representable(inp[k], dtype) != inp[k]).double().mean()) > 0.5, (case, dtype, k)
        if case[5] == "neg":
            v = inp["x"][..., [1, 5]]
            assert bool(((v == 0) & torch.signbit(v)).any()) and bool((v < 0).any()) and bool((v > 0).any())


def _finite_ratio(got, ref, gate):
    r = R.ratio(got, ref, gate)
    r = r[gate > 0]
    r = r[torch.isfinite(r)]
    return float(r.max()) if r.numel() else 0.0


def _mutant_factor(mutant):
    """(worst error / gate over every case, kind, type and output -- NaN counts as inf; the same over the elements whose gate is not 0; whether
    any value changed at all)."""
    worst, finite, changed = 0.0, 0.0, False
    for case, dtype, kind in ALL:
        ref = R.head_reference(case, dtype, kind, True, True)
        got = R.evaluate(R.head_inputs(case, dtype, kind), case[0], dtype, accumulate=True, prefilled=True, mut={mutant}, budget=False)
        for name in OUTPUTS:
            if not bool(torch.isfinite(got[name]).all()):
                worst, changed = math.inf, True
                continue
            changed = changed or not torch.equal(got[name], ref[name])
            worst = max(worst, R.worst_ratio(got[name], ref[name], ref["gate_" + name]))
            finite = max(finite, _finite_ratio(got[name], ref[name], ref["gate_" + name]))
    return worst, finite, changed


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_the_gates_flag_every_mutant(mutant):
    kind, what = R.MUTANTS[mutant]
    worst, finite, changed = _mutant_factor(mutant)
    print("%-40s %-8s worst error / gate %10.3g   (where the gate is not 0: %10.3g)   %s" % (mutant, kind, worst, finite, what))
    if mutant in R.EQUIVALENT_MUTANTS:
        assert not changed, "%s changes a value after all: give it a factor" % mutant
        return
    assert set(FACTORS) | set(R.EQUIVALENT_MUTANTS) == set(R.MUTANTS)
    assert worst >= FACTORS[mutant], "%s: exceeds a gate by %.3g only, recorded %.3g" % (mutant, worst, FACTORS[mutant])
    assert worst >= 10.0 if kind == "index" else worst > 1.0, "%s (%s): %.3g" % (mutant, kind, worst)


def test_flip_gates_are_monotone_and_zero_only_where_the_value_must_be_exact():
    gen = torch.Generator().manual_seed(3)
    for dtype in R.DTYPES:
        v = torch.randn(20000, generator=gen, dtype=F64) * torch.pow(2.0, torch.randint(-12, 6, (20000,), generator=gen).double())
        prev = torch.zeros_like(v)
        for k in range(-30, -4, 2):
            cur = R.flip(v, v.abs() * 2.0 ** k, dtype)
            assert bool((cur >= prev).all()), (dtype, k)
            prev = cur
        assert bool((R.flip(v, torch.zeros_like(v), dtype) == 0).all())
        tie = R.to_storage(v, dtype) + R.half_ulp(R.to_storage(v, dtype), dtype)      # exactly between two neighbours: any budget lets it flip
        assert float((R.flip(tie, tie.abs() * 2.0 ** -20, dtype) > 0).double().mean()) > 0.99      # (all but values the type flushes to 0)
        h = R.half_ulp(v, dtype)
        assert bool((R.half_ulp(2 * v, dtype) >= h).all()) and bool((h > 0).all())
    for case, dtype, kind in ALL:
        ref = R.head_reference(case, dtype, kind, False, False)
        masked = ~R.positive16(R.head_inputs(case, dtype, kind)["x"])
        assert bool((ref["gate_dx"][masked] == 0).all()) and bool((ref["dx"][masked] == 0).all()) and not bool(torch.signbit(ref["dx"][masked]).any())
        assert bool((ref["gate_out"] > 0).all()) and all(bool((ref["gate_" + n] >= 0).all()) for n in OUTPUTS)
        acc = R.head_reference(case, dtype, kind, True, True)
        old = R.head_inputs(case, dtype, kind)["dx_old"]
        assert bool((acc["gate_dx"][masked] == 0).all()) and torch.equal(acc["dx"][masked], old[masked])      # old + 0, stored as it was
