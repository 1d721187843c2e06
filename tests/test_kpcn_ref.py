"""CPU checks of tests/kpcn_ref.py, the float64 reference, gates, inputs and mutants of tests/test_gpu_kpcn_ops.py, on the inputs those tests use:
  * with every rounding switched off the reference equals torch float64 autograd of oracle.tf_ops.kernel_prediction (HID: behind the matmul) for
    the output and the d logits of every case, to 1e-12;
  * head_ref._index is sym_index of csrc/dd_pointwise.hip for every n >= P, P in 1..3, and stays inside the image; the generator refuses n < P;
  * an fp32 evaluation in each of the four summation orders stays strictly inside every gate, for every case, storage type and kind (the worst
    error / gate is printed);
  * every mutant of kpcn_ref.MUTANTS exceeds a gate on at least one case (the factor is printed; "inf": an element whose gate is 0 -- it must be
    bit-exact -- changed, or a NaN); kpcn_ref.EQUIVALENT_MUTANTS (at most two) change no value at all;
  * the input generators keep their promises: representability, logit - max >= -18, the overflow of the 96 offset, the spread, flat p = 1 / K;
  * the dispatch rule sends every case down the route it is named after.
No element of any output is left out of any comparison."""
import math

import pytest
import torch

import kpcn_ref as R
from oracle import tf_ops

OUTPUTS = ("out", "dl_row")
KS = (3, 5, 7)


def _all(ks=None, dtype=None):
    return [(c, dt, kind) for c in R.ALL_CASES for dt in R.DTYPES for kind in R.KINDS if ks in (None, c.ks) and dtype in (None, dt)]


def _close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= 1e-12 * scale, "%s: %.3e" % (what, float((a - b).abs().max()))


def _logits_plain(case, dtype, inp):
    lay = R.layout(case, dtype)
    if not lay.hid:
        return inp["lg"][..., lay.off:lay.off + lay.K]
    col = R.WB_C0 + lay.off
    return inp["hid"][..., :lay.kh] @ inp["wb"][:lay.kh, col:col + lay.K] + inp["bb"][col:col + lay.K]


@pytest.mark.parametrize("ks", KS)
def test_reference_without_roundings_equals_autograd_of_the_plain_formula(ks):
    for case, dtype, kind in _all(ks, "bf16"):
        inp = R.kpcn_inputs(case, dtype, kind)
        lay = R.layout(case, dtype)
        ref = R.evaluate(inp, case, dtype, rounding=False, budget=False)
        lg = _logits_plain(case, dtype, inp).clone().requires_grad_()
        out = tf_ops.kernel_prediction(inp["src"][..., :3], lg, ks)
        (out * inp["dout"][..., :3]).sum().backward()
        what = "%s %s" % (R.case_id(case), kind)
        _close(ref["out"], out.detach(), what + " out")
        _close(ref["dl_row"][..., lay.off:lay.off + lay.K], lg.grad, what + " d logits")
        rest = ref["dl_row"].clone()
        rest[..., lay.off:lay.off + lay.dl_pad] = R.SENTINEL
        assert bool((rest == R.SENTINEL).all()) and bool((ref["dl_row"][..., lay.off + lay.K:lay.off + lay.dl_pad] == 0).all()), what


def test_symmetric_pad_index_is_the_kernels():
    for P in (1, 2, 3):
        for n in range(P, 12):
            i = torch.arange(-P, n + P)
            want = torch.tensor([(-v - 1) if v < 0 else (2 * n - 1 - v if v >= n else v) for v in i.tolist()])      # sym_index, dd_pointwise.hip
            assert torch.equal(R._index(i, n, "symmetric"), want) and int(want.min()) >= 0 and int(want.max()) < n, (P, n)
        for n in range(1, P):      # below the pad sym_index leaves the image: such shapes are refused, never generated
            i = torch.arange(-P, n + P)
            got = R._index(i, n, "symmetric")
            assert int(got.min()) < 0 or int(got.max()) >= n, (P, n)
            for shape in ((1, n, 8), (1, 8, n)):
                with pytest.raises(ValueError):
                    R.generate(R.Case("vec", 2 * P + 1, shape[0], shape[1], shape[2], 1, 0), "bf16", "real")


def test_dispatch_rule_sends_every_case_down_its_route():
    for case in R.ALL_CASES:
        for dtype in R.DTYPES:
            fwd, bwd = R.EXPECTED_ROUTE[case.route]
            assert R.route_of(case, dtype, True) == fwd and R.route_of(case, dtype, False) == bwd, (case, dtype)
            lay = R.layout(case, dtype)
            assert lay.off + lay.dl_pad < lay.lddl and lay.dl_pad >= lay.K and (lay.off + lay.K2P <= lay.ldl or lay.hid), (case, dtype)
            if lay.hid:
                assert lay.ldw > lay.kh and lay.ldh % lay.N == 0 and lay.kh % lay.N != 0 and R.WB_C0 + case.M * lay.K <= lay.ldw, (case, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("ks", KS)
def test_fp32_emulation_stays_below_every_gate(ks, dtype):
    worst = {}
    for case, dt, kind in _all(ks, dtype):
        inp, ref = R.kpcn_inputs(case, dtype, kind), R.kpcn_reference(case, dtype, kind)
        for order in R.ORDERS:
            emu = R.evaluate(inp, case, dtype, budget=False, order=order)
            for name in OUTPUTS:
                w = R.worst_ratio(emu[name].double(), ref[name], ref["gate_" + name])
                key = (case.route, kind, name, order)
                worst[key] = max(worst.get(key, 0.0), w)
                assert w < 1.0, "%s %s %s %s: the fp32 emulation (%s) is at %.4f of its gate" % (R.case_id(case), dtype, kind, name, order, w)
    for key in sorted(worst):
        print("fp32 emulation ks %d %-4s worst error / gate: %-10s %-6s %-6s %-8s %.3f" % ((ks, dtype) + key + (worst[key],)))


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_the_input_generators_keep_their_promises(dtype):
    for case, dt, kind in _all(None, dtype):
        inp, ref = R.kpcn_inputs(case, dtype, kind), R.kpcn_reference(case, dtype, kind)
        lay = R.layout(case, dtype)
        what = "%s %s %s" % (R.case_id(case), dtype, kind)
        assert ref["arg_min"] >= R.ARG_MIN, what
        for k in ("src", "dout"):
            assert torch.equal(inp[k].float().double(), inp[k]), what
        if lay.hid:
            assert torch.equal(R.representable(inp["hid"], dtype), inp["hid"]) and bool((inp["hid"] >= 0).all()), what
            assert torch.equal(inp["wb"].float().double(), inp["wb"]) and torch.equal(inp["bb"].float().double(), inp["bb"]), what
            if kind == "real" and dtype != "f32":
                col = slice(R.WB_C0, R.WB_C0 + case.M * lay.K)
                for v in (inp["wb"][:lay.kh, col], inp["bb"][col]):
                    assert float((R.representable(v, dtype) != v).double().mean()) > 0.5, what
        else:
            assert torch.equal(R.representable(inp["lg"], dtype), inp["lg"]), what + ": a logit is not representable"
            if kind == "offset":
                same = R.kpcn_inputs(case, dtype, "real")["lg"][..., :case.M * lay.K]
                shifted = inp["lg"][..., :case.M * lay.K] - R.offset_of(case, dtype)
                assert float((shifted - same).abs().max()) <= 0.5 * R.offset_grid(dtype) + 2.0 ** -7 * 8, what      # the same logits, on the grid
        if kind == "real":
            assert ref["spread"] >= 2.0, "%s: median logit spread %.2f" % (what, ref["spread"])
        if kind == "offset" and R.offset_of(case, dtype) == 96.0:
            assert bool(torch.isinf(torch.exp(ref["logits"].float()).sum(-1)).all()), what + ": exp(logit) does not overflow fp32"
            assert float(ref["logits"].min()) >= 80.0, what
        if kind == "flat":
            assert float((ref["p"] - 1.0 / lay.K).abs().max()) < 1e-15, what
        assert bool((ref["gate_out"] > 0).all()) and bool((ref["gate_dl_row"] >= 0).all()), what
        outside = torch.ones(lay.lddl, dtype=torch.bool)
        outside[lay.off:lay.off + lay.K] = False
        assert bool((ref["gate_dl_row"][..., outside] == 0).all()), what


def _finite_ratio(got, ref, gate):
    r = R.ratio(got, ref, gate)
    r = r[gate > 0]
    r = r[torch.isfinite(r)]
    return float(r.max()) if r.numel() else 0.0


def _mutant_factor(mutant):
    """(worst error / gate over every case, kind, type and output -- NaN counts as inf; the same over the elements whose gate is not 0; whether
    any value changed at all)."""
    worst, finite, changed = 0.0, 0.0, False
    for case, dtype, kind in _all():
        ref = R.kpcn_reference(case, dtype, kind)
        got = R.evaluate(R.kpcn_inputs(case, dtype, kind), case, dtype, mut={mutant}, budget=False)
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
    assert len(R.EQUIVALENT_MUTANTS) <= 2 and set(R.EQUIVALENT_MUTANTS) <= set(R.MUTANTS)
    worst, finite, changed = _mutant_factor(mutant)
    print("%-32s worst error / gate %10.3g   (where the gate is not 0: %10.3g)   %s" % (mutant, worst, finite, R.MUTANTS[mutant]))
    if mutant in R.EQUIVALENT_MUTANTS:
        assert not changed, "%s changes a value after all: give it a factor" % mutant
        return
    assert worst >= 1.0, "%s: exceeds no gate (worst error / gate %.3g)" % (mutant, worst)
