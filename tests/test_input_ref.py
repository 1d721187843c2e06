"""CPU tests of tests/input_ref.py, the float64 reference and error budget that tests/test_gpu_input_ops.py gates the input kernels with:
  * the whole-image index arithmetic equals the loop forms of oracle/np_ops.py (variance, pad_symmetric);
  * an f32 emulation of the same formulas (torch float32, division and reciprocal-multiply forms) stays within 1x the budget on every input the
    GPU tests use -- the inputs were chosen so that the reference alone passes -- and within the gate after rounding to each storage type;
  * the gate has teeth: every mutant of MUTANTS, on those same inputs, breaks the gate on at least one element of every case it applies to.
A mutant APPLIES to a case where it changes some element of the float64 result by at least 2 % of that element and by more than 1e-10
(measured between two float64 evaluations, nothing from a device): "1/8 for 1/9" does not apply to a neighbor-mode pass, the channel swap not to a 1-channel pass, and
nothing but the border and count mutants to a constant plane.  Every mutant must apply to a fair share of the cases (MIN_APPLIES), so that an
inapplicable-everywhere mutant cannot pass vacuously."""
import numpy as np
import pytest
import torch

import input_ref as R
from oracle import np_ops

APPLIES = 0.02
FLOOR = 1e-10      # float64's own rounding of a variance that is exactly 0 (a 1x1 image, a constant plane) is ~1e-16: not a change
DTYPES = ("f32", "bf16", "f16")


# ---------------------------------------------------------------------------------------------------------------- against the loop forms
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 2), (1, 5), (3, 1), (4, 7)])
def test_variance_equals_the_loop_form(H, W):
    g = torch.Generator().manual_seed(10 * H + W)
    x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
    for neighbor in (0, 1):
        for relative in (0, 1):
            for compress in (0, 1):
                fp = R.params(use_variance=1, mode_neighbor=neighbor, relative=relative, compress=compress)
                got, _ = R.local_variance(x, torch.zeros_like(x), fp)
                want = np_ops.variance(x.numpy(), "neighbor" if neighbor else "uniform", bool(relative), bool(compress), epsilon=fp["epsilon"])
                assert got.shape == want.shape
                np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 5), (4, 3)])
def test_shifted_equals_pad_symmetric(H, W):
    x = torch.arange(2 * H * W * 2, dtype=torch.float64).view(2, H, W, 2)
    padded = np_ops.pad_symmetric(x.numpy(), 1)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            assert np.array_equal(R.shifted(x, a, b).numpy(), padded[:, 1 + a:1 + a + H, 1 + b:1 + b + W, :])


def test_pixel_record_layout():
    v = R.make_values("signed", 1, 3, 4, 1, 5)
    rec, err = R.pixel_record(v, R.feature_params("signed", "default"))
    assert rec.shape == (1, 3, 4, 4) and torch.equal(rec[..., 0], rec[..., 1]) and torch.equal(rec[..., 0], rec[..., 2])      # replicated, nv = 1
    assert torch.equal(rec[..., 0], (v[..., 0] - R.f32(0.3)) * 0.5) and bool((err >= 0).all())
    rec, _ = R.pixel_record(v, R.feature_params("signed", "uniform_relative_per_channel"))
    assert rec.shape[3] == 4                                                                            # nv = 1 whether compressed or not
    rec, _ = R.pixel_record(R.make_values("signed", 1, 3, 4, 3, 5), R.feature_params("signed", "uniform_relative_per_channel"))
    assert rec.shape[3] == 6
    rec, _ = R.pixel_record(v, R.feature_params("signed", "identity"))
    assert torch.equal(rec, v.expand(-1, -1, -1, 3))


def test_network_input_layout():
    name, T, shape = "late", 1, (1, 2, 2)
    (val, err, recs), = R.assemble_reference(name, T, shape)
    en = R.assemble_entries(name, T, shape)[0]
    assert [e["dst_ch"] for e in en] == [0, 2, 5, 11, 11, 15] and val.shape == (1, 2, 2, 24)
    assert torch.equal(val[..., 0:2], en[0]["src"].view(1, 1, 1, 2).expand(1, 2, 2, 2)) and torch.equal(val[..., 2:5], en[1]["src"])
    assert torch.equal(val[..., 5:11], recs[2][0]) and recs[3] is None and torch.equal(val[..., 11:15], recs[4][0])
    assert not val[..., 19:].any() and not err[..., 19:].any() and not err[..., :5].any()


def test_storage_rounding_is_half_an_ulp():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 3e-6, 0.0, 1000.0], dtype=torch.float64)
    assert torch.equal(R.storage_rounding(x, "bf16"), torch.tensor([2.0 ** -8] * 3 + [2.0 ** -7, 2.0 ** -9, 2.0 ** -27, 2.0 ** -134, 2.0], dtype=torch.float64))
    assert torch.equal(R.storage_rounding(x, "f16"), torch.tensor([2.0 ** -11] * 3 + [2.0 ** -10, 2.0 ** -12, 2.0 ** -25, 2.0 ** -25, 2.0 ** -2], dtype=torch.float64))
    assert not R.storage_rounding(x, "f32").any()
    for dt in ("bf16", "f16"):      # rounding to nearest never exceeds it
        g = torch.Generator().manual_seed(3)
        v = (torch.randn(4000, generator=g, dtype=torch.float64) * 3).float().double()
        assert bool(((R.to_storage(v, dt) - v).abs() <= R.storage_rounding(v, dt)).all())


# ---------------------------------------------------------------------------------------------------------------- the GPU-test inputs
def _evaluations(kind, key):
    """-> (inputs description, reference (value, budget), callable(dtype, form, mut) -> value) of one GPU-test case, tuples concatenated."""
    if kind == "prepare":
        v, fp = R.prepare_inputs(key)
        ref, err = R.prepare_reference(key)
        return ref, err, lambda dtype, form, mut: R.pixel_record(v, fp, dtype, form, mut)[0]
    name, T, shape = key
    refs = R.assemble_reference(name, T, shape)
    entries = R.assemble_entries(name, T, shape)
    c_pad = R.TABLES[name][1]

    def run(dtype, form, mut):
        return torch.cat([R.network_input(en, *shape, c_pad, dtype, form, mut)[0] for en in entries])
    return torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs]), run


ALL_CASES = [("prepare", i) for i in range(len(R.PREPARE_CASES))] + [("assemble", c) for c in R.ASSEMBLE_CASES]


def _case_name(kind, key):
    return R.PREPARE_CASES[key]["name"] if kind == "prepare" else "%s-T%d-%dx%dx%d" % ((key[0], key[1]) + key[2])


def test_reference_values_fit_every_storage_type():
    """fp16 tops out at 65504: no reference value of a case that runs in fp16 comes near it, and every value is finite."""
    for kind, key in ALL_CASES:
        ref, err, _ = _evaluations(kind, key)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(err).all()) and bool((err >= 0).all()), _case_name(kind, key)
        if kind == "assemble":
            assert float(ref.abs().max()) < 3e4, (_case_name(kind, key), float(ref.abs().max()))


def test_f32_emulation_stays_within_the_budget():
    """1x the budget before the store, the gate (2x + r_T) after rounding to the storage type; both forms."""
    worst = {}
    for kind, key in ALL_CASES:
        ref, err, run = _evaluations(kind, key)
        for form in ("div", "rcp"):
            emu = run(torch.float32, form, R.NO_MUTATION)
            w = 2 * R.worst_ratio(emu, ref, err, "f32")      # worst_ratio is against 2x the budget
            worst[(kind, form)] = max(worst.get((kind, form), 0.0), w)
            assert w <= 1.0, "%s (%s): the f32 emulation is %.2f x the budget off the reference" % (_case_name(kind, key), form, w)
            for dt in DTYPES if kind == "assemble" else ("f32",):
                g = R.worst_ratio(R.to_storage(emu, dt), ref, err, dt)
                assert g <= 1.0, "%s (%s, %s): the emulation misses the gate, %.2f" % (_case_name(kind, key), form, dt, g)
    print("worst f32 emulation error / budget:", {k: round(v, 3) for k, v in worst.items()})
    assert min(worst.values()) > 0.02, "the budget is more than 50x what an f32 evaluation needs: %s" % worst


MIN_APPLIES = {"clamp_to_edge": 0, "dst_ch_off_by_one": 56, "epsilon_1e-3": 40, "compress_by_sum": 40, "neighbor_with_diagonal": 60}      # the others: 100 cases


@pytest.mark.parametrize("name", list(R.MUTANTS))
def test_the_gate_has_teeth(name):
    mut = R.mutation(name)
    applied = 0
    for kind, key in ALL_CASES:
        if kind == "prepare" and name == "dst_ch_off_by_one":
            continue                                           # a lone pixel record has no dst_ch
        ref, err, run = _evaluations(kind, key)
        got = run(torch.float64, "div", mut)
        if name in R.EQUIVALENT_MUTANTS:
            assert torch.equal(got, ref), "%s: %s is not equivalent after all" % (_case_name(kind, key), name)
            continue
        diff = (got - ref).abs()
        if not bool(((diff >= APPLIES * ref.abs()) & (diff >= FLOOR)).any()):
            continue
        applied += 1
        for dt in DTYPES if kind == "assemble" else ("f32",):
            w = R.worst_ratio(R.to_storage(got, dt), ref, err, dt)
            assert w > 1.0, "%s (%s): mutant %s passes the gate (worst error / gate %.3f)" % (_case_name(kind, key), dt, name, w)
    print("%s: applies to %d of %d cases" % (name, applied, len(ALL_CASES)))
    assert applied >= MIN_APPLIES.get(name, 100), (name, applied)
