"""Tracked metrics, host side (deepdenoiser_amd/metrics.py) against tests/golden/metrics_golden.*: names, order and values of the reference's
own evaluation branch (Training.model_fn in EVAL mode, executed by tests/golden/make_metrics_golden.py)."""
import copy

import numpy as np
import pytest
import torch

import metrics_util as U
from deepdenoiser_amd import configs
from deepdenoiser_amd import metrics as M
from deepdenoiser_amd.architecture import Architecture
from oracle import training as OT


@pytest.mark.parametrize("case", U.CASES)
def test_plan_names_and_order(case):
    c = U.Case(case)
    assert [e.name for e in c.plan] == c.names
    assert len(set(c.names)) == len(c.names)
    if not c.tj["use_multiscale_metrics"]:
        assert all(e.scale_index == 0 for e in c.plan)


def test_fixture_covers_the_ground():
    by = {n: U.Case(n) for n in U.CASES}
    assert any(e.quantity == "masked_mean" and e.source[0] == "combined" and e.scale_index == 2 for e in by["full_multiscale_smape"].plan)
    assert any(e.source[0] == "image" and e.quantity == "variation_mean" for e in by["full_multiscale_smape"].plan)
    assert by["full_scale0_absolute"].tj["loss_difference"] == "ABSOLUTE"
    assert {e.source[0] for e in by["one_triple_ms_ssim"].plan if e.quantity == "ms_ssim"} == {"feature", "combined"}
    assert any(e.source == ("feature", "Alpha") for e in by["alpha_unmasked"].plan)
    # track_variation alone on the combined level (no weights, no track_mean): the reference builds no combined training (Training.py:1086-1093)
    assert all(e.source[0] == "feature" for e in by["combined_variation_alone"].plan)
    assert by["combined_variation_alone"].tj["combined_features_training_settings"]["statistics"]["track_variation"]


def _arch(combined=None):
    return Architecture(configs.architecture(filters=(4, 6), convs=1, combined=combined), device="cpu")


@pytest.mark.parametrize("level", ["features_training_settings", "combined_features_training_settings"])
@pytest.mark.parametrize("flag,exc", [("track_variation", ValueError), ("track_ms_ssim", NotImplementedError)])
def test_rejected_masked_flags_name_the_key(level, flag, exc):
    no_alpha = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
    tj = configs.training()
    M.metric_plan(_arch(no_alpha), tj, out=lambda *a: None)      # accepted as it is
    tj[level]["statistics_masked"][flag] = True
    with pytest.raises(exc) as e:
        M.metric_plan(_arch(no_alpha), tj, out=lambda *a: None)
    assert "%s.statistics_masked.%s" % (level, flag) in str(e.value)


def test_masked_tracking_with_alpha_is_refused_like_the_reference():
    tj = configs.training()
    tj["features_training_settings"]["statistics_masked"]["track_mean"] = True
    with pytest.raises(Exception) as e:
        M.metric_plan(_arch(), tj, out=lambda *a: None)
    assert "Masking is not supported for the alpha pass" in str(e.value) and "statistics_masked" in str(e.value)
    tj["features_training_settings"]["statistics_masked"]["track_mean"] = False
    assert M.metric_plan(_arch(), tj, out=lambda *a: None)


def test_feature_ms_ssim_with_a_one_channel_pass_is_refused():
    tj = configs.training()
    tj["features_training_settings"]["statistics"]["track_ms_ssim"] = True
    with pytest.raises(ValueError) as e:
        M.metric_plan(_arch(), tj, out=lambda *a: None)
    assert "features_training_settings.statistics.track_ms_ssim" in str(e.value) and "Alpha" in str(e.value)


def test_histogram_flag_only_prints_once():
    M._said_histograms.clear()
    tj = configs.training()
    plain = M.metric_plan(_arch(), tj, out=lambda *a: None)
    tj["features_training_settings"]["statistics"]["track_difference_histogram"] = True
    said = []
    assert M.metric_plan(_arch(), tj, out=said.append) == plain
    assert M.metric_plan(_arch(), tj, out=said.append) == plain
    assert len(said) == 1 and "histograms are not written" in said[0]


def _values(c, real=None):
    tables = {s: c.table(s) for s in c.scales}
    ms = c.ms_values() if any(e.quantity == "ms_ssim" for e in c.plan) else None
    return M.metric_values(c.plan, c.slot_of, tables, c.dims, real, ms)


@pytest.mark.parametrize("case", U.CASES)
def test_values_from_a_float64_table_equal_the_reference(case):
    c = U.Case(case)
    got = _values(c)
    worst = 0.0
    for name, g, w in zip(c.names, got, c.values):
        err = abs(g - w) / max(abs(w), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-12, (name, g, w)
    print("%s: %d metrics, worst relative error %.2e" % (case, len(got), worst))
    masked = [(e, v) for e, v in zip(c.plan, got) if e.quantity == "masked_mean" and e.scale_index == 0]
    for e, v in masked:      # the masks are neither empty nor full: the masked mean is another number than the mean
        mean = [x for f, x in zip(c.plan, got) if f.source == e.source and f.quantity == "mean" and f.scale_index == 0][0]
        assert v != mean and v > 0


def _reference_on_first(c, real):
    """The reference's formulas (oracle/training.py's _FT, checked against the executed reference by tests/test_wiring_golden.py) on the first
    `real` images."""
    import msssim_ref
    kind = c.tj["loss_difference"]
    fts = {}
    for s in range(c.n_scales):
        for src, (p, y, m) in c.sources(s, images=real).items():
            ft = fts.setdefault(src, OT._FT(src[1], kind, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
            ft.predicted.append(p), ft.target.append(y), ft.mask.append(m)
    out = []
    for e in c.plan:
        ft = fts[e.source]
        if e.quantity == "mean":
            out.append(float(ft.mean(e.scale_index)))
        elif e.quantity == "variation_mean":
            out.append(float(ft.variation_mean(e.scale_index)))
        elif e.quantity == "masked_mean":
            out.append(float(ft.masked_mean(e.scale_index)))
        else:
            out.append(float(1.0 - msssim_ref.ms_ssim(ft.predicted[0], ft.target[0]).mean()))
    return out


@pytest.mark.parametrize("case", U.CASES)
def test_real_examples_only(case):
    c = U.Case(case)
    want_all = _reference_on_first(c, c.B)
    for g, w in zip(want_all, c.values):      # the restatement used for the slices reproduces the fixture on the whole batch
        assert abs(g - w) <= 1e-12 * abs(w)
    got, want = _values(c, real=1), _reference_on_first(c, 1)
    assert any(abs(a - b) > 1e-6 * abs(b) for a, b in zip(want, want_all))
    for name, g, w in zip(c.names, got, want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (name, g, w)


def test_empty_mask_gives_zero():
    c = U.Case("full_scale0_absolute")
    tables = {0: c.table(0)}
    tables[0][:, :, 3] = 0.0
    got = M.metric_values(c.plan, c.slot_of, tables, c.dims)
    assert all(v == 0.0 for e, v in zip(c.plan, got) if e.quantity == "masked_mean")


def test_summed_rows_with_a_count():
    """Data parallelism: one row per source = the sum over the images of all ranks, `count` = their number."""
    c = U.Case("full_multiscale_smape")
    tables = {s: c.table(s) for s in c.scales}
    summed = {s: t.sum(axis=1, keepdims=True) for s, t in tables.items()}
    a = M.metric_values(c.plan, c.slot_of, tables, c.dims)
    b = M.metric_values(c.plan, c.slot_of, summed, c.dims, count=c.B)
    assert np.allclose(a, b, rtol=1e-14, atol=0)


def test_accumulator_even_batches_equal_the_plain_mean():
    rng = np.random.RandomState(0)
    batches = rng.rand(5, 7)
    acc = M.MeanAccumulator(7)
    for b in batches:
        acc.add(b, 8)
    assert np.allclose(acc.result(), batches.mean(axis=0), rtol=1e-15, atol=0)


def test_accumulator_padded_last_batch_counts_real_examples():
    a, b = np.array([1.0, 10.0]), np.array([3.0, 30.0])
    acc = M.MeanAccumulator(2)
    acc.add(a, 8)
    acc.add(b, 2)      # 2 real examples, 6 repeats
    assert np.allclose(acc.result(), (8 * a + 2 * b) / 10)
    # two ranks: the states are summed (all-reduce), a rank whose last batch holds repeats only adds nothing
    other = M.MeanAccumulator(2)
    other.add(a, 8)
    merged = M.MeanAccumulator(2).from_state(acc.state() + other.state())
    assert np.allclose(merged.result(), (16 * a + 2 * b) / 18) and merged.weight == 18
    assert M.MeanAccumulator(2).result() == [0.0, 0.0]


def test_combined_levels_follow_training_main():
    tj = configs.training(combined_mean=0.0, image_mean=0.0)
    assert M.combined_levels(tj) == (False, False)
    t2 = copy.deepcopy(tj)
    t2["combined_features_training_settings"]["statistics"]["track_variation"] = True
    assert M.combined_levels(t2) == (False, False)
    t2["combined_features_training_settings"]["statistics_masked"]["track_mean"] = True
    assert M.combined_levels(t2) == (False, True)
    t3 = copy.deepcopy(tj)
    t3["combined_image_training_settings"]["statistics"]["track_mean"] = True
    assert M.combined_levels(t3) == (True, True)
