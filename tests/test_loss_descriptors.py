"""What Program._build_loss asks the loss kernels to do: prog.loss_descs (and prog.ms_ssim_desc) field by field against expectations worked out
here from the architecture and the Training.json -- the reference's rules restated in this file, not taken from deepdenoiser_amd/loss_desc.py.
Every pointer is checked as an offset into the program buffer it must lie in.  Built on the CPU device from the cross-compiled library;
nothing is launched."""
import ctypes as C

import pytest

from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, metrics
from deepdenoiser_amd.architecture import Architecture

LEVELS = ("features_training_settings", "combined_features_training_settings", "combined_image_training_settings")
SMALL = dict(filters=(16, 16), convs=1)
TWO_TRIPLES = {"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
               "Glossy": {"Color": "Glossy Color", "Direct": "Glossy Direct", "Indirect": "Glossy Indirect"}}
NO_ALPHA = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}      # (a features-level ms_ssim weight refuses a loaded 1-channel pass)
VARIATION = dict(feature_variation=0.7, combined_variation=2.0, image_variation=3.0)
IMAGE_COMBINED = ("Diffuse", "Glossy", "Subsurface", "Transmission")                  # CombinedImageFeatureTraining.initialize,
IMAGE_SINGLE = ("Volume Direct", "Volume Indirect", "Emission", "Environment")        # Training.py:475-495


def _masked_two_triples():
    tj = configs.training(image_mean=0.0, masked_mean=0.8, combined_masked_mean=1.7)      # test_masked_mean_loss_terms_parity_f32
    tj[LEVELS[2]]["statistics"]["track_mean"] = False
    return tj


def _ms_ssim_all():
    tj = configs.training(ms_ssim=(0.3, 0.5, 0.7))
    for lv in LEVELS:
        tj[lv]["statistics"].update(track_mean=True, track_variation=True, track_ms_ssim=True, track_difference_histogram=True,
                                    track_variation_difference_histogram=True)
    tj["use_multiscale_metrics"] = True
    return tj


# name: (architecture, Training.json, dtype, (B, H, W))
CASES = {
    "example_f32": (configs.architecture(**SMALL), configs.training(), "f32", (2, 16, 32)),
    "example_bf16": (configs.architecture(**SMALL), configs.training(), "bf16", (2, 16, 32)),
    "variation_f32": (configs.architecture(**SMALL), configs.training(**VARIATION), "f32", (2, 16, 32)),
    "variation_bf16": (configs.architecture(**SMALL), configs.training(**VARIATION), "bf16", (2, 16, 32)),
    "combined_tuples": (configs.architecture(tuple_type="COMBINED", **SMALL), configs.training(), "bf16", (2, 16, 32)),
    "generated_pass": (configs.architecture(combined={"Emission": {"Color": "Emission", "Direct": "", "Indirect": ""}}, **SMALL),
                       configs.bench_training(), "bf16", (2, 16, 32)),
    "invert_before_multiscale": (configs.architecture(invert_after_multiscale=False, **SMALL), configs.training(), "bf16", (2, 16, 32)),
    "masked_two_triples": (configs.architecture(combined=TWO_TRIPLES, **SMALL), _masked_two_triples(), "f32", (2, 16, 32)),
    "ms_ssim_all_levels": (configs.architecture(combined=NO_ALPHA, **SMALL), _ms_ssim_all(), "bf16", (2, 48, 48)),
    # a Training.json whose ONLY combined-features setting is a masked weight: the combined level exists (Training.py:1086-1093)
    "masked_weight_alone": (configs.architecture(combined=TWO_TRIPLES, **SMALL),
                            configs.training(combined_mean=0.0, image_mean=0.0, combined_masked_mean=1.7), "f32", (2, 16, 32)),
}


def _positive(j):
    return bool(j) and (j["mean"] > 0 or j["variation"] > 0 or j["ms_ssim"] > 0)


def _levels(tj):
    """(use the combined image, use the combined features): Training.main, Training.py:1063-1093."""
    ci, cf = tj[LEVELS[2]], tj[LEVELS[1]]
    use_image = _positive(ci["loss_weights"]) or ci["statistics"]["track_mean"]
    use_comb = (use_image or _positive(cf["loss_weights"]) or cf["statistics"]["track_mean"] or _positive(cf.get("loss_weights_masked"))
                or cf.get("statistics_masked", {}).get("track_mean", False))
    return bool(use_image), bool(use_comb)


def _colour_pass(name):
    """The pass whose target defines the mask of `name` (FeatureTraining.initialize, Training.py:379-392).  An '... Indirect' pass masks with
    ITSELF: the reference looks for ' Inirect' when it maps such a pass to its colour pass (RenderPasses.py:88), and the product keeps that."""
    if name.endswith((" Color", " Indirect")) or name in ("Environment", "Emission", "Volume Direct"):
        return name
    if name.endswith(" Direct"):
        return name[:-len(" Direct")] + " Color"
    return None


def _f32(x):
    return C.c_float(x).value


def _build(case, monkeypatch):
    monkeypatch.delenv("DD_FUSE_LOSS_INVERT", raising=False)
    aj, tj, dtype, (B, H, W) = CASES[case]
    arch = Architecture(aj, device="cpu", dtype=dtype, seed=2)
    return arch, tj, arch.program(B, H, W, training_json=tj), B


def _expected_triples(arch, head_names, tj):
    if not _levels(tj)[1]:
        return []
    if arch.feature_prediction_tuple_type == "COMBINED":
        triples = [(t.name, [f.name for f in t.feature_predictions]) for t in arch.feature_prediction_tuples]
    else:
        triples = list(arch.combined_feature_names)
    return [(c, names) for c, names in triples if all(n in head_names for n in names)]


def _check(arch, tj, prog, B):
    tuples = arch.feature_prediction_tuples
    head = [t.feature_predictions[j] for j in range(arch.tuple_size) for t in tuples]      # member-major head order
    names = [f.name for f in head]
    index = {n: i for i, n in enumerate(names)}
    assert [f.name for f in prog.head] == names
    fs, cf, ci = (tj[lv] for lv in LEVELS)
    use_image, _ = _levels(tj)
    triples = _expected_triples(arch, names, tj)
    m_feat, m_comb = fs.get("loss_weights_masked", {}).get("mean", 0.0), cf.get("loss_weights_masked", {}).get("mean", 0.0)
    weights = [lv["loss_weights"] for lv in (fs, cf, ci)]
    ms_ssim = ((weights[0]["ms_ssim"] > 0 and any(f.load_data for f in head)) or (weights[1]["ms_ssim"] > 0 and triples)
               or weights[2]["ms_ssim"] > 0)
    fused = (arch.invert_standardization_after_multiscale_predictions and not ms_ssim and all(wt["variation"] == 0 for wt in weights))
    n_scales = arch.number_of_scales() if tj["use_multiscale_loss"] else 1
    norm = 1.0 / sum(1.0 / 4.0 ** s for s in range(n_scales))
    nm = L.MAX_FEATURES + L.MAX_COMBINED
    assert len(prog.loss_descs) == n_scales
    for s, (d, msums) in enumerate(prog.loss_descs):
        h, w = prog.H >> s, prog.W >> s
        sf = norm / 4.0 ** s
        block = B * h * w * 3 * 4
        P = prog.predictions[s]
        rec = prog.loss_inverts.get(s)      # (standardized prediction, groups) of an inversion the loss head runs itself
        assert (rec is not None) == (fused and any(f.load_data for f in head)), "the fused inversion is taken exactly when nothing rules it out"
        grad = (rec[0] if rec is not None else P).gstate["buf"]
        assert d.n_features == len(head) and d.kind == {"SMAPE": 5, "SMOOTH_ABSOLUTE": 3}[tj["loss_difference"]] and d.epsilon == _f32(1e-2)
        masked = False
        for i, f in enumerate(head):
            assert (d.target[i], d.target_ld[i], d.nch[i]) == (prog.targets[s].data_ptr() + i * block, 3, f.number_of_channels), f.name
            assert d.pred_ld[i] == 3
            if f.load_data:
                assert d.pred[i] == P.buf.data_ptr() + i * block and d.dpred[i] == grad.data_ptr() + i * block, f.name
                assert d.pred_std[i] == (rec[0].buf.data_ptr() + i * block if rec is not None else None), f.name
                assert d.pred_inv[i] == (d.pred[i] if rec is not None else None), f.name
                assert (d.weight[i], d.var_weight[i]) == (_f32(weights[0]["mean"] * sf), _f32(weights[0]["variation"] * sf)), f.name
                cp = _colour_pass(f.name) if m_feat > 0 else None
                assert d.mask_feature[i] == (index[cp] if cp is not None else -1), f.name
                assert d.masked_weight[i] == (_f32(m_feat * sf) if cp is not None else 0.0), f.name
                masked = masked or cp is not None
            else:      # a generated pass: the echo of its source, no loss, a gradient nobody reads
                assert d.pred[i] == prog.echo[(f.name, s)].data_ptr() and d.dpred[i] == prog._dummy_dpred[s].data_ptr(), f.name
                assert (d.weight[i], d.var_weight[i], d.masked_weight[i], d.mask_feature[i]) == (0.0, 0.0, 0.0, -1), f.name
                assert d.pred_std[i] is None and d.pred_inv[i] is None
        assert d.n_combined == len(triples)
        for k, (cname, members) in enumerate(triples):      # in the order of the architecture
            assert list(d.comb[k]) == [index[n] for n in members], cname
            assert (d.comb_weight[k], d.comb_var_weight[k]) == (_f32(weights[1]["mean"] * sf), _f32(weights[1]["variation"] * sf)), cname
            assert d.comb_masked_weight[k] == _f32(m_comb * sf), cname
            assert d.comb_mask_feature[k] == (index[members[0]] if m_comb > 0 else -1), cname      # the triple's colour pass
            masked = masked or m_comb > 0
        if use_image:
            by_name = {c: k for k, (c, _) in enumerate(triples)}
            assert list(d.image_combined[:d.n_image_combined]) == [by_name[c] for c in IMAGE_COMBINED]
            assert list(d.image_features[:d.n_image_features]) == [index[n] for n in IMAGE_SINGLE]
            assert (d.image_weight, d.image_var_weight) == (_f32(weights[2]["mean"] * sf), _f32(weights[2]["variation"] * sf))
        else:
            assert (d.n_image_combined, d.n_image_features, d.image_weight, d.image_var_weight) == (0, 0, 0.0, 0.0)
        assert d.mask_sums == (prog.mask_sums.data_ptr() + s * nm * 4 if masked else None)
        assert (msums is not None) == masked and (not masked or msums.data_ptr() == d.mask_sums)
    return head, triples, weights, bool(ms_ssim)


@pytest.mark.parametrize("case", [c for c in CASES if c != "masked_weight_alone"])
def test_loss_descriptors(lib, monkeypatch, case):
    arch, tj, prog, B = _build(case, monkeypatch)
    head, triples, weights, ms_ssim = _check(arch, tj, prog, B)
    assert (getattr(prog, "ms_ssim_desc", None) is not None) == ms_ssim
    if not ms_ssim:
        return
    # the ms_ssim term: the sources of scale 0's loss launch, the three weights without the multi-scale factor (Training.py:231-232)
    d, m = prog.loss_descs[0][0], prog.ms_ssim_desc[0]
    assert (m.n_features, m.n_combined, m.n_image_combined, m.n_image_features) == (d.n_features, d.n_combined, d.n_image_combined,
                                                                                     d.n_image_features)
    assert m.n_combined == len(triples) > 0 and m.n_image_combined == 4 and m.n_image_features == 4
    for i, f in enumerate(head):
        assert (m.pred[i], m.target[i], m.pred_ld[i], m.target_ld[i], m.nch[i]) == (d.pred[i], d.target[i], d.pred_ld[i], d.target_ld[i], d.nch[i])
        assert m.dpred[i] == (d.dpred[i] if f.load_data else None), f.name
        assert m.ssim_weight[i] == (_f32(weights[0]["ms_ssim"]) if f.load_data else 0.0), f.name
    for k in range(m.n_combined):
        assert list(m.comb[k]) == list(d.comb[k]) and m.comb_ssim_weight[k] == _f32(weights[1]["ms_ssim"])
    assert list(m.image_combined[:4]) == list(d.image_combined[:4]) and list(m.image_features[:4]) == list(d.image_features[:4])
    assert m.image_ssim_weight == _f32(weights[2]["ms_ssim"])


def test_masked_combined_weight_alone_builds_the_combined_level(lib, monkeypatch):
    """loss_weights_masked of the combined features is one of the settings that make the combined level exist (Training.py:1086-1093): the
    two triples are evaluated with the masked weight, 1.7 * norm / 4**s, and nothing else."""
    arch, tj, prog, B = _build("masked_weight_alone", monkeypatch)
    assert metrics.combined_levels(tj) == (False, True)
    _check(arch, tj, prog, B)
    n_scales = len(prog.loss_descs)
    norm = 1.0 / sum(1.0 / 4.0 ** s for s in range(n_scales))
    for s, (d, msums) in enumerate(prog.loss_descs):
        assert d.n_combined == len(metrics.combined_triples(arch)) == 2
        assert [d.comb_masked_weight[k] for k in range(2)] == [_f32(1.7 * norm / 4.0 ** s)] * 2
        assert [d.comb_weight[k] for k in range(2)] == [0.0, 0.0] and d.mask_sums is not None and msums is not None
    assert prog.masked
