"""Generates tests/golden/metrics_golden.npz + .json by EXECUTING the reference's evaluation branch (Training.model_fn in EVAL mode,
Training.py:704-719 -> BaseFeatureTraining.add_tracked_metrics_to_dictionary, :283-302) on the stub of make_wiring_golden.py.

`architecture.predict` is replaced by a function that returns seeded prediction dictionaries, so the tracked metrics are functions of the
stored predictions and labels alone (no network, no variables).  Inputs are rounded to fp32 before the reference sees them (float32 storage
loses nothing); the reference computes in float64.  tf.metrics.mean of the stub is the identity, so a metric's value is the value of ONE
batch.  tf.image.ssim_multiscale, which the stub refuses, is bound at run time to tests/msssim_ref.ms_ssim -- a restatement of TensorFlow's
function, like the loss term it pins (README, "unpinned").

Nothing of the reference travels: the .npz holds predictions and labels, the .json the names in dictionary order, their values and the JSON
documents the cases were run on.  Run in the build container only:
    python tests/golden/make_metrics_golden.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_wiring_golden as W  # noqa: E402  (installs the stub, imports the reference's modules)
import msssim_ref  # noqa: E402

from deepdenoiser_amd import configs  # noqa: E402

tf_stub, tf, RefTraining, RefArchitecture, Naming = W.tf_stub, W.tf, W.RefTraining, W.RefArchitecture, W.Naming
MIN_FACTOR = 0.05      # as tests/test_gpu_msssim.py: no MS factor near the relu clamp


def f32(x):
    return x.float().double()


def make_case_inputs(arch, B, H, W_, n_scales, seed, unit_range):
    """labels {target name: [B,H,W,C]} and predictions [scale]{prediction name: [B,h,w,C]}: fp32-exact float64 tensors.  Heavy-tailed with
    exact zeros (the non-zero masks, sign(0)); `unit_range`: values in [0, 1] and scale-0 predictions close to the labels (ms_ssim)."""
    g = torch.Generator().manual_seed(seed)
    labels, preds = {}, [dict() for _ in range(n_scales)]
    for f in arch.feature_predictions:
        if not f.is_target:
            continue
        c = f.number_of_channels
        if not f.load_data:      # a generated member of a COMBINED tuple: the reference's input_fn makes it up, and its prediction echoes it
            one_t = {}
            RefTraining.FeatureTrainingLoader(f).add_to_targets_dictionary(one_t, H, W_)
            (k, v), = one_t.items()
            labels[k] = v[None].repeat(B, 1, 1, 1).double()
            for s in range(n_scales):
                preds[s][Naming.feature_prediction_name(f.name)] = labels[k][:, :H >> s, :W_ >> s, :].clone()
            continue

        def heavy(h, w, keep):
            x = torch.randn(B, h, w, c, generator=g, dtype=torch.float64).abs() * torch.exp(0.5 * torch.randn(B, h, w, 1, generator=g, dtype=torch.float64))
            return f32(x * (torch.rand(B, h, w, 1, generator=g, dtype=torch.float64) > keep))
        if unit_range:
            t = f32(torch.rand(B, H, W_, c, generator=g, dtype=torch.float64) * (torch.rand(B, H, W_, 1, generator=g, dtype=torch.float64) > 0.03))
        else:
            t = heavy(H, W_, 0.2)
        labels[Naming.target_feature_name(f.name)] = t
        for s in range(n_scales):
            h, w = H >> s, W_ >> s
            if unit_range and s == 0:
                p = f32(t + 0.1 * torch.randn(B, h, w, c, generator=g, dtype=torch.float64))
            elif unit_range:
                p = f32(torch.rand(B, h, w, c, generator=g, dtype=torch.float64))
            else:
                p = heavy(h, w, 0.1)
            preds[s][Naming.feature_prediction_name(f.name)] = p
    return labels, preds


def run_case(name, aj, tj, B, H, W_, seed, unit_range=False):
    tf_stub.STORE.reset(seed)
    arch = RefArchitecture.Architecture(copy.deepcopy(aj), source_data_format="channels_last", data_format="channels_last")
    n_scales = 3 if aj["architecture"]["multiscale_prediction"]["use_multiscale_predictions"] else 1
    labels, preds = make_case_inputs(arch, B, H, W_, n_scales, seed + 1, unit_range)
    params = {"architecture": arch, "learning_rate": tj["learning_rate"], "batch_size": tj["batch_size"]}
    params.update(W.build_trainings(arch, aj, copy.deepcopy(tj)))
    arch.predict = lambda features, mode: preds
    factors = []

    def ssim_multiscale(x, y, max_val, power_factors):
        assert max_val == 1.0 and tuple(power_factors) == msssim_ref.POWER_FACTORS
        factors.append(float(msssim_ref.ms_ssim_factors(x, y, power_factors).min()))
        return msssim_ref.ms_ssim(x, y, power_factors)
    tf.image.ssim_multiscale = ssim_multiscale
    spec = RefTraining.model_fn({}, dict(labels), tf.estimator.ModeKeys.EVAL, params)
    names = list(spec.eval_metric_ops.keys())
    values = [float(spec.eval_metric_ops[n]) for n in names]
    # conditions on the inputs: every mask neither empty nor full at scale 0, no MS factor near the clamp
    trainings = list(params["feature_trainings"]) + list(params["combined_feature_trainings"] or [])
    for t in trainings:
        if t.mask_sum:
            assert 0 < float(t.mask_sum[0]) < B * H * W_, (name, t.name, float(t.mask_sum[0]))
    assert all(f > MIN_FACTOR for f in factors), (name, min(factors))
    arrays = {}
    for k, v in labels.items():
        arrays["label:" + k] = v.numpy().astype(np.float32)
        assert (arrays["label:" + k].astype(np.float64) == v.numpy()).all()
    for s, d in enumerate(preds):
        for k, v in d.items():
            arrays["prediction:%d:%s" % (s, k)] = v.numpy().astype(np.float32)
            assert (arrays["prediction:%d:%s" % (s, k)].astype(np.float64) == v.numpy()).all()
    meta = {"architecture_json": aj, "training_json": tj, "B": B, "H": H, "W": W_, "n_scales": n_scales, "names": names, "values": values,
            "loss": float(spec.loss)}
    print("%-28s B=%d %dx%d  %d metrics, loss %.12g%s" % (name, B, H, W_, len(names), meta["loss"],
                                                          ("  min MS factor %.3f" % min(factors)) if factors else ""))
    return meta, arrays


def _stats(tj, level, section, **flags):
    tj[level][section].update(flags)


def cases():
    no_alpha = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
    arch_full = configs.architecture(filters=(4, 6, 8), convs=1, combined=no_alpha)
    levels = ("features_training_settings", "combined_features_training_settings", "combined_image_training_settings")
    c = []
    # (a) every pass but Alpha, 3 scales, SMAPE, mean + variation on all three levels, masked mean on features and combined features
    tj = configs.training()
    for lv in levels:
        _stats(tj, lv, "statistics", track_mean=True, track_variation=True)
    for lv in levels[:2]:
        _stats(tj, lv, "statistics_masked", track_mean=True)
    c.append(("full_multiscale_smape", arch_full, tj, 2, 16, 16, False))
    # (b) the same sources at scale 0 only, ABSOLUTE
    tj = copy.deepcopy(tj)
    tj["use_multiscale_metrics"] = False
    tj["loss_difference"] = "ABSOLUTE"
    c.append(("full_scale0_absolute", arch_full, tj, 2, 16, 16, False))
    # (c) tracked ms_ssim on features and combined features of a one-triple architecture
    one = {"Diffuse": configs._FULL_COMBINED["Diffuse"]}
    tj = configs.training(image_mean=0.0)
    for lv in levels[:2]:
        _stats(tj, lv, "statistics", track_mean=True, track_ms_ssim=True)
    c.append(("one_triple_ms_ssim", configs.architecture(filters=(4, 6, 8), convs=1, combined=one), tj, 2, 48, 44, True))
    # (d) Alpha (1 channel) among the passes, tracked unmasked
    small = {k: configs._FULL_COMBINED[k] for k in ("Diffuse", "Volume", "Emission", "Alpha")}
    tj = configs.training(image_mean=0.0, combined_mean=1.0)
    for lv in levels[:2]:
        _stats(tj, lv, "statistics", track_mean=True, track_variation=True)
    c.append(("alpha_unmasked", configs.architecture(filters=(4, 6, 8), convs=1, combined=small), tj, 2, 16, 16, False))
    # (e) track_variation alone on the combined level, no weights there or on the image: the reference builds no combined training
    tj = configs.training(image_mean=0.0, combined_mean=0.0)
    _stats(tj, levels[1], "statistics", track_mean=False, track_variation=True)
    _stats(tj, levels[0], "statistics", track_mean=True, track_variation=True)
    c.append(("combined_variation_alone", arch_full, tj, 2, 16, 16, False))
    return c


def main():
    meta, arrays = {}, {}
    for i, (name, aj, tj, B, H, W_, unit) in enumerate(cases()):
        m, a = run_case(name, aj, tj, B, H, W_, seed=300 + i, unit_range=unit)
        meta[name] = m
        arrays.update({name + "|" + k: v for k, v in a.items()})
    assert not any(n.startswith("combined") for n in meta["combined_variation_alone"]["names"])
    np.savez_compressed(os.path.join(HERE, "metrics_golden.npz"), **arrays)
    with open(os.path.join(HERE, "metrics_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    size = os.path.getsize(os.path.join(HERE, "metrics_golden.npz")) + os.path.getsize(os.path.join(HERE, "metrics_golden.json"))
    assert size < 2 * 1024 * 1024, size
    print("wrote metrics_golden.npz + .json (%.1f KiB)" % (size / 1024))


if __name__ == "__main__":
    main()
