"""Generates tests/golden/histogram_golden.json by EXECUTING the reference's training branch (Training.model_fn in TRAIN mode,
Training.py:679-686 -> BaseFeatureTraining.add_tracked_histograms, :267-281) on the stub of make_wiring_golden.py, for the five cases of
make_metrics_golden.py: the same JSON documents, predictions and labels (tests/golden/metrics_golden.npz), with the histogram flags switched on
at all levels (tests/histogram_ref.with_histogram_flags; the case with an Alpha pass without the masked ones: the reference refuses any
masking there, Training.py:103-113).

tf.summary.histogram of the stub module is bound at run time to a recorder: the fixture holds, per case, the tags in call order and per tag
num / min / max / sum / sum_squares of the float64 tensor the reference passed.  It also records that a run with
statistics_masked.track_variation_difference_histogram fails inside the reference (a [B, pairs] tensor times a [B,H,W,1] mask).

Nothing of the reference travels: names and numbers only.  Run in the build container only:
    python tests/golden/make_histogram_golden.py
"""
import copy
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_metrics_golden as G  # noqa: E402  (imports make_wiring_golden: the stub is installed, the reference's modules run on it)
import histogram_ref  # noqa: E402
import msssim_ref  # noqa: E402

W, tf, tf_stub, RefTraining, RefArchitecture = G.W, G.tf, G.tf_stub, G.RefTraining, G.RefArchitecture


def run_train(aj, tj, B, H, W_, seed, unit_range, stored=None):
    """Training.model_fn(TRAIN) on the inputs of make_metrics_golden.run_case; returns [(tag, float64 numpy values)] in call order."""
    tf_stub.STORE.reset(seed)
    arch = RefArchitecture.Architecture(copy.deepcopy(aj), source_data_format="channels_last", data_format="channels_last")
    n_scales = 3 if aj["architecture"]["multiscale_prediction"]["use_multiscale_predictions"] else 1
    labels, preds = G.make_case_inputs(arch, B, H, W_, n_scales, seed + 1, unit_range)
    if stored is not None:      # the very tensors of metrics_golden.npz
        for k, v in labels.items():
            assert np.array_equal(stored["label:" + k].astype(np.float64), v.numpy()), k
        for s, d in enumerate(preds):
            for k, v in d.items():
                assert np.array_equal(stored["prediction:%d:%s" % (s, k)].astype(np.float64), v.numpy()), k
    params = {"architecture": arch, "learning_rate": tj["learning_rate"], "batch_size": tj["batch_size"]}
    params.update(W.build_trainings(arch, aj, copy.deepcopy(tj)))
    arch.predict = lambda features, mode: preds
    tf.image.ssim_multiscale = lambda x, y, max_val, power_factors: msssim_ref.ms_ssim(x, y, power_factors)
    calls = []
    tf.summary.histogram = lambda name, tensor, *a, **k: calls.append((name, tensor.detach().double().reshape(-1).numpy().copy()))
    try:
        RefTraining.model_fn({}, dict(labels), tf.estimator.ModeKeys.TRAIN, params)
    finally:
        tf.summary.histogram = lambda *a, **k: None
    return calls


def main():
    npz = np.load(os.path.join(HERE, "metrics_golden.npz"))
    meta = {"cases": {}}
    total = 0
    for i, (name, aj, tj, B, H, W_, unit) in enumerate(G.cases()):
        stored = {k.split("|", 1)[1]: npz[k] for k in npz.files if k.startswith(name + "|")}
        masked = True
        try:
            calls = run_train(aj, histogram_ref.with_histogram_flags(tj, True), B, H, W_, 300 + i, unit, stored)
        except Exception as e:      # noqa: BLE001  (Training.py:103-113: no masking with an Alpha pass)
            if "alpha pass" not in str(e):
                raise
            masked = False
            calls = run_train(aj, histogram_ref.with_histogram_flags(tj, False), B, H, W_, 300 + i, unit, stored)
        tags = [t for t, _ in calls]
        assert len(set(tags)) == len(tags), name
        stats = {}
        for t, v in calls:
            assert np.isfinite(v).all()
            stats[t] = {"num": int(v.size), "min": float(v.min()), "max": float(v.max()), "sum": float(v.sum()), "sum_squares": float((v * v).sum())}
            total += v.size
        meta["cases"][name] = {"masked": masked, "tags": tags, "stats": stats}
        print("%-28s masked=%d  %d histograms, %d values" % (name, masked, len(tags), sum(s["num"] for s in stats.values())))
    # a masked variation histogram cannot run in the reference
    name, aj, tj, B, H, W_, unit = G.cases()[0]
    bad = histogram_ref.with_histogram_flags(tj, True)
    bad["features_training_settings"]["statistics_masked"]["track_variation_difference_histogram"] = True
    try:
        run_train(aj, bad, B, H, W_, 300, unit)
        failed = None
    except Exception as e:      # noqa: BLE001
        failed = type(e).__name__
    assert failed is not None
    meta["masked_variation_difference_histogram"] = {"case": name, "key": "features_training_settings.statistics_masked.track_variation_difference_histogram",
                                                     "fails_in_reference": True, "error_type": failed}
    meta["values_total"] = total
    path = os.path.join(HERE, "histogram_golden.json")
    with open(path, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    print("wrote histogram_golden.json (%.1f KiB), %d values in all; masked variation: %s" % (os.path.getsize(path) / 1024, total, failed))


if __name__ == "__main__":
    main()
