"""Tracked metrics: the `statistics` / `statistics_masked` sections of Training.json.

The reference writes them as TensorBoard scalars every 100 steps while training (BaseFeatureTraining.add_tracked_summaries,
Training.py:246-265, 688-698, 1214) and as eval_metric_ops averaged over the validation set (add_tracked_metrics_to_dictionary,
Training.py:283-302, 704-719, 874-877).  This module holds the host side: which metrics a configuration asks for, in the reference's order
and under its names (metric_plan), how the per-image sums of dd_loss_metrics / dd_loss_msssim_values (include/dd_hip.h) become their values
(metric_values), and the running mean over batches (MeanAccumulator).  The launches are Program.metrics() (program.py).

Not built: the four *_histogram flags (said once on stdout, then ignored).
"""
import collections

import numpy as np

from .naming import Naming
from .render_passes import RenderPasses

MetricEntry = collections.namedtuple("MetricEntry", "name source quantity scale_index")
# source: ("feature", pass name) | ("combined", combined name) | ("image", "Combined")
# quantity: "mean" | "variation_mean" | "masked_mean" | "ms_ssim"
IMAGE_NAME = "Combined"      # RenderPasses.COMBINED: the name Training.main gives the CombinedImageFeatureTraining
_LEVELS = ("features_training_settings", "combined_features_training_settings", "combined_image_training_settings")
_HISTOGRAMS = ("track_difference_histogram", "track_variation_difference_histogram")
_said_histograms = []


def _weights_positive(j):
    return bool(j) and (j["mean"] > 0. or j["variation"] > 0. or j["ms_ssim"] > 0.)


def combined_levels(training_json):
    """(use_combined_image, use_combined_features) exactly as Training.main decides them (Training.py:1063-1093): the weights and track_mean
    are consulted, nothing else (the reference tests track_mean five times over) -- track_variation or track_ms_ssim alone on a level
    without weights and without track_mean builds no combined training and therefore yields no metric."""
    ci, cf = training_json[_LEVELS[2]], training_json[_LEVELS[1]]
    use_image = _weights_positive(ci["loss_weights"]) or bool(ci["statistics"]["track_mean"])
    use_comb = (use_image or _weights_positive(cf["loss_weights"]) or bool(cf["statistics"]["track_mean"])
                or _weights_positive(cf.get("loss_weights_masked")) or bool(cf.get("statistics_masked", {}).get("track_mean", False)))
    return use_image, use_comb


def mask_pass(name):
    """FeatureTraining.initialize, Training.py:379-392: the colour pass whose target defines the mask of pass `name`, or None."""
    if RenderPasses.is_color_render_pass(name) or name in ("Environment", "Emission", "Volume Direct", "Volume Indirect"):
        return name
    if RenderPasses.is_direct_or_indirect_render_pass(name):
        return RenderPasses.direct_or_indirect_to_color_render_pass(name)
    return None


def combined_triples(arch):
    """(combined name, [color, direct, indirect] pass names) of the combined features whose three members are all target passes of `arch`
    (Training.py:1095-1141 for SINGLE tuples, :1143-1147 for COMBINED ones)."""
    targets = {f.name for f in arch.feature_predictions if f.is_target}
    if arch.feature_prediction_tuple_type == "COMBINED":
        triples = [(t.name, [f.name for f in t.feature_predictions]) for t in arch.feature_prediction_tuples]
    else:
        triples = list(arch.combined_feature_names)
    return [(c, names) for c, names in triples if all(n in targets for n in names)]


def _flags(section):
    section = section or {}
    return {k: bool(section.get(k, False)) for k in ("track_mean", "track_variation", "track_ms_ssim") + _HISTOGRAMS}


def _check_masked(level, flags):
    key = level + ".statistics_masked."
    if flags["track_variation"]:
        raise ValueError("%strack_variation cannot be tracked: the reference multiplies the [B, pairs] variation difference by the [B,H,W,1] "
                         "mask (BaseFeatureTraining.masked_variation_difference, Training.py:146-149), which has no meaning" % key)
    if flags["track_ms_ssim"]:
        raise NotImplementedError("%strack_ms_ssim: Not implemented (BaseFeatureTraining.masked_ms_ssim raises the same, Training.py:206-207)" % key)


def metric_plan(arch, training_json, out=print):
    """The ordered list of MetricEntry that the reference's add_tracked_metrics_to_dictionary calls produce for `arch` (an Architecture; no
    device is touched) and a parsed Training.json: the feature trainings in Training.main's order (target passes; a generated pass, load_data
    false, tracks nothing: Training.py:1020-1044), the combined feature trainings, the combined image training.  Per source: mean and
    variation mean of every scale (scale 0 only unless use_multiscale_metrics), ms_ssim once, then the masked mean of every scale.

    statistics_masked of the features level applies to passes that have a corresponding colour pass (Training.py:379-392).  For any other
    loaded pass the reference would index an empty mask list and fail; such a pass is LEFT OUT here (Alpha is refused like the reference).

    Raises, naming the key, when a flag that cannot be served is true: statistics_masked.track_variation, statistics_masked.track_ms_ssim,
    any masked tracking with an Alpha pass, track_ms_ssim of the features level with a loaded 1-channel pass (Program._check_ms_ssim adds
    the tile-size rule when the launches are built).  A *_histogram flag is reported once through `out` and ignored."""
    tj = training_json
    fs, cf, ci = (tj[k] for k in _LEVELS)
    stat = [_flags(lv.get("statistics")) for lv in (fs, cf, ci)]
    masked = [_flags(lv.get("statistics_masked")) for lv in (fs, cf, ci)]
    if any(s[h] for s in stat + masked for h in _HISTOGRAMS) and not _said_histograms:
        _said_histograms.append(True)
        out("tracked metrics: the *_histogram flags of Training.json are set, but histograms are not written")
    loaded = [f for f in arch.feature_predictions if f.is_target and f.load_data]
    if any(masked[0].values()) and any(f.name == "Alpha" for f in loaded):      # Training.py:103-113
        raise Exception("Masking is not supported for the alpha pass, because it does not seem to make sense. "
                        "(features_training_settings.statistics_masked)")
    for level, m in zip(_LEVELS, masked):
        _check_masked(level, m)
    if stat[0]["track_ms_ssim"]:
        for f in loaded:
            if f.number_of_channels != 3:
                raise ValueError("features_training_settings.statistics.track_ms_ssim cannot be used with the loaded 1-channel target pass '%s': "
                                 "the reference transposes such a tensor into an image 1 pixel high (Training.py:187-190)" % f.name)
    scales = range(arch.number_of_scales() if tj["use_multiscale_metrics"] else 1)
    plan = []

    def add(source, name, s, m, has_mask):      # BaseFeatureTraining.add_tracked_metrics_to_dictionary, Training.py:283-302
        for k in scales:
            if s["track_mean"]:
                plan.append(MetricEntry(Naming.mean_name(name, scale_index=k), source, "mean", k))
            if s["track_variation"]:
                plan.append(MetricEntry(Naming.variation_mean_name(name, scale_index=k), source, "variation_mean", k))
        if s["track_ms_ssim"]:
            plan.append(MetricEntry(Naming.ms_ssim_name(name), source, "ms_ssim", 0))
        for k in scales:
            if m["track_mean"] and has_mask:
                plan.append(MetricEntry(Naming.mean_name(name, masked=True, scale_index=k), source, "masked_mean", k))

    for f in loaded:
        add(("feature", f.name), f.name, stat[0], masked[0], mask_pass(f.name) is not None)
    use_image, use_comb = combined_levels(tj)
    if use_comb:
        for cname, _ in combined_triples(arch):
            add(("combined", cname), cname, stat[1], masked[1], True)
    if use_image:
        add(("image", IMAGE_NAME), IMAGE_NAME, stat[2], _flags(None), False)
    return plan


def metric_values(plan, slot_of, tables, dims, real=None, ms_values=None, count=None):
    """Values of `plan`, in order, as Python floats.

    tables[k]: array [rows, B, 4] of scale k as dd_loss_metrics leaves it (per source row `slot_of[source]` and image: sum of difference,
    sum of variation difference, sum of difference * mask, sum of mask); dims[k] = (H, W) of scale k; ms_values[source] = [B] values MS of
    dd_loss_msssim_values.  The images 0 .. real-1 are evaluated (None: all), n of them -- or `count`, when the rows already are sums
    over that many images (data parallelism).  Sums over images in float64, then
      mean = S0 / (n H W)                        (Training.py:126-129, LossDifference sums the channels)
      variation_mean = S1 / (n (H (W-1) + (H-1) W))   (:139-176)
      masked_mean = S2 / S3 if S3 > 0 else 0     (:131-137: the mask sum of the evaluated images)
      ms_ssim = 1 - mean over images of MS       (:203)"""
    out = []
    for e in plan:
        if e.quantity == "ms_ssim":
            ms = np.asarray(ms_values[e.source], dtype=np.float64)
            ms = ms if real is None else ms[:real]
            out.append(float(1.0 - ms.sum() / (count or ms.shape[0])))
            continue
        t = np.asarray(tables[e.scale_index], dtype=np.float64)[slot_of[e.source]]
        t = t if real is None else t[:real]
        n = count or t.shape[0]
        s = t.sum(axis=0)
        h, w = dims[e.scale_index]
        if e.quantity == "mean":
            out.append(float(s[0] / (n * h * w)))
        elif e.quantity == "variation_mean":
            out.append(float(s[1] / (n * (h * (w - 1) + (h - 1) * w))))
        else:
            out.append(float(s[2] / s[3]) if s[3] > 0 else 0.0)
    return out


class MeanAccumulator:
    """tf.metrics.mean over batches, weighted by the number of real examples of each batch (as run_validation weighs the loss): for a data
    set that divides evenly this is the reference's plain mean of the batch values.  state() / from_state() carry numerators and weight
    through an all-reduce (sum)."""

    def __init__(self, n):
        self.num = np.zeros(n, dtype=np.float64)
        self.weight = 0.0

    def add(self, values, weight):
        self.num += np.asarray(values, dtype=np.float64) * float(weight)
        self.weight += float(weight)

    def state(self):
        return np.concatenate([self.num, [self.weight]])

    def from_state(self, state):
        state = np.asarray(state, dtype=np.float64)
        self.num, self.weight = state[:-1].copy(), float(state[-1])
        return self

    def result(self):
        return [float(v) for v in (self.num / self.weight if self.weight > 0 else np.zeros_like(self.num))]
