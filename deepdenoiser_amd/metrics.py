"""Tracked metrics: the `statistics` / `statistics_masked` sections of Training.json.

The reference writes them as TensorBoard scalars every 100 steps while training (BaseFeatureTraining.add_tracked_summaries,
Training.py:246-265, 688-698, 1214) and as eval_metric_ops averaged over the validation set (add_tracked_metrics_to_dictionary,
Training.py:283-302, 704-719, 874-877).  This module holds the host side: which metrics a configuration asks for, in the reference's order
and under its names (metric_plan), how the per-image sums of dd_loss_metrics / dd_loss_msssim_values (include/dd_hip.h) become their values
(metric_values), and the running mean over batches (MeanAccumulator).  The launches are Program.metrics() (built in tracking.py).

Histograms (the four *_histogram flags; BaseFeatureTraining.add_tracked_histograms, Training.py:267-281, written in TRAIN mode only, :679-686):
histogram_plan lists the tags in the reference's call order, histogram_limits is TensorFlow's default bucket table, decode_histogram_records /
histogram_values turn the device records of dd_histogram_values / dd_loss_histograms (include/dd_hip.h) into what a HistogramProto holds
(Histogram::EncodeToProto with the empty buckets collapsed), merge_histogram_tables adds the tables of several ranks.  The TensorFlow side is
restated from tensorflow/core/lib/histogram/histogram.cc (PARITY UNPINNED, like ssim_multiscale and the event format).  The launches are
Program.histograms(); `python -m deepdenoiser_amd.train --histograms` writes them.  metric_plan alone still says once that the flags are set
and nothing is written, unless its caller passes histograms=True.

Image summaries (new functionality: the reference writes none): preview_plan lists the sources whose source | prediction | target previews
dd_loss_previews (include/dd_hip.h) renders, preview_thresholds is the table it compares against -- the sRGB transfer function lives here,
on the host, the device only counts table entries --, preview_tags names the images the way TF 1.x's tf.summary.image does.  The launch is
Program.previews(); `python -m deepdenoiser_amd.train --image_steps N` writes them.
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


def _levels(arch, tj):
    """(statistics flags, statistics_masked flags) of the three levels and the loaded target passes, after the checks metric_plan and
    histogram_plan share: Alpha with any masked flag, statistics_masked.track_variation, statistics_masked.track_ms_ssim."""
    fs, cf, ci = (tj[k] for k in _LEVELS)
    stat = [_flags(lv.get("statistics")) for lv in (fs, cf, ci)]
    masked = [_flags(lv.get("statistics_masked")) for lv in (fs, cf, ci)]
    loaded = [f for f in arch.feature_predictions if f.is_target and f.load_data]
    if any(masked[0].values()) and any(f.name == "Alpha" for f in loaded):      # Training.py:103-113
        raise Exception("Masking is not supported for the alpha pass, because it does not seem to make sense. "
                        "(features_training_settings.statistics_masked)")
    for level, m in zip(_LEVELS, masked):
        _check_masked(level, m)
    return stat, masked, loaded


def metric_plan(arch, training_json, out=print, histograms=False):
    """The ordered list of MetricEntry that the reference's add_tracked_metrics_to_dictionary calls produce for `arch` (an Architecture; no
    device is touched) and a parsed Training.json: the feature trainings in Training.main's order (target passes; a generated pass, load_data
    false, tracks nothing: Training.py:1020-1044), the combined feature trainings, the combined image training.  Per source: mean and
    variation mean of every scale (scale 0 only unless use_multiscale_metrics), ms_ssim once, then the masked mean of every scale.

    statistics_masked of the features level applies to passes that have a corresponding colour pass (Training.py:379-392).  For any other
    loaded pass the reference would index an empty mask list and fail; such a pass is LEFT OUT here (Alpha is refused like the reference).

    Raises, naming the key, when a flag that cannot be served is true: statistics_masked.track_variation, statistics_masked.track_ms_ssim,
    any masked tracking with an Alpha pass, track_ms_ssim of the features level with a loaded 1-channel pass (loss_desc.check_ms_ssim adds
    the tile-size rule when the launches are built).  A *_histogram flag is not this plan's business (histogram_plan): a caller that does
    not write histograms (histograms=False) has that said once through `out`."""
    tj = training_json
    stat, masked, loaded = _levels(arch, tj)
    if not histograms and any(s[h] for s in stat + masked for h in _HISTOGRAMS) and not _said_histograms:
        _said_histograms.append(True)
        out("tracked metrics: the *_histogram flags of Training.json are set, but histograms are not written")
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


# ---------------------------------------------------------------------------------------------------------------- histograms
HistogramEntry = collections.namedtuple("HistogramEntry", "tag source kind scale_index")
# kind: "difference" | "variation_difference" | "masked_difference" (DD_HISTOGRAM_* of include/dd_hip.h, in this order)
HISTOGRAM_KINDS = ("difference", "variation_difference", "masked_difference")
_STAT_KEYS = ("min", "max", "sum", "sum_squares")
_said_nonfinite = set()


def histogram_limits():
    """TensorFlow's default bucket limits (InitDefaultBucketsInner, histogram.cc): v = 1e-12, while v < 1e20: append v, v *= 1.1 (IEEE double);
    then DBL_MAX; the list is the negated list reversed, 0.0, the list.  1551 float64 values, [775] == 0.0."""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(np.finfo(np.float64).max)
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)


def histogram_plan(arch, training_json):
    """The ordered list of HistogramEntry that the reference's add_tracked_histograms calls produce (Training.py:267-281, 679-686): sources in
    Training.main's order; per source and scale (scale 0 only unless use_multiscale_metrics) the difference, the variation difference, then
    the masked difference.  The rules of metric_plan hold: generated passes track nothing, a masked flag on a pass without a colour pass is
    left out, Alpha with any masked flag raises, the combined levels exist only when combined_levels() says so.

    statistics_masked.track_variation_difference_histogram raises, naming the key: like statistics_masked.track_variation it multiplies a
    [B, pairs] tensor by a [B,H,W,1] mask."""
    tj = training_json
    stat, masked, loaded = _levels(arch, tj)
    for level, m in zip(_LEVELS, masked):
        if m["track_variation_difference_histogram"]:
            raise ValueError("%s.statistics_masked.track_variation_difference_histogram cannot be tracked: the reference multiplies the "
                             "[B, pairs] variation difference by the [B,H,W,1] mask (BaseFeatureTraining.masked_variation_difference, "
                             "Training.py:146-149), which has no meaning" % level)
    scales = range(arch.number_of_scales() if tj["use_multiscale_metrics"] else 1)
    plan = []

    def add(source, name, s, m, has_mask):
        for k in scales:
            if s["track_difference_histogram"]:
                plan.append(HistogramEntry(Naming.difference_name(name, scale_index=k), source, "difference", k))
            if s["track_variation_difference_histogram"]:
                plan.append(HistogramEntry(Naming.variation_difference_name(name, scale_index=k), source, "variation_difference", k))
            if m["track_difference_histogram"] and has_mask:
                plan.append(HistogramEntry(Naming.difference_name(name, masked=True, scale_index=k), source, "masked_difference", k))

    for f in loaded:
        add(("feature", f.name), f.name, stat[0], masked[0], mask_pass(f.name) is not None)
    use_image, use_comb = combined_levels(tj)
    if use_comb:
        for cname, _ in combined_triples(arch):
            add(("combined", cname), cname, stat[1], masked[1], True)
    if use_image:
        add(("image", IMAGE_NAME), IMAGE_NAME, stat[2], _flags(None), False)
    return plan


def decode_histogram_records(raw, n, nb):
    """n device records (include/dd_hip.h: uint32 counts[nb] | double min, max, sum, sum_squares | uint64 num, nonfinite) as a host TABLE:
    {"counts": int64 [n, nb], "min" / "max" / "sum" / "sum_squares": float64 [n], "num" / "nonfinite": int64 [n]}."""
    off = (nb + 1) // 2 * 8
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).reshape(n, off + 48))
    stats = np.ascontiguousarray(raw[:, off:off + 32]).view(np.float64)
    nums = np.ascontiguousarray(raw[:, off + 32:off + 48]).view(np.uint64).astype(np.int64)
    table = {"counts": np.ascontiguousarray(raw[:, :4 * nb]).view(np.uint32).astype(np.int64)}
    table.update({k: stats[:, j].copy() for j, k in enumerate(_STAT_KEYS)})
    table["num"], table["nonfinite"] = nums[:, 0].copy(), nums[:, 1].copy()
    return table


_ADD_KEYS = ("counts", "num", "nonfinite", "sum", "sum_squares")


def histogram_reduce_pack(table):
    """A table as the two float64 vectors a merge works on: `adds` (counts, num, nonfinite, sum, sum_squares: they ADD; a count is exact in
    a double up to 2^53) and `ext` ([max, -min]: the element-wise MAXIMUM is taken).  train.py all-reduces them (SUM, MAX)."""
    adds = np.concatenate([np.asarray(table[k], dtype=np.float64).reshape(-1) for k in _ADD_KEYS])
    ext = np.concatenate([np.asarray(table["max"], dtype=np.float64), -np.asarray(table["min"], dtype=np.float64)])
    return adds, ext


def histogram_reduce_unpack(adds, ext, n, nb):
    """The table of n records with nb buckets from reduced `adds` / `ext` vectors."""
    adds, ext = np.asarray(adds, dtype=np.float64), np.asarray(ext, dtype=np.float64)
    assert adds.size == n * nb + 4 * n and ext.size == 2 * n, "not the vectors of histogram_reduce_pack"
    table, at = {}, 0
    for k in _ADD_KEYS:
        size = n * nb if k == "counts" else n
        part = adds[at:at + size]
        table[k] = part.copy() if k in ("sum", "sum_squares") else np.rint(part).astype(np.int64)
        at += size
    table["counts"] = table["counts"].reshape(n, nb)
    table["max"], table["min"] = ext[:n].copy(), -ext[n:]
    return table


def merge_histogram_tables(tables):
    """The table of the values of all `tables` together (the ranks of a data-parallel run): counts, num, nonfinite, sum and sum_squares add,
    min / max are taken -- the SUM and the MAX that train.py's two all-reduces apply to the vectors of histogram_reduce_pack."""
    packed = [histogram_reduce_pack(t) for t in tables]
    n, nb = tables[0]["counts"].shape
    return histogram_reduce_unpack(np.sum([a for a, _ in packed], axis=0), np.max([e for _, e in packed], axis=0), n, nb)


def compress_buckets(limits, counts):
    """Histogram::EncodeToProto without preserve_zero_buckets: every non-empty bucket is an entry (its limit, its count); a run of empty
    buckets collapses into ONE entry with the limit of the run's last bucket and a count of 0 (an all-empty histogram: (DBL_MAX, 0))."""
    counts = np.asarray(counts)
    keep = counts > 0
    keep[:-1] |= counts[1:] > 0      # the last bucket of a run of empty ones: its successor is not empty ...
    keep[-1] = True                  # ... or it is the last bucket
    return [float(x) for x in np.asarray(limits)[keep]], [float(c) for c in counts[keep]]


def histogram_values(plan, table, limits=None, out=print):
    """[(tag, {"min", "max", "num", "sum", "sum_squares", "bucket_limit", "bucket"})] of `plan` from a table whose row i belongs to plan[i]:
    the fields of a HistogramProto.  tf.summary.histogram fails the run on a NaN or inf; here a tag whose record counted a non-finite value
    is LEFT OUT for this step (said once per tag through `out`): a skipped fp16 step must not end the training."""
    limits = histogram_limits() if limits is None else limits
    res = []
    for i, e in enumerate(plan):
        if int(table["nonfinite"][i]) > 0:
            if e.tag not in _said_nonfinite:
                _said_nonfinite.add(e.tag)
                out("histogram %s: %d value(s) are inf or NaN -- not written for this step (said once per tag)" % (e.tag, int(table["nonfinite"][i])))
            continue
        bl, bc = compress_buckets(limits, table["counts"][i])
        h = {k: float(table[k][i]) for k in _STAT_KEYS}
        h.update(num=float(table["num"][i]), bucket_limit=bl, bucket=bc)
        res.append((e.tag, h))
    return res


# ---------------------------------------------------------------------------------------------------------------- image summaries
PreviewEntry = collections.namedtuple("PreviewEntry", "name source")
# source as in MetricEntry; name: what the tag carries (previews/<name>/image[/<k>])
PREVIEW_PANELS = ("source", "prediction", "target", "difference")      # bit k of dd_loss_previews' panel mask
IMAGE_COMBINED = ("Diffuse", "Glossy", "Subsurface", "Transmission")                          # CombinedImageFeatureTraining.initialize,
IMAGE_SINGLE = ("Volume Direct", "Volume Indirect", "Emission", "Environment")                # Training.py:475-495


def srgb_oetf(x):
    """The sRGB opto-electronic transfer function (IEC 61966-2-1) of linear values in [0, 1], float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055)


def srgb_inverse_oetf(y):
    """The inverse of srgb_oetf on [0, 1], float64."""
    y = np.asarray(y, dtype=np.float64)
    return np.where(y <= 12.92 * 0.0031308, y / 12.92, np.power((np.maximum(y, 0.0) + 0.055) / 1.055, 2.4))


def preview_thresholds():
    """The 255 fp32 thresholds of an 8-bit sRGB display value: entry k-1 is the linear value at which round(255 * OETF) steps from k-1 to k,
    the inverse OETF of (k - 0.5) / 255, k = 1 .. 255, computed in float64 and rounded to fp32 (strictly increasing in fp32).  The byte of a
    value v is the number of entries <= v: below the first is 0, at or above the last 255, so the table clamps by construction."""
    k = np.arange(1, 256, dtype=np.float64)
    return srgb_inverse_oetf((k - 0.5) / 255.0).astype(np.float32)


def image_members(arch):
    """(combined names, single pass names) the combined image sums, when the architecture defines all four combined features and the single
    passes (CombinedImageFeatureTraining.initialize, Training.py:475-495); None otherwise."""
    targets = {f.name for f in arch.feature_predictions if f.is_target}
    combined = {c for c, _ in combined_triples(arch)}
    if all(c in combined for c in IMAGE_COMBINED) and all(n in targets for n in IMAGE_SINGLE):
        return IMAGE_COMBINED, IMAGE_SINGLE
    return None


def preview_plan(arch, training_json=None, which="combined"):
    """The ordered list of PreviewEntry of an image summary.  which = "combined": the combined image (when image_members(arch) exists), then
    every combined feature; "all": these, then every predicted pass that is loaded (a generated pass has nothing to show).  "combined" on an
    architecture without combined features means "all".  The plan depends on the architecture alone: a preview shows a source whether or
    not a loss weight or a tracked statistic of `training_json` uses it."""
    if which not in ("combined", "all"):
        raise ValueError("previews: which = %r ('combined' or 'all')" % (which,))
    plan = []
    triples = combined_triples(arch)
    if image_members(arch) is not None:
        plan.append(PreviewEntry(Naming.tensorboard_name(IMAGE_NAME), ("image", IMAGE_NAME)))
    for cname, _ in triples:      # named like the statistics of a combined feature (Naming._statistics_name): "Combined <name>"
        plan.append(PreviewEntry(Naming.tensorboard_name("Combined " + cname), ("combined", cname)))
    if which == "all" or not plan:
        for f in arch.feature_predictions:
            if f.is_target and f.load_data:
                plan.append(PreviewEntry(Naming.tensorboard_name(f.name), ("feature", f.name)))
    return plan


def preview_tags(name, count):
    """TF 1.x's tf.summary.image convention: <name>/image for a single image, <name>/image/<k> for several."""
    base = "previews/%s/image" % name
    return [base] if count == 1 else ["%s/%d" % (base, k) for k in range(count)]


def preview_panel_mask(panels):
    """The panel bit mask of dd_loss_previews from names of PREVIEW_PANELS (the mosaic shows them in PREVIEW_PANELS order, whatever the
    order given)."""
    mask = 0
    for p in panels:
        if p not in PREVIEW_PANELS:
            raise ValueError("previews: unknown panel %r (one of %s)" % (p, ", ".join(PREVIEW_PANELS)))
        mask |= 1 << PREVIEW_PANELS.index(p)
    if not mask:
        raise ValueError("previews: no panel asked for")
    return mask


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
