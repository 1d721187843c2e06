"""The descriptors of the loss and tracking launches (dd_loss_desc / dd_loss_msssim_desc, include/dd_hip.h), filled in ONE place.

Host only: ctypes structures are filled and buffers allocated, nothing is launched.  The loss build (program.py) and the tracked metrics,
histograms and image summaries (tracking.py) all name the sources of a scale through fill_sources; which sources exist is decided by
metrics.combined_levels / metrics.combined_triples, which pass defines a mask by metrics.mask_pass.  loss_plan decides what the loss of a
training program evaluates before the program records anything."""
import os
import types

import torch

from . import _lib as L
from . import metrics as M
from .render_passes import RenderPasses

LOSS_KIND = {"DIFFERENCE": 1, "ABSOLUTE": 2, "SMOOTH_ABSOLUTE": 3, "SQUARED": 4, "SMAPE": 5}
EPSILON = 1e-2      # the epsilon of the SMAPE form (LossDifference.py:18-34)


def check_ms_ssim(head, dim, q_feat):
    """Build-time rules of the ms_ssim term (BaseFeatureTraining.ms_ssim, Training.py:178-204) on tiles of dim = (h, w)."""
    h, w = dim
    if h % 4 or w % 4 or min(h, w) < 44:
        raise ValueError("the ms_ssim loss term needs tiles whose height and width are multiples of 4 and at least 44 (got %d x %d): "
                         "tf.image.ssim_multiscale refuses a level smaller than its 11 x 11 filter (3 levels: side / 4 >= 11), and "
                         "levels of odd size would need its symmetric pad before the 2x2 pool, which is not built" % (h, w))
    if q_feat > 0:
        for f in head:
            if f.load_data and f.number_of_channels != 3:
                raise ValueError("a features-level ms_ssim weight cannot be used with the loaded 1-channel target pass '%s': the reference "
                                 "transposes such a tensor into an image 1 pixel high (Training.py:187-190) and cannot build either" % f.name)


def loss_plan(arch, head, training_json, dims):
    """What the loss of a training program evaluates, decided before anything is recorded (Training.model_fn, Training.py:607-660): the weights
    of the three levels, which sources exist, how many scales carry a loss, and whether dd_loss_head runs the inverse standardization of those
    scales itself (fuse_invert).  dims: (h, w) of every scale.  Raises what the reference raises for settings it cannot build."""
    tj = training_json

    def w3(j):      # (mean, variation, ms_ssim) weights of one level (BaseFeatureTraining.loss, Training.py:210-243)
        return float(j["mean"]), float(j["variation"]), float(j["ms_ssim"])

    def wm(j):      # masked-mean weight of one level (Training.py:131-137, 233-241)
        if j and j["ms_ssim"] > 0:
            raise NotImplementedError("the masked ms_ssim loss term cannot run: the reference raises 'Not implemented' there too "
                                      "(BaseFeatureTraining.masked_ms_ssim, Training.py:206-207)")
        if j and j["variation"] > 0:
            raise NotImplementedError("the masked variation loss term is out of scope (weight 0 in TrainingExample.json)")
        return float(j["mean"]) if j else 0.0
    fs, cf, ci = tj["features_training_settings"], tj["combined_features_training_settings"], tj["combined_image_training_settings"]
    p = types.SimpleNamespace()
    p.masked_features, p.masked_combined = wm(fs.get("loss_weights_masked")), wm(cf.get("loss_weights_masked"))
    p.features, p.combined, p.image = w3(fs["loss_weights"]), w3(cf["loss_weights"]), w3(ci["loss_weights"])
    p.use_image, p.use_comb = M.combined_levels(tj)      # Training.py:1063-1093
    p.triples = M.combined_triples(arch) if p.use_comb else []
    p.loss_scales = len(dims) if tj["use_multiscale_loss"] else 1
    p.norm = 1.0 / sum(1.0 / 4.0 ** s for s in range(p.loss_scales))
    # (decided by the sources that exist, not by the weights alone: a combined-features weight on a network without a complete triple
    # evaluates nothing and must not cost the fused launch)
    p.ms_ssim = (p.features[2] > 0 and any(f.load_data for f in head)) or (p.combined[2] > 0 and len(p.triples) > 0) or p.image[2] > 0
    if p.ms_ssim:
        check_ms_ssim(head, dims[0], p.features[2])
    # A loss without variation terms (every term a function of one pixel) behind an inverse standardization that feeds nothing else: the
    # inversion and its gradient run inside dd_loss_head (one launch per scale instead of three; DD_FUSE_LOSS_INVERT=0 keeps them apart)
    # (an ms_ssim term rules the fusion out like a variation term does: the fused launch leaves dL/d(standardized value) in dpred, and
    # dd_loss_msssim_bwd adds a gradient with respect to the inverted value)
    p.fuse_invert = (arch.invert_standardization_after_multiscale_predictions and p.features[1] == 0 and p.combined[1] == 0 and p.image[1] == 0
                     and not p.ms_ssim and os.environ.get("DD_FUSE_LOSS_INVERT", "1") != "0")
    if p.masked_features > 0 and any(f.load_data and f.name == "Alpha" for f in head):
        raise Exception("Masking is not supported for the alpha pass, because it does not seem to make sense.")   # Training.py:103-113
    return p


def block_ptr(t, image_offset):
    """Pointer to image `image_offset` of head tensor t (fp32)."""
    return t.ptr + image_offset * t.H * t.W * t.ld * 4


def set_kind(d, training_json):
    d.kind, d.epsilon = LOSS_KIND[training_json["loss_difference"]], EPSILON


def fill_sources(d, program, s, triples, use_image):
    """The sources of scale s: prediction, target and channel count of every head feature (a loaded pass: its block of predictions[s]; a
    generated pass: its echo), the combined index triples, and the members of the combined image."""
    B = program.B
    h, w = program.dims[s]
    P = program.predictions[s]
    d.n_features = program.NF
    for i, f in enumerate(program.head):
        d.target[i], d.target_ld[i], d.nch[i] = program.targets[s].data_ptr() + i * B * h * w * 3 * 4, 3, f.number_of_channels
        d.pred[i] = block_ptr(P, i * B) if f.load_data else program.echo[(f.name, s)].data_ptr()
        d.pred_ld[i] = P.ld if f.load_data else 3
    d.n_combined = len(triples)
    for k, (_, names) in enumerate(triples):
        for c in range(3):
            d.comb[k][c] = program.head_index[names[c]]
    d.n_image_combined = d.n_image_features = 0
    if use_image:      # CombinedImageFeatureTraining.initialize, Training.py:475-495
        cidx = {c: k for k, (c, _) in enumerate(triples)}
        for n in M.IMAGE_COMBINED:
            d.image_combined[d.n_image_combined] = cidx[n]
            d.n_image_combined += 1
        for n in M.IMAGE_SINGLE:
            d.image_features[d.n_image_features] = program.head_index[n]
            d.n_image_features += 1


def sources_desc(program, s, triples, use_image):
    """A LossDesc with the loss difference of the program's Training.json and the sources of scale s."""
    d = L.LossDesc()
    set_kind(d, program.training_json)
    fill_sources(d, program, s, triples, use_image)
    return d


def fill_mask_features(d, head, head_index, triples, features_masked, combined_masked, missing_ok=False):
    """mask_feature of every loaded pass that has a colour pass (FeatureTraining.initialize, Training.py:379-392) when `features_masked`,
    comb_mask_feature of every triple (CombinedFeatureTraining.initialize, Training.py:434-437) when `combined_masked`; -1 otherwise.
    missing_ok: a colour pass the network does not predict gives -1 instead of a KeyError."""
    def index(name):
        return head_index.get(name, -1) if missing_ok else head_index[name]
    for i, f in enumerate(head):
        cp = M.mask_pass(f.name) if (features_masked and f.load_data) else None
        d.mask_feature[i] = index(cp) if cp is not None else -1
    for k, (cname, _) in enumerate(triples):
        d.comb_mask_feature[k] = index(RenderPasses.combined_to_color_render_pass(cname)) if combined_masked else -1


def ms_ssim_desc(d, feature_weight, combined_weight, image_weight, dpred=None):
    """The MsSsimDesc over the sources of LossDesc `d`.  feature_weight / combined_weight: one weight per head feature / combined triple,
    image_weight: the combined image's (a positive weight selects the source); dpred: one gradient pointer (or None) per head feature,
    None for a launch without a backward.  Returns (descriptor, number of selected sources)."""
    m = L.MsSsimDesc()
    m.n_features, m.n_combined = d.n_features, d.n_combined
    m.n_image_combined, m.n_image_features = d.n_image_combined, d.n_image_features
    for i in range(d.n_features):
        m.pred[i], m.target[i], m.pred_ld[i], m.target_ld[i], m.nch[i] = d.pred[i], d.target[i], d.pred_ld[i], d.target_ld[i], d.nch[i]
        m.dpred[i] = dpred[i] if dpred is not None else None
        m.ssim_weight[i] = feature_weight[i]
    for k in range(d.n_combined):
        for c in range(3):
            m.comb[k][c] = d.comb[k][c]
        m.comb_ssim_weight[k] = combined_weight[k]
    for k in range(d.n_image_combined):
        m.image_combined[k] = d.image_combined[k]
    for k in range(d.n_image_features):
        m.image_features[k] = d.image_features[k]
    m.image_ssim_weight = image_weight
    n_sources = sum(wt > 0 for wt in list(feature_weight[:d.n_features]) + list(combined_weight[:d.n_combined]) + [image_weight])
    return m, n_sources


def slot_table(head, triples):
    """source -> row of the per-source tables of dd_loss_metrics / dd_loss_histograms / dd_loss_previews (include/dd_hip.h)."""
    slot_of = {("feature", f.name): i for i, f in enumerate(head)}
    slot_of.update({("combined", c): L.MAX_FEATURES + k for k, (c, _) in enumerate(triples)})
    slot_of[("image", M.IMAGE_NAME)] = L.MAX_FEATURES + L.MAX_COMBINED
    return slot_of


def device_scratch(nbytes, dtype, device):
    """Zeroed scratch of `nbytes` as a library *_scratch_bytes call reports them; a negative answer is the library's error."""
    if nbytes < 0:
        L.check(int(nbytes))
    return torch.zeros(nbytes // dtype.itemsize, dtype=dtype, device=device)
