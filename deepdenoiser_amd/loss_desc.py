"""The descriptors of the loss and tracking launches (dd_loss_desc / dd_loss_msssim_desc, include/dd_hip.h), filled in ONE place.

Host only: ctypes structures are filled and buffers allocated, nothing is launched.  The loss build (program.py) and the tracked metrics,
histograms and image summaries (tracking.py) all name the sources of a scale through fill_sources; which sources exist is decided by
metrics.combined_levels / metrics.combined_triples, which pass defines a mask by metrics.mask_pass."""
import torch

from . import _lib as L
from . import metrics as M
from .render_passes import RenderPasses

LOSS_KIND = {"DIFFERENCE": 1, "ABSOLUTE": 2, "SMOOTH_ABSOLUTE": 3, "SQUARED": 4, "SMAPE": 5}
EPSILON = 1e-2      # the epsilon of the SMAPE form (LossDifference.py:18-34)


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
