"""-m gpu: the tracked metrics on the device -- dd_loss_metrics / dd_loss_msssim_values (csrc/dd_metrics.hip, csrc/dd_loss_msssim.hip) against
tests/golden/metrics_golden.* (the reference's own evaluation branch, executed), Program.metrics() against the loss the same forward
computed, and the training command line's event files.

Gates: every metric of an fp32 table against the float64 reference at gpu_util.ACC32["f32"] (5e-6 relative: fp32 terms, fp32 sums in a fixed
tree); ms_ssim values at the 1e-4 of test_gpu_msssim.test_op_parity; sum of weight * metric against program.loss_buf at the 2e-5 step-1 loss
gate of tests/test_gpu_model.py.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_util as U
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, summaries, tf_checkpoint, tfrecords
from deepdenoiser_amd import metrics as M
from deepdenoiser_amd.naming import Naming
from deepdenoiser_amd.render_passes import RenderPasses
from gpu_util import ACC32, gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"DIFFERENCE": 1, "ABSOLUTE": 2, "SMOOTH_ABSOLUTE": 3, "SQUARED": 4, "SMAPE": 5}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_table(d, B, h, w):
    lib = L.load()
    nbytes = lib.dd_loss_metrics_scratch_bytes(B, h, w)
    assert nbytes > 0
    scratch = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")      # (every partial that is read must have been written)
    table = torch.full((L.METRIC_SOURCES * B * 4,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.dd_loss_metrics(C.byref(d), B, h, w, scratch.data_ptr(), table.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return table


class _CaseOp:
    """Device tensors + descriptors of one fixture case.  Feature 1 keeps its prediction with a pixel stride of 4; a 1-channel pass (Alpha)
    keeps its prediction in channel 0 of a 3-float pixel and its target with a pixel stride of 1."""

    def __init__(self, c):
        self.c, self.keep = c, []

    def desc(self, s, masked=True):
        c = self.c
        h, w = c.dims[s]
        tg = c.targets(s)
        d = L.LossDesc()
        d.n_features = len(c.head)
        d.kind, d.epsilon = KIND[c.tj["loss_difference"]], 1e-2
        for i, f in enumerate(c.head):
            nch = f.number_of_channels
            ld = 4 if i == 1 else 3
            p = torch.full((c.B, h, w, ld), 7.0, dtype=torch.float32, device="cuda")
            p[..., :nch] = c.preds[s][f.name].cuda()
            t = tg[f.name].float().cuda().contiguous()
            self.keep += [p, t]
            d.pred[i], d.pred_ld[i], d.target[i], d.target_ld[i], d.nch[i] = p.data_ptr(), ld, t.data_ptr(), nch, nch
            cp = M.mask_pass(f.name)
            d.mask_feature[i] = c.index[cp] if (masked and cp is not None) else -1
        d.n_combined = len(c.triples)
        for k, (cname, names) in enumerate(c.triples):
            for j in range(3):
                d.comb[k][j] = c.index[names[j]]
            d.comb_mask_feature[k] = c.index[RenderPasses.combined_to_color_render_pass(cname)] if masked else -1
        if c.use_image:
            cidx = {cn: k for k, (cn, _) in enumerate(c.triples)}
            for n in ("Diffuse", "Glossy", "Subsurface", "Transmission"):
                d.image_combined[d.n_image_combined] = cidx[n]
                d.n_image_combined += 1
            for n in ("Volume Direct", "Volume Indirect", "Emission", "Environment"):
                d.image_features[d.n_image_features] = c.index[n]
                d.n_image_features += 1
        return d

    def ms_values(self):
        c = self.c
        ms_sources = [e.source for e in c.plan if e.quantity == "ms_ssim"]
        if not ms_sources:
            return None
        h, w = c.dims[0]
        ld = self.desc(0)
        m = L.MsSsimDesc()
        m.n_features, m.n_combined = ld.n_features, ld.n_combined
        for i, f in enumerate(c.head):
            m.pred[i], m.target[i], m.pred_ld[i], m.target_ld[i], m.nch[i] = ld.pred[i], ld.target[i], ld.pred_ld[i], ld.target_ld[i], ld.nch[i]
            m.ssim_weight[i] = 1.0 if ("feature", f.name) in ms_sources else 0.0
        for k, (cname, _) in enumerate(c.triples):
            for j in range(3):
                m.comb[k][j] = ld.comb[k][j]
            m.comb_ssim_weight[k] = 1.0 if ("combined", cname) in ms_sources else 0.0
        order = [("feature", f.name) for f in c.head if ("feature", f.name) in ms_sources] + \
                [("combined", cn) for cn, _ in c.triples if ("combined", cn) in ms_sources]
        lib = L.load()
        nbytes = lib.dd_loss_msssim_scratch_bytes(c.B, h, w, len(order))
        assert nbytes > 0
        scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        out = torch.full((len(order) * c.B,), float("nan"), dtype=torch.float32, device="cuda")
        L.check(lib.dd_loss_msssim_values(C.byref(m), c.B, h, w, scratch.data_ptr(), out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        return out, {src: out[j * c.B:(j + 1) * c.B].cpu().numpy() for j, src in enumerate(order)}


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("case", U.CASES)
def test_op_against_the_reference(case):
    """5 + 6: every metric of every fixture case from the device table, all scales; two runs give the same bits."""
    _need_gpu()
    c = U.Case(case)
    op = _CaseOp(c)
    tables, again = {}, {}
    for s in c.scales:
        h, w = c.dims[s]
        d = op.desc(s)
        tables[s] = _run_table(d, c.B, h, w)
        again[s] = _run_table(d, c.B, h, w)
        assert torch.isfinite(tables[s]).all()
        assert torch.equal(tables[s], again[s]), "scale %d: two runs differ" % s
    ms = op.ms_values()
    if ms is not None:
        assert torch.equal(ms[0], op.ms_values()[0])
    host = {s: t.cpu().numpy().reshape(L.METRIC_SOURCES, c.B, 4) for s, t in tables.items()}
    got = M.metric_values(c.plan, c.slot_of, host, c.dims, None, ms[1] if ms is not None else None)
    worst = {"table": 0.0, "ms_ssim": 0.0}
    for e, g, w in zip(c.plan, got, c.values):
        err = abs(g - w) / abs(w)
        key = "ms_ssim" if e.quantity == "ms_ssim" else "table"
        worst[key] = max(worst[key], err)
        print("%-48s %.9g (reference %.9g) rel %.2e" % (e.name, g, w, err))
    gate("%s: worst metric from the table" % case, worst["table"], ACC32["f32"])
    if ms is not None:
        gate("%s: worst ms_ssim metric" % case, worst["ms_ssim"], 1e-4)
    # mask sums are counts: exact
    for s in c.scales:
        assert np.array_equal(host[s][:, :, 3], c.table(s)[:, :, 3])
    # rows of sources the descriptor does not have are zeros
    used = set(c.slot_of[src] for src in c.sources(0))
    for slot in range(L.METRIC_SOURCES):
        if slot not in used:
            assert not host[c.scales[0]][slot].any()


def test_op_odd_shape_against_numpy():
    """B = 3, 20 x 12 (not a multiple of the 16 x 4 tile: clipped tiles, scalar staging), pixel stride 4 everywhere, every loss kind."""
    _need_gpu()
    B, H, W = 3, 20, 12
    g = torch.Generator().manual_seed(11)
    n = 4
    pred = [torch.randn(B, H, W, 3, generator=g).abs() * torch.exp(0.5 * torch.randn(B, H, W, 1, generator=g)) for _ in range(n)]
    tgt = [torch.randn(B, H, W, 3, generator=g).abs() * (torch.rand(B, H, W, 1, generator=g) > 0.3) for _ in range(n)]
    keep = []
    for kind_name, kind in sorted(KIND.items()):
        if kind_name == "DIFFERENCE":
            continue      # (a signed sum cancels: no relative gate applies)
        d = L.LossDesc()
        d.n_features, d.kind, d.epsilon = n, kind, 1e-2
        for f in range(n):
            p, t = torch.zeros(B, H, W, 4, device="cuda"), torch.zeros(B, H, W, 4, device="cuda")
            p[..., :3], t[..., :3] = pred[f].cuda(), tgt[f].cuda()
            keep += [p, t]
            d.pred[f], d.pred_ld[f], d.target[f], d.target_ld[f], d.nch[f], d.mask_feature[f] = p.data_ptr(), 4, t.data_ptr(), 4, 3, (0 if f < 3 else -1)
        d.n_combined = 1
        d.comb[0][0], d.comb[0][1], d.comb[0][2], d.comb_mask_feature[0] = 0, 1, 2, 0
        d.n_image_combined, d.n_image_features = 1, 1
        d.image_combined[0], d.image_features[0] = 0, 3
        got = _run_table(d, B, H, W).cpu().numpy().reshape(L.METRIC_SOURCES, B, 4).astype(np.float64)
        from oracle import tf_ops as T
        P, Y = [p.double() for p in pred], [t.double() for t in tgt]
        mask0 = torch.sign(Y[0].abs().sum(dim=3))
        comb = (P[0] * (P[1] + P[2]), Y[0] * (Y[1] + Y[2]))
        srcs = {f: (P[f], Y[f], mask0 if f < 3 else None) for f in range(n)}
        srcs[L.MAX_FEATURES] = (comb[0], comb[1], mask0)
        srcs[L.MAX_FEATURES + L.MAX_COMBINED] = (comb[0] + P[3], comb[1] + Y[3], None)
        worst = 0.0
        for slot, (p, y, m) in srcs.items():
            dd = T.loss_difference(p, y, kind_name)
            var = (T.loss_difference(p[:, :, 1:] - p[:, :, :-1], y[:, :, 1:] - y[:, :, :-1], kind_name).sum(dim=(1, 2))
                   + T.loss_difference(p[:, 1:] - p[:, :-1], y[:, 1:] - y[:, :-1], kind_name).sum(dim=(1, 2)))
            want = torch.stack([dd.sum(dim=(1, 2)), var, (dd * m).sum(dim=(1, 2)) if m is not None else torch.zeros(B, dtype=torch.float64),
                                m.sum(dim=(1, 2)) if m is not None else torch.zeros(B, dtype=torch.float64)], dim=1).numpy()
            assert np.array_equal(got[slot][:, 3], want[:, 3])
            nz = want != 0
            assert not got[slot][~nz].any()
            worst = max(worst, float(np.max(np.abs(got[slot][nz] - want[nz]) / np.abs(want[nz]))))
        gate("odd shape %s: worst table entry" % kind_name, worst, ACC32["f32"])


def test_bad_descriptors_are_refused():
    _need_gpu()
    c = U.Case("alpha_unmasked")
    op = _CaseOp(c)
    lib = L.load()
    d = op.desc(0)
    d.comb[0][1] = 99
    buf = torch.zeros(L.METRIC_SOURCES * c.B * 4, device="cuda")
    scratch = torch.zeros(lib.dd_loss_metrics_scratch_bytes(c.B, c.H, c.W) // 4, device="cuda")
    assert lib.dd_loss_metrics(C.byref(d), c.B, c.H, c.W, scratch.data_ptr(), buf.data_ptr(), _stream()) != 0
    assert b"comb[0][1]" in lib.dd_last_error()
    d = op.desc(0)
    d.mask_feature[0] = d.n_features
    assert lib.dd_loss_metrics(C.byref(d), c.B, c.H, c.W, scratch.data_ptr(), buf.data_ptr(), _stream()) != 0
    assert lib.dd_loss_metrics_scratch_bytes(0, 4, 4) < 0


# ---------------------------------------------------------------------------------------------------------------- whole program
NO_ALPHA = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
LEVELS = ("features_training_settings", "combined_features_training_settings", "combined_image_training_settings")


def _all_terms_training():
    """every supported loss term with the matching track_* flag"""
    tj = configs.training(feature_variation=0.5, masked_mean=0.25, combined_variation=0.25, image_variation=0.125, combined_masked_mean=0.5,
                          ms_ssim=(0.6, 2.0, 4.0))
    for lv in LEVELS:
        tj[lv]["statistics"].update(track_mean=True, track_variation=True, track_ms_ssim=True)
    for lv in LEVELS[:2]:
        tj[lv]["statistics_masked"].update(track_mean=True)
    return tj


def _program_inputs(arch, B, H, W, seed=0):
    """smooth labels in [0.1, 1], sources = label + noise (an untrained kernel-predicting network returns a blurred source: no ms_ssim factor
    is clamped); one corner of every pass is exactly zero, so that the masks are neither empty nor full"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    hole = torch.ones(1, H, W, 1)
    hole[:, :12, :12] = 0.0

    def smooth(ch):
        grid = torch.rand(B, ch, 8, 8, generator=g)
        return (0.1 + 0.9 * F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)).permute(0, 2, 3, 1).contiguous()
    feats, labels = {}, {}
    for f in arch.feature_predictions:
        ch = f.number_of_channels
        if f.load_data:
            t = smooth(ch) * hole
            v = (t + 0.05 * torch.randn(B, H, W, ch, generator=g)) * hole
        else:
            t = torch.full((B, H, W, ch), 1.0 if f.feature_prediction_type == "COLOR" else 0.5)
            v = t.clone()
        labels[Naming.target_feature_name(f.name)] = t.cuda()
        feats[Naming.source_feature_name(f.name, index=0)] = v.cuda()
    for f in arch.auxiliary_features:
        feats[Naming.source_feature_name(f.name, index=0)] = (smooth(f.number_of_channels) + 0.05 * torch.randn(B, H, W, f.number_of_channels, generator=g)).cuda()
    return feats, labels


def _weighted_sum(tj, plan, values, n_scales):
    """BaseFeatureTraining.loss (Training.py:210-243) from the tracked metrics: sum over sources and scales of weight * scale factor * metric,
    plus weight * ms_ssim once per source."""
    scales = n_scales if tj["use_multiscale_loss"] else 1
    norm = 1.0 / sum(1.0 / 4.0 ** s for s in range(scales))
    level = {"feature": LEVELS[0], "combined": LEVELS[1], "image": LEVELS[2]}
    total = 0.0
    for e, v in zip(plan, values):
        lv = tj[level[e.source[0]]]
        if e.quantity == "ms_ssim":
            total += lv["loss_weights"]["ms_ssim"] * v
            continue
        if e.scale_index >= scales:
            continue
        w = {"mean": lv["loss_weights"]["mean"], "variation_mean": lv["loss_weights"]["variation"],
             "masked_mean": lv.get("loss_weights_masked", {}).get("mean", 0.0)}[e.quantity]
        total += w * norm / 4.0 ** e.scale_index * v
    return total


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_program_metrics_add_up_to_the_loss(dtype):
    """7: the new kernel against the loss kernels of the same forward, and Program.metrics() against the op-level call on its predictions."""
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    B, H, W = 2, 48, 48
    aj, tj = configs.architecture(filters=(16, 16, 16), convs=1, flag_mode="NONE", combined=NO_ALPHA), _all_terms_training()
    arch = Architecture(aj, device="cuda", dtype=dtype)
    prog = arch.program(B, H, W, training_json=tj)
    n_fwd = len(prog.g.fwd_ops)
    feats, labels = _program_inputs(arch, B, H, W)
    prog.set_inputs(feats, labels)
    prog.zero_grads()
    prog.forward()
    loss = float(prog.loss_buf)
    values = prog.metrics()
    torch.cuda.synchronize()
    plan = prog.metric_plan()
    assert len(prog.g.fwd_ops) == n_fwd, "metrics() must not add to the forward program"
    assert [e.name for e in plan] == [e.name for e in M.metric_plan(arch, tj)]
    quantities = {(e.source[0], e.quantity) for e in plan}
    assert quantities == {(a, b) for a in ("feature", "combined", "image") for b in ("mean", "variation_mean", "ms_ssim")} | \
        {("feature", "masked_mean"), ("combined", "masked_mean")}
    by = dict(zip([e.name for e in plan], values))
    assert by["diffuse_color_mean_masked/1"] != by["diffuse_color_mean/1"]
    total = _weighted_sum(tj, plan, values, arch.number_of_scales())
    print("%s: loss_buf %.8f, sum of weighted metrics %.8f (%d metrics)" % (dtype, loss, total, len(plan)))
    gate("%s: weighted metrics against loss_buf" % dtype, abs(total - loss) / abs(loss), 2e-5)
    # metrics() == the op-level call on prediction_dictionaries(), to the bit
    table = prog.metric_table().clone()
    st = prog.tracking_metrics
    preds = prog.prediction_dictionaries()
    head = [f for f in arch.feature_predictions if f.is_target]
    index = {f.name: i for i, f in enumerate(head)}
    triples = M.combined_triples(arch)
    for j, s in enumerate(st.scales):
        h, w = H >> s, W >> s
        d = L.LossDesc()
        d.n_features, d.kind, d.epsilon = len(head), KIND[tj["loss_difference"]], 1e-2
        keep = []
        for i, f in enumerate(head):
            p = preds[s][Naming.feature_prediction_name(f.name)].contiguous().clone()
            t = prog.targets[s][i * B:(i + 1) * B].contiguous().clone()
            keep += [p, t]
            d.pred[i], d.pred_ld[i], d.target[i], d.target_ld[i], d.nch[i] = p.data_ptr(), p.shape[3], t.data_ptr(), 3, f.number_of_channels
            cp = M.mask_pass(f.name)
            d.mask_feature[i] = index[cp] if cp is not None else -1
        d.n_combined = len(triples)
        for k, (cname, names) in enumerate(triples):
            for q in range(3):
                d.comb[k][q] = index[names[q]]
            d.comb_mask_feature[k] = index[RenderPasses.combined_to_color_render_pass(cname)]
        cidx = {cn: k for k, (cn, _) in enumerate(triples)}
        for nme in ("Diffuse", "Glossy", "Subsurface", "Transmission"):
            d.image_combined[d.n_image_combined] = cidx[nme]
            d.n_image_combined += 1
        for nme in ("Volume Direct", "Volume Indirect", "Emission", "Environment"):
            d.image_features[d.n_image_features] = index[nme]
            d.n_image_features += 1
        got = _run_table(d, B, h, w)
        assert torch.equal(got, table[j * st.rows:(j + 1) * st.rows]), "scale %d" % s
    # rows summed over the images (what the ranks of a data-parallel run all-reduce), with their count
    nt = len(st.scales) * st.rows
    sums = torch.cat([table[:nt].double().reshape(-1, B, 4).sum(dim=1).reshape(-1), table[nt:].double().reshape(-1, B).sum(dim=1)])
    for a, b in zip(prog.metric_values(sums.cpu().numpy(), count=B), values):
        assert abs(a - b) <= 1e-12 * abs(b)
    # real < B: the first image alone
    one = prog.metric_values(table, real=1)
    assert one != values and len(one) == len(values)


CHILD_STEP = r"""
import sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from deepdenoiser_amd.architecture import Architecture
import test_gpu_metrics as TM
B, H, W = 2, 48, 48
aj, tj = TM.configs.architecture(filters=(16, 16, 16), convs=1, flag_mode="NONE", combined=TM.NO_ALPHA), TM._all_terms_training()
out = []
for with_metrics in (False, True):
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    prog = arch.program(B, H, W, training_json=tj)
    feats, labels = TM._program_inputs(arch, B, H, W)
    prog.set_inputs(feats, labels)
    if with_metrics:
        prog.zero_grads(); prog.forward(); values = prog.metrics()
        assert len(values) > 0
    loss = prog.train_step().clone()
    torch.cuda.synchronize()
    out.append((loss, arch.params.grads.clone(), arch.params.values.clone()))
same = [int(torch.equal(a, b)) for a, b in zip(out[0], out[1])]
print("RESULT loss=%%d grads=%%d values=%%d nonzero=%%d" %% (same[0], same[1], same[2], int((out[0][1] != 0).sum())))
"""


def test_metrics_leave_the_step_alone():
    """8: loss, gradients and updated weights of train_step() are bit-identical with and without a forward() + metrics() before it
    (DD_DETERMINISTIC=1 in a child process: the plain step's atomics are not ordered)."""
    _need_gpu()
    env = dict(os.environ, DD_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, "-c", CHILD_STEP % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0]
    r = dict(kv.split("=") for kv in line.split()[1:])
    assert r["loss"] == "1" and r["grads"] == "1" and r["values"] == "1", line
    assert int(r["nonzero"]) > 1000


def test_captured_step_replays_after_metrics():
    """8: a Trainer whose step has been captured replays it correctly after a forward() + metrics() in between.  Two trainers from the same
    seed run the same four steps (two eager, capture, replay), one of them with the metric launches before the replayed step: the plain
    step's fp32 atomics are unordered, so the losses are compared at the 2e-5 of the step-1 loss gate rather than to the bit."""
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.training import Trainer
    B, H, W = 2, 48, 48
    aj, tj = configs.architecture(filters=(16, 16, 16), convs=1, flag_mode="NONE", combined=NO_ALPHA), _all_terms_training()
    losses = []
    for with_metrics in (False, True):
        arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
        trainer = Trainer(arch, tj, B, H, W)
        feats, labels = _program_inputs(arch, B, H, W)
        trainer.program.set_inputs(feats, labels)
        run = []
        for k in range(4):
            if with_metrics and k == 3:
                assert trainer._graphs is not None
                trainer.program.zero_grads()
                trainer.program.forward()
                before = trainer.program.metrics()
            run.append(float(trainer.step()))
        torch.cuda.synchronize()
        losses.append(run)
        if with_metrics:      # the metrics were those of the step's own forward: same weights, same inputs
            total = _weighted_sum(tj, trainer.program.metric_plan(), before, arch.number_of_scales())
            gate("metrics before the replayed step against its loss", abs(total - run[3]) / abs(run[3]), 2e-5)
    print("losses without / with metrics:", losses)
    assert losses[0][3] != losses[0][0]      # (the steps do change the weights)
    for a, b in zip(*losses):
        gate("captured step after metrics", abs(a - b) / abs(a), 2e-5)


# ---------------------------------------------------------------------------------------------------------------- command line
T_, SPP = 32, 16


def _write_dataset(base, arch, mode, n_files, per_file, seed):
    """(the miniature data set of tests/test_gpu_end_to_end.py, for any mode) tiles of smooth radiance: sources = target * (1 + noise)"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(base, mode))
    json.dump({"tiles_height_width": T_, "number_of_sources_per_example": 1, "source_samples_per_pixel_list": [SPP]},
              open(os.path.join(base, mode + ".json"), "w"))
    passes = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    targets = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    yy, xx = np.meshgrid(np.linspace(0, 1, T_, dtype=np.float32), np.linspace(0, 1, T_, dtype=np.float32), indexing="ij")
    for n in range(n_files):
        records = []
        for _ in range(per_file):
            feats, clean = {}, {}
            for name, ch in passes.items():
                a, b, c = rng.random(3).astype(np.float32)
                img = np.stack([(a + b * yy + c * xx) * (0.5 + 0.5 * k / max(ch, 1)) for k in range(ch)], axis=-1).astype(np.float32)
                clean[name] = img
                noisy = img * (1.0 + 0.3 * rng.standard_normal(img.shape).astype(np.float32))
                feats[Naming.source_feature_name(name, samples_per_pixel=SPP, index=0)] = noisy.astype(np.float32).tobytes()
            for name in targets:
                feats[Naming.target_feature_name(name)] = clean[name].tobytes()
            records.append(tfrecords.serialize_example(feats))
        tfrecords.write_records(os.path.join(base, mode, "%s_%d.tfrecords.gz" % (mode, n)), records)


def test_cli_writes_event_files(tmp_path):
    """9: two epochs with validation and --summary_steps 1 in one child process."""
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", combined=NO_ALPHA)
    aj["model_directory"] = "model"
    tj = configs.training(learning_rate=2e-3, batch_size=4)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "data", "modes": ["training", "validation"], "number_of_source_index_tuples": 1})
    tj["data_augmentation"] = {"use_rotate_90": True, "use_flip_left_right": False, "use_rgb_permutation": True, "use_normal_rotation": False}
    for lv in LEVELS:
        tj[lv]["statistics"].update(track_mean=True, track_variation=True)
    for lv in LEVELS[:2]:
        tj[lv]["statistics_masked"].update(track_mean=True)
    tj["features_training_settings"]["statistics"]["track_difference_histogram"] = True      # said once, not written
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    json.dump(tj, open(tmp_path / "training.json", "w"))
    arch = Architecture(aj, device="cpu")
    base = str(tmp_path / "data")
    _write_dataset(base, arch, "training", 2, 4, 0)
    _write_dataset(base, arch, "validation", 1, 6, 1)      # 6 examples in batches of 4: the last one is padded with 2 repeats
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "deepdenoiser_amd.train", str(tmp_path / "training.json"), "--train_epochs", "2", "--dtype", "f32",
                        "--summary_steps", "1"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = p.stdout
    # the old lines are still there
    assert "epoch 1: global_step 2" in out and "epoch 2: global_step 4" in out, out
    assert "epoch 2: validation loss " in out and " over 6 batches" in out, out
    assert out.count("histograms are not written") == 1
    model = str(tmp_path / "model")
    assert tf_checkpoint.latest_checkpoint(model) is not None and tf_checkpoint.latest_checkpoint(model).endswith("-4")
    names = [e.name for e in M.metric_plan(arch, tj, out=lambda *a: None)]
    assert len(names) > 100
    # training summaries: loss, learning_rate, batch_size and every tracked scalar at steps 1 .. 4
    (train_file,) = summaries.event_files(model)
    scalars = summaries.read_scalars(train_file)
    assert sorted({s for s, _, _ in scalars}) == [1, 2, 3, 4]
    for step in (1, 2, 3, 4):
        assert [t for s, t, _ in scalars if s == step] == ["loss", "learning_rate", "batch_size"] + names
    at = {(s, t): v for s, t, v in scalars}
    assert at[(1, "batch_size")] == 4.0 and abs(at[(3, "learning_rate")] - 2e-3) < 1e-9
    assert all(np.isfinite(v) for v in at.values())

    def printed(marker):
        line = [ln for ln in out.splitlines() if marker in ln][0]
        return float(line.split("loss ")[1].split()[0].rstrip(","))
    # the epoch line prints the loss of the epoch's last step with 5 decimals (the only sampled step of a 2-step epoch); the event stores an
    # fp32: half a unit of the last printed digit + the fp32 rounding of a loss of this size
    for epoch, step in ((1, 2), (2, 4)):
        want = printed("epoch %d: global_step %d" % (epoch, step))
        assert abs(at[(step, "loss")] - want) <= 0.5e-5 + 2.0 ** -23 * abs(want), (step, at[(step, "loss")], want)
    # evaluation summaries: eval_validation/, one event file of the run, one event per validation pass at the global step of the pass
    (eval_file,) = summaries.event_files(os.path.join(model, "eval_validation"))
    sc_all = summaries.read_scalars(eval_file)
    seen = []
    for step in sorted({s for s, _, _ in sc_all}):
        sc = [x for x in sc_all if x[0] == step]
        assert [t for _, t, _ in sc] == ["loss"] + names
        seen.append((step, dict((t, v) for _, t, v in sc)))
    assert sorted(s for s, _ in seen) == [2, 4]
    for step, values in seen:
        want = printed("epoch %d: validation loss" % (step // 2))
        assert abs(values["loss"] - want) <= 0.5e-5 + 2.0 ** -23 * abs(want)
        line = [ln for ln in out.splitlines() if ln.startswith("epoch %d: validation diffuse_color_mean/1 " % (step // 2))][0]
        assert abs(float(line.split()[-1]) - values["diffuse_color_mean/1"]) <= 1e-5 * abs(values["diffuse_color_mean/1"])
    # the weighted metrics of the validation set add up to its loss (mean weights only in this configuration)
    for step, values in seen:
        norm = 1.0 / sum(1.0 / 4.0 ** s for s in range(arch.number_of_scales()))
        total = 0.0
        for e in M.metric_plan(arch, tj, out=lambda *a: None):
            if e.quantity == "mean":
                w = tj[{"feature": LEVELS[0], "combined": LEVELS[1], "image": LEVELS[2]}[e.source[0]]]["loss_weights"]["mean"]
                total += w * norm / 4.0 ** e.scale_index * values[e.name]
        gate("validation: weighted metrics against the loss at step %d" % step, abs(total - values["loss"]) / abs(values["loss"]), 2e-5)
