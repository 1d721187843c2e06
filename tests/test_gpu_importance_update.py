"""-m gpu: importance scores refreshed from the model's error (csrc/dd_importance_update.hip, frame_importance.ImportanceScorer).

Op level: acc_sum / acc_count of dd_importance_update against tests/importance_update_ref.update_ref as INTEGERS.  The per-term fp32 values
are identical by construction (the same IEEE operations in the same order, no product that could contract) and the restatement adds them in
double in the kernel's documented order (lane partition, then the tree), so the double, its mean and llrint(mean 2^32) are the same.

Geometry: tiles cut by dd_sample_tiles under each of the eight (rotate, flip) draws, the sampled SOURCE tile in the prediction's place: for
every whole cell of every window acc_sum = count * llrint(ImportanceMap.cells 2^32), the map from dd_importance_cells at the same G -- equal,
because a lane walks the cell in the frame's order whatever the tile's orientation.  With an RGB permutation the three terms of a pixel are
added in another order: the mean is then within rtol = n 2^-52 of the map's (n the terms of a cell; the gate test_gpu_importance.py uses
for a double sum taken in another order), which -- llrint being monotone -- bounds the integer by llrint of the two ends of that interval.

Inside the step: a tiny f32 program on a tiny EXR tree (tiles of 32), the launch between forward and backward, eager and through the
Trainer's captured hipGraph; and `train.main --frames_importance_refresh 1` end to end."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import frames_util as U
import importance_update_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, summaries

pytestmark = pytest.mark.gpu

EPS = 1e-2
T, B = 32, 4
SIZES = [(40, 56), (33, 47)]                # scene s owns plane 2 s (a source) and 2 s + 1 (the target)
PLANE_HW = [hw for hw in SIZES for _ in range(2)]
TARGETS = [1, 3]
_CONTENT = {}


def _content(nb):
    """Two passes of nb examples, pred_ld 3 and 4: negative values, exact zeros in both at once, pixels with p = t, a 1e4 firefly per example;
    channel 3 of the wider prediction is NaN (it must not be read).  Made once per nb, never modified."""
    if nb not in _CONTENT:
        rng = np.random.default_rng(41 + nb)
        passes = []
        for ld in (3, 4):
            target = rng.standard_normal((nb, T, T, 3)).astype(np.float32)
            pred = np.full((nb, T, T, ld), np.nan, dtype=np.float32)
            q = (target + 0.5 * rng.standard_normal((nb, T, T, 3))).astype(np.float32)
            zero, same = rng.random((nb, T, T)) < 0.03, rng.random((nb, T, T)) < 0.10
            q[same] = target[same]
            q[zero], target[zero] = 0.0, 0.0
            for b in range(nb):
                q[b, rng.integers(T), rng.integers(T), rng.integers(3)] = 1e4
            pred[..., :3] = q
            passes.append((pred, target))
        _CONTENT[nb] = passes
    return _CONTENT[nb]


def _records(G):
    """Three batches of B records (source plane, target plane, y0, x0) and their (flip, rotate) draws: the eight combinations over A and B
    (rotate carries bits above the low two: only rotate & 3 counts); origins aligned to G on both axes, on one and on neither, (h - T, w - T)
    of both scenes; in B two examples over the same cells.  C: records the kernel has to clamp, and a plane that is no target plane."""
    A = [(0, 1, 0, 0), (0, 1, 8, 24), (2, 3, 1, 15), (0, 1, 0, 19)]
    Bb = [(0, 1, 0, 16), (0, 1, 3, 16), (2, 3, 0, 0), (2, 3, 1, 8)]
    Cc = [(0, 99, -5, 1000), (0, -3, 0, 0), (0, 1, 7, 5), (2, 3, 1, 15)]
    aligned = [(y0 % G == 0, x0 % G == 0) for _, _, y0, x0 in A + Bb]
    assert (True, True) in aligned and (False, False) in aligned and ((True, False) in aligned or (False, True) in aligned)
    flips = [np.array(f, dtype=np.int32) for f in ([0, 1, 0, 1], [1, 0, 1, 0], [1, 1, 0, 1])]
    rotates = [np.array(r, dtype=np.int32) for r in ([0, 1, 6, 3], [4, 5, 2, 7], [1, 2, 3, 1])]
    assert sorted((int(f), int(r) & 3) for fs, rs in zip(flips[:2], rotates[:2]) for f, r in zip(fs, rs)) == [(f, r) for f in (0, 1) for r in range(4)]
    return [np.array(x, dtype=np.int32) for x in (A, Bb, Cc)], flips, rotates


def _table(records, flips, rotates, permutes=None):
    from deepdenoiser_amd.frame_bank import RECORD_DTYPE
    table = np.zeros(len(records), dtype=RECORD_DTYPE)
    for k, key in enumerate(("source_plane", "target_plane", "y0", "x0")):
        table[key] = records[:, k]
    table["flip"], table["rotate"] = flips, rotates
    if permutes is not None:
        table["permute"] = permutes
    table["normal_rotation"] = np.eye(3, dtype=np.float32).reshape(9)
    return torch.from_numpy(table.view(np.uint8).copy()).cuda()


class _Launch:
    """One descriptor over device copies of `passes`, with fresh accumulators."""

    def __init__(self, lib, passes, cell_base, n_cells, nb):
        self.lib, self.nb = lib, nb
        self.dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()) for p, t in passes]
        self.hw = torch.tensor(PLANE_HW, dtype=torch.int32).cuda()
        self.base = torch.from_numpy(np.asarray(cell_base, dtype=np.int32)).cuda()
        d = self.desc = L.ImportanceUpdateDesc()
        d.n_passes, d.n_planes, d.plane_hw, d.cell_base, d.epsilon = len(passes), len(PLANE_HW), self.hw.data_ptr(), self.base.data_ptr(), EPS
        for en, (p, t) in zip(d.pass_, self.dev):
            en.pred, en.pred_ld, en.target, en.target_ld = p.data_ptr(), int(p.shape[-1]), t.data_ptr(), int(t.shape[-1])
        self.acc_sum = torch.zeros(n_cells, dtype=torch.int64, device="cuda")
        self.acc_count = torch.zeros(n_cells, dtype=torch.int32, device="cuda")

    def run(self, table, G, use_flip, use_rotate):
        L.check(self.lib.dd_importance_update(ctypes.byref(self.desc), table.data_ptr(), self.nb, T, G, use_flip, use_rotate, self.acc_sum.data_ptr(),
                                              self.acc_count.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return self.acc_sum.cpu().numpy().view(np.uint64).copy(), self.acc_count.cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("G", [8, 16])      # 64 pixels: one per lane; 256: four per lane
def test_update_matches_numpy_as_integers(lib, G):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    passes = _content(B)
    cell_base, n_cells = R.cell_bases(SIZES, TARGETS, len(PLANE_HW), G)
    batches, flips, rotates = _records(G)
    for name, k, use_flip, use_rotate in (("A", 0, 1, 1), ("B", 1, 1, 1), ("B, switches off", 1, 0, 0), ("B, flip only", 1, 1, 0), ("C", 2, 1, 1)):
        want_sum, want_count, visited = R.update_ref(passes, batches[k], flips[k], rotates[k], PLANE_HW, cell_base, n_cells, T, G, use_flip, use_rotate, EPS)
        launch = _Launch(lib, passes, cell_base, n_cells, B)
        table = _table(batches[k], flips[k], rotates[k])
        have_sum, have_count = launch.run(table, G, use_flip, use_rotate)
        print("G=%d %s: %d of %d cells visited, counts up to %d" % (G, name, int((want_count > 0).sum()), n_cells, int(want_count.max())))
        assert (have_count == want_count).all(), (name, np.nonzero(have_count != want_count)[0][:8].tolist())
        bad = np.nonzero(have_sum != want_sum)[0]
        assert bad.size == 0, (name, bad[:8].tolist(), have_sum[bad[:4]].tolist(), want_sum[bad[:4]].tolist())
        # cells a window covers in part, and cells no window touches, stay 0
        assert 0 < (want_count > 0).sum() < n_cells and (have_sum[want_count == 0] == 0).all()
        if k == 0:      # (8, 24) in a 40 x 56 plane at G = 16: one whole cell per axis, the partly covered ones around it get nothing
            assert len(R.whole_cells(8, 24, T, 16)) == 1 and len(R.whole_cells(0, 0, T, G)) == (T // G) ** 2
        if k == 1:      # two examples over the same cells
            assert want_count.max() == 2
        if k == 2:      # plane 99 -> the last plane, origin (-5, 1000) -> (0, w - T); plane -3 -> plane 0, which is no target plane
            assert sorted(set(b for b, _ in visited)) == [0, 2, 3]
        # a second launch doubles both tables
        again_sum, again_count = launch.run(table, G, use_flip, use_rotate)
        assert (again_sum == 2 * want_sum).all() and (again_count == 2 * want_count).all()


@pytest.mark.parametrize("G", [8, 16])
def test_nonfinite_cells_and_planes_without_cells(lib, G):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    passes = _content(B)
    cell_base, n_cells = R.cell_bases(SIZES, TARGETS, len(PLANE_HW), G)
    batches, flips, rotates = _records(G)
    records, fl, ro = batches[0], flips[0], rotates[0]
    clean_sum, clean_count, visited = R.update_ref(passes, records, fl, ro, PLANE_HW, cell_base, n_cells, T, G, 1, 1, EPS)
    # a NaN in one cell of example 0 (pass 0) and an inf in one cell of example 2 (pass 1), each in a cell visited once
    once = [(b, c) for b, c in visited if clean_count[c] == 1]
    (b_nan, c_nan), (b_inf, c_inf) = next(v for v in once if v[0] == 0), next(v for v in reversed(once) if v[0] == 2)
    planted = [(p.copy(), t) for p, t in passes]
    for (b, cell, p, value) in ((b_nan, c_nan, 0, np.nan), (b_inf, c_inf, 1, np.inf)):
        tp = int(records[b, 1])
        h, w = PLANE_HW[tp]
        cy, cx = divmod(cell - int(cell_base[tp]), w // G)
        k, flip = int(ro[b]) & 3, int(fl[b]) > 0
        ty, tx = R.tile_index(T, k, flip)
        fy, fx = cy * G - int(records[b, 2]) + G // 2, cx * G - int(records[b, 3]) + 1      # a pixel inside the cell, in window coordinates
        planted[p][0][b, ty[fy, fx], tx[fy, fx], 1] = value
    want_sum, want_count = clean_sum.copy(), clean_count.copy()
    want_sum[[c_nan, c_inf]], want_count[[c_nan, c_inf]] = 0, 0
    ref_sum, ref_count, _ = R.update_ref(planted, records, fl, ro, PLANE_HW, cell_base, n_cells, T, G, 1, 1, EPS)
    assert (ref_sum == want_sum).all() and (ref_count == want_count).all()      # the restatement agrees on what a planted value does
    have_sum, have_count = _Launch(lib, planted, cell_base, n_cells, B).run(_table(records, fl, ro), G, 1, 1)
    assert have_sum[c_nan] == 0 and have_count[c_nan] == 0 and have_sum[c_inf] == 0 and have_count[c_inf] == 0
    assert (have_sum == want_sum).all() and (have_count == want_count).all()      # every other cell as without the planted values
    # a plane with cell_base = -1 adds nothing: the second scene's cells stay 0, the first scene's are what they were
    off = cell_base.copy()
    off[TARGETS[1]] = -1
    have_sum, have_count = _Launch(lib, passes, off, n_cells, B).run(_table(records, fl, ro), G, 1, 1)
    first = int(cell_base[TARGETS[1]])
    assert (clean_count[first:] > 0).any()
    assert (have_sum[first:] == 0).all() and (have_count[first:] == 0).all()
    assert (have_sum[:first] == clean_sum[:first]).all() and (have_count[:first] == clean_count[:first]).all()


# ---------------------------------------------------------------------------------------------------- geometry, against the existing kernels
class _Scene:
    def __init__(self, h, w):
        self.height, self.width = h, w


class _SyntheticBank:
    """What ImportanceMap reads of a FrameBank: one source per scene, two colour passes that are both a source and a target."""

    def __init__(self):
        rng = np.random.default_rng(17)
        self.tile, self.S, self.scenes, self.device = T, 1, [_Scene(h, w) for h, w in SIZES], torch.device("cuda")
        self.n_planes = len(PLANE_HW)
        self.source_channels = self.target_channels = {"a": 3, "b": 3}
        self.host = {}
        for name in ("a", "b"):
            planes = []
            for (h, w) in SIZES:
                target = np.abs(rng.standard_normal((h, w, 3))).astype(np.float32)
                source = np.abs(target + rng.standard_normal((h, w, 3)).astype(np.float32) * rng.random((h, w, 1)).astype(np.float32))
                source[rng.random((h, w)) < 0.1] = 0.0
                planes += [source.astype(np.float32), target]
            self.host[name] = planes
        self.planes = {n: [torch.from_numpy(p).cuda() for p in ps] for n, ps in self.host.items()}
        self.pointers = {n: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).cuda() for n, ts in self.planes.items()}
        self.plane_hw = torch.tensor(PLANE_HW, dtype=torch.int32).cuda()

    def source_plane(self, s, k):
        return 2 * s + k

    def target_plane(self, s):
        return 2 * s + 1


@pytest.mark.parametrize("G", [8, 16])
def test_geometry_against_the_sampler_and_the_noise_map(lib, G):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.frame_importance import ImportanceMap
    bank = _SyntheticBank()
    imap = ImportanceMap(bank, cell=G)
    assert imap.passes == ["a", "b"]
    want_cells = np.concatenate([c.reshape(-1) for c in imap.cells])
    cell_base, n_cells = R.cell_bases(SIZES, TARGETS, len(PLANE_HW), G)
    assert n_cells == len(want_cells) and (want_cells > 0).all()
    nb = 8
    records = np.array([(0, 1, 0, 0), (0, 1, 8, 24), (2, 3, 1, 15), (0, 1, 0, 19), (0, 1, 5, 16), (2, 3, 0, 0), (2, 3, 1, 8), (0, 1, 3, 11)], dtype=np.int32)
    flips, rotates = (np.arange(nb) // 4).astype(np.int32), (np.arange(nb) % 4).astype(np.int32)
    count = np.zeros(n_cells, dtype=np.int64)
    for (_, tp, y0, x0) in records.tolist():
        for cy, cx in R.whole_cells(y0, x0, T, G):
            count[int(cell_base[tp]) + cy * (PLANE_HW[tp][1] // G) + cx] += 1
    assert count.max() >= 2 and (count > 0).sum() > n_cells // 2
    n_terms = G * G * 3 * 2
    for permutes in (None, (1 + np.arange(nb) % 5).astype(np.int32)):
        # the sampler cuts the source tiles into the prediction blocks (leading dimensions 3 and 4) and the target tiles into the targets
        preds = [torch.full((nb, T, T, ld), float("nan"), dtype=torch.float32, device="cuda") for ld in (3, 4)]
        targets = [torch.zeros((nb, T, T, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
        sd = L.TileSamplerDesc()
        sd.n_passes, sd.n_planes, sd.plane_hw = 4, bank.n_planes, bank.plane_hw.data_ptr()
        jobs = [("a", preds[0], 0), ("b", preds[1], 0), ("a", targets[0], 1), ("b", targets[1], 1)]
        for en, (name, dst, from_target) in zip(sd.pass_, jobs):
            en.planes, en.dst, en.C, en.kind, en.ld_dst, en.from_target = bank.pointers[name].data_ptr(), dst.data_ptr(), 3, L.AUG_RGB, int(dst.shape[-1]), from_target
        table = _table(records, flips, rotates, permutes)
        stream = torch.cuda.current_stream().cuda_stream
        L.check(lib.dd_sample_tiles(ctypes.byref(sd), table.data_ptr(), nb, T, 1, 1, int(permutes is not None), 0, stream))
        d = L.ImportanceUpdateDesc()
        base_dev = torch.from_numpy(cell_base).cuda()
        d.n_passes, d.n_planes, d.plane_hw, d.cell_base, d.epsilon = 2, bank.n_planes, bank.plane_hw.data_ptr(), base_dev.data_ptr(), EPS
        for en, p, t in zip(d.pass_, preds, targets):
            en.pred, en.pred_ld, en.target, en.target_ld = p.data_ptr(), int(p.shape[-1]), t.data_ptr(), 3
        acc_sum = torch.zeros(n_cells, dtype=torch.int64, device="cuda")
        acc_count = torch.zeros(n_cells, dtype=torch.int32, device="cuda")
        L.check(lib.dd_importance_update(ctypes.byref(d), table.data_ptr(), nb, T, G, 1, 1, acc_sum.data_ptr(), acc_count.data_ptr(), stream))
        torch.cuda.synchronize()
        have_sum, have_count = acc_sum.cpu().numpy(), acc_count.cpu().numpy().astype(np.int64)
        assert (have_count == count).all()
        if permutes is None:
            want = np.rint(want_cells * 4294967296.0).astype(np.int64) * count
            bad = np.nonzero(have_sum != want)[0]
            assert bad.size == 0, (bad[:8].tolist(), have_sum[bad[:4]].tolist(), want[bad[:4]].tolist())
        else:
            rtol = n_terms * 2.0 ** -52
            lo = np.rint(want_cells * (1.0 - rtol) * 4294967296.0).astype(np.int64) * count
            hi = np.rint(want_cells * (1.0 + rtol) * 4294967296.0).astype(np.int64) * count
            seen = count > 0
            err = np.abs(have_sum[seen] / count[seen] / 4294967296.0 - want_cells[seen]) / want_cells[seen]
            print("G=%d, permuted channels: worst relative error of a mean %.3e (n 2^-52 = %.3e; one unit of 2^-32 is %.3e of the smallest mean)"
                  % (G, err.max(), rtol, 2.0 ** -32 / want_cells[seen].min()))
            assert ((lo <= have_sum) & (have_sum <= hi)).all(), np.nonzero((have_sum < lo) | (have_sum > hi))[0][:8].tolist()


# ---------------------------------------------------------------------------------------------------- inside the step, and end to end
G2, SPP, BEST, B2 = 16, 4, 16, 2
SCENES = (("scene_a", 48, 72), ("scene_b", 40, 40))


def _architecture_json():
    """The tiny kernel-predicting network of test_gpu_tile_sampler.py: its predictions are convex combinations of source pixels, so they are
    finite on random frames from the first step on (a direct-prediction head of an untrained network overflows expm1 on such data, and a
    cell whose mean is not finite is -- rightly -- not scored)."""
    return configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE",
                                combined={"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
                                          "Alpha": {"Color": "Alpha", "Direct": "", "Indirect": ""}})


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from deepdenoiser_amd.architecture import Architecture
    root = str(tmp_path_factory.mktemp("importance_refresh"))
    aj = _architecture_json()
    aj["model_directory"] = "model"
    arch = Architecture(aj, device="cpu")
    source = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    target = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    rng = np.random.default_rng(9)
    for name, h, w in SCENES:
        U.write_scene(root, name, [SPP], list(source), target, h, w, rng, sources=2, target_spp=BEST)
    frames_json = U.write_json(root, {"training": [n for n, _, _ in SCENES]}, T, [SPP], 2, list(source), target)
    tj = configs.training(learning_rate=1e-3, batch_size=B2, image_mean=0.0)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "no_such_directory", "modes": ["training"],
               "number_of_source_index_tuples": 2})
    json.dump(aj, open(os.path.join(root, "architecture.json"), "w"))
    json.dump(tj, open(os.path.join(root, "training.json"), "w"))
    return {"root": root, "aj": aj, "tj": tj, "frames_json": frames_json, "flip": "Normal" not in source,
            "colour": sorted(n for n in target if source.get(n) == 3)}


def test_scoring_launch_inside_the_step(dataset):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.data_augmentation import DataAugmentation, DataAugmentationUsage
    from deepdenoiser_amd.frame_bank import FrameBank, FrameSet, TileSampler
    from deepdenoiser_amd.frame_importance import ImportanceMap, ImportanceScorer
    from deepdenoiser_amd.training import Trainer
    arch = Architecture(dataset["aj"], device="cuda", dtype="f32", seed=2)
    trainer = Trainer(arch, dataset["tj"], B2, T, T, use_graph=True)
    prog = trainer.program
    assert prog.step_tail_ops == []                             # without a scorer attached
    bank = FrameBank(arch, FrameSet.from_json(dataset["frames_json"], "training", log=lambda m: None), SPP, "cuda", threads=2, log=lambda m: None)
    usage = DataAugmentationUsage(True, dataset["flip"], True, True)
    sampler = TileSampler(prog, bank, usage)
    imap = ImportanceMap(bank, cell=G2)
    sampler.set_importance(imap)
    scorer = ImportanceScorer(prog, sampler, imap)
    assert len(prog.step_tail_ops) == 1 and scorer.passes == dataset["colour"] == imap.passes
    hw = [bank.hw[p] for p in range(bank.n_planes)]
    cell_base, n_cells = R.cell_bases([(h, w) for _, h, w in SCENES], [bank.target_plane(s) for s in range(2)], bank.n_planes, G2)
    assert n_cells == scorer.n_cells == 3 * 4 + 2 * 2 and (scorer.cell_base.cpu().numpy() == cell_base).all()
    gen = torch.Generator().manual_seed(3)
    batches = [np.array(r, dtype=np.int32) for r in ([(0, 2, 16, 32), (4, 5, 3, 8)], [(1, 2, 5, 40), (3, 5, 0, 0)], [(0, 2, 0, 7), (1, 2, 16, 16)],
                                                     [(3, 5, 8, 8), (0, 2, 11, 29)], [(4, 5, 8, 0), (1, 2, 0, 40)], [(0, 2, 16, 40), (3, 5, 1, 2)])]

    def expected_count(records):
        out = np.zeros(n_cells, dtype=np.int64)
        for (_, tp, y0, x0) in records.tolist():
            for cy, cx in R.whole_cells(y0, x0, T, G2):
                out[int(cell_base[tp]) + cy * (hw[tp][1] // G2) + cx] += 1
        return out

    # forward() plus an explicit run of the tail ops, against the restatement on copies of predictions[0] and targets[0]
    draws = DataAugmentation.draw(B2, gen)
    draws["rotate"], draws["flip"] = np.array([1, 2], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    sampler.sample(batches[0], draws)
    prog.zero_grads()
    prog.forward()
    torch.cuda.synchronize()
    assert int(scorer.acc_count.sum()) == 0                     # forward() scores nothing
    prog.run_step_tail()
    torch.cuda.synchronize()
    P, targets = prog.predictions[0].buf.cpu().numpy(), prog.targets[0].cpu().numpy()
    index = {f.name: i for i, f in enumerate(prog.head)}
    passes = [(P[index[n] * B2:(index[n] + 1) * B2], targets[index[n] * B2:(index[n] + 1) * B2]) for n in scorer.passes]
    want_sum, want_count, _ = R.update_ref(passes, batches[0], draws["flip"], draws["rotate"], hw, cell_base, n_cells, T, G2,
                                           int(usage.use_flip_left_right), int(usage.use_rotate_90), EPS)
    have_sum, have_count = scorer.tables()
    for n, (p, t) in zip(scorer.passes, passes):
        print("%s: prediction %s ld %d, %d values not finite, |p| up to %.3g; target %d not finite" % (n, p.shape, p.shape[-1], int((~np.isfinite(p[..., :3])).sum()),
                                                                                                  float(np.nanmax(np.abs(p[..., :3]))), int((~np.isfinite(t)).sum())))
    print("counts: kernel %s\n        numpy  %s\n        records %s" % (have_count.tolist(), want_count.tolist(), expected_count(batches[0]).tolist()))
    assert (want_count == expected_count(batches[0])).all() and want_count.sum() > 0
    assert (have_count == want_count).all() and (have_sum == want_sum).all()
    sums, counts = scorer.collect()
    assert (sums == want_sum).all() and (counts == want_count).all() and int(scorer.acc_count.sum()) == 0 and int(scorer.acc_sum.sum()) == 0
    # five steps of the Trainer: eager twice, then captured and replayed; acc_count is what the records alone predict
    total = np.zeros(n_cells, dtype=np.int64)
    for step in range(5):
        records = batches[1 + step]
        sampler.sample(records, DataAugmentation.draw(B2, gen))
        loss = trainer.step()
        total += expected_count(records)
        assert (scorer.tables()[1] == total).all(), step
        assert np.isfinite(float(loss))
        before = scorer.tables()
        prog.forward()                                          # a forward in between (summaries, validation) changes nothing
        after = scorer.tables()
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    assert trainer._graphs is not None and total.max() >= 2
    with pytest.raises(RuntimeError, match="after the trainer had built its segments"):
        prog.add_step_tail_op(lambda stream: None)
    # the fold of what the five steps left
    sums, counts = scorer.collect()
    assert imap.fold(sums, counts, 0.5) == int((total > 0).sum())


def test_train_cli_with_refreshed_importance(dataset, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd import train
    root = dataset["root"]
    pngs = os.path.join(root, "pngs")
    common = [os.path.join(root, "training.json"), "--frames", dataset["frames_json"], "--frames_crops", "importance",
              "--frames_importance_png", pngs, "--train_epochs", "1", "--dtype", "f32", "--summary_steps", "0", "--threads", "2"]
    pattern = (r"frames: importance refresh at step (\d+) -- (\d+) cells folded \(([\d.]+) % of 16\), mean model error ([\d.]+), "
               r"the heaviest tenth of the windows holds ([\d.]+) % of the weight")
    # without the flag: no such line, and the pictures of the noise map
    train.main(train.parser().parse_args(common))
    out = capsys.readouterr().out
    assert re.search(r"epoch 1: global_step 3, ", out) is not None, out      # (1 * 2 + 1 * 1) tiles * 2 index tuples / 2
    assert "importance refresh" not in out
    assert sorted(os.listdir(pngs)) == ["scene_a_importance.png", "scene_b_importance.png"]
    noise = [open(os.path.join(pngs, n), "rb").read() for n in sorted(os.listdir(pngs))]
    for n in os.listdir(pngs):
        os.remove(os.path.join(pngs, n))
    # with it: a line per step with cells folded, and the pictures rewritten from the refreshed map
    train.main(train.parser().parse_args(common + ["--frames_importance_refresh", "1", "--frames_importance_rate", "1.0"]))
    out = capsys.readouterr().out
    lines = re.findall(pattern, out)
    assert [int(l[0]) for l in lines] == [4, 5, 6], out                # (resumed from the first run's checkpoint at step 3)
    for step, folded, share, error, tenth in lines:
        assert 1 <= int(folded) <= 16 and abs(float(share) - 100.0 * int(folded) / 16) < 0.06 and 0.0 < float(error) <= 1.0
    assert re.search(r"epoch 1: global_step 6, loss ([-+.\deinfa]+) ", out) is not None, out      # (resumed from the first run's checkpoint)
    assert re.search(r"frames: importance crops -- cells of 16, 7 lattice windows, passes Diffuse Color, Diffuse Direct, Diffuse Indirect, floor 0.25, ", out)
    assert sorted(os.listdir(pngs)) == ["scene_a_importance.png", "scene_b_importance.png"]
    refreshed = [open(os.path.join(pngs, n), "rb").read() for n in sorted(os.listdir(pngs))]
    shapes = [summaries.decode_png(b).shape for b in refreshed]
    assert shapes == [(2, 3), (1, 1)] and refreshed != noise
