"""-m gpu: importance scores of resident frames (csrc/dd_frame_importance.hip, deepdenoiser_amd/frame_importance.py).

Op level: every cell of dd_importance_cells against tests/importance_ref.cell_sums_ref at rtol = n * 2^-52, n the number of terms of the cell
(at most 16 * 16 * 3 * 2 * 2 = 3072).  The per-term fp32 values are identical by construction (the same IEEE operations in the same order, no
product that could contract); what differs is the order of the double sum, and a sum of n non-negative doubles in any order is within
n * 2^-53 of the exact sum, relative -- once for the kernel, once for numpy.

End to end: a tiny EXR tree (24 x 40 and 16 x 16, tiles of 8, cells of 4) whose source colour passes equal the target except in one quadrant
of scene_a: the map's cell means, where the draws land, and `train.main --frames_crops importance`."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import frames_util as U
import importance_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, openexr, summaries

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- op level
SIZES = [(40, 56), (33, 47), (64, 64)]      # as test_gpu_tile_sampler.py: a row pitch (47 * 12 bytes) that is no multiple of 16 bytes
SOURCES = 2
SENTINEL = -7.5
EPS = 1e-2
ABSENT = ("b", 3)                           # pass b is not loaded in plane 3 (scene 1, source 0)
_PLANES = {}


def _planes():
    """{pass: [9 host planes]}: scene s owns planes 3 s + 0, 1 (sources) and 3 s + 2 (target).  Made once, never modified.  Negative values;
    exact zeros in source and target at once; pixels where a source equals the target; a few 1e4 fireflies in the sources."""
    if not _PLANES:
        rng = np.random.default_rng(29)
        for name in ("a", "b"):
            planes = []
            for (h, w) in SIZES:
                target = rng.standard_normal((h, w, 3)).astype(np.float32)
                zero = rng.random((h, w)) < 0.03
                target[zero] = 0.0
                sources = []
                for _ in range(SOURCES):
                    s = (target + rng.standard_normal((h, w, 3)).astype(np.float32)).astype(np.float32)
                    same = rng.random((h, w)) < 0.10
                    s[same] = target[same]
                    s[zero] = 0.0
                    fire = rng.random((h, w)) < 0.004
                    s[fire] = 1e4
                    sources.append(s)
                planes += sources + [target]
            _PLANES[name] = planes
        _PLANES[ABSENT[0]][ABSENT[1]] = None
    return _PLANES


def _cells(G):
    """Every full cell of every scene, row-major, plus the last origin (h - G, w - G) where the grid does not hold it."""
    out = []
    for s, (h, w) in enumerate(SIZES):
        out += [(3 * s, 3 * s + SOURCES, cy * G, cx * G) for cy in range(h // G) for cx in range(w // G)]
        if h % G or w % G:
            out.append((3 * s, 3 * s + SOURCES, h - G, w - G))
    return np.array(out, dtype=np.int32).reshape(-1, 4)


@pytest.mark.parametrize("G", [4, 16])      # 16 pixels: fewer than lanes; 256 pixels: four per lane
def test_cells_match_numpy_and_repeat(lib, G):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    planes, cells = _planes(), _cells(G)
    assert ((cells[:, 2] % G != 0) | (cells[:, 3] % G != 0)).sum() == (2 if G == 16 else 1)
    for (sp0, tp, y0, x0) in cells.tolist():      # all entries in range
        h, w = SIZES[tp // 3]
        assert 0 <= y0 <= h - G and 0 <= x0 <= w - G and sp0 + SOURCES == tp
    dev = {n: [None if p is None else torch.from_numpy(p).cuda() for p in ps] for n, ps in planes.items()}
    ptrs = {n: torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64).cuda() for n, ts in dev.items()}
    hw = torch.tensor([hw for hw in SIZES for _ in range(SOURCES + 1)], dtype=torch.int32).cuda()
    desc = L.ImportanceDesc()
    desc.n_passes, desc.n_planes, desc.plane_hw, desc.n_sources, desc.epsilon = 2, len(SIZES) * (SOURCES + 1), hw.data_ptr(), SOURCES, EPS
    for en, name in zip(desc.pass_, ("a", "b")):
        en.planes = ptrs[name].data_ptr()
    table = torch.from_numpy(np.ascontiguousarray(cells)).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((len(cells),), SENTINEL, dtype=torch.float64, device="cuda")
        L.check(lib.dd_importance_cells(ctypes.byref(desc), table.data_ptr(), len(cells), G, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()               # repeatability: two launches, the same bytes
    have = outs[0]
    assert (have != SENTINEL).all()                            # every entry is written
    want, terms = R.cell_sums_ref([planes["a"], planes["b"]], cells, G, SOURCES, EPS)
    assert terms.max() == G * G * 3 * 2 * SOURCES and terms.min() == G * G * 3 * (2 * SOURCES - 1)      # the absent plane drops one pair
    assert (want > 0).all()
    err = np.abs(have - want) / want
    gate = terms * 2.0 ** -52
    print("G=%d: %d cells, %d .. %d terms; worst relative error %.3e (gate %.3e .. %.3e), worst error / gate %.3f"
          % (G, len(cells), terms.min(), terms.max(), err.max(), gate.min(), gate.max(), (err / gate).max()))
    assert (err <= gate).all(), (int(np.argmax(err / gate)), float((err / gate).max()))


# ---------------------------------------------------------------------------------------------------- end to end
T2, G2, SPP, BEST, B2 = 8, 4, 4, 16, 16
SCENES = (("scene_a", 24, 40), ("scene_b", 16, 16))
QUADRANT = (slice(12, 24), slice(20, 40))                      # of scene_a: the sources are noisy here and equal the target elsewhere


def _architecture_json():
    return configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", kernel_prediction=False, multiscale=False,
                                combined={"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
                                          "Alpha": {"Color": "Alpha", "Direct": "", "Indirect": ""}})


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from deepdenoiser_amd.architecture import Architecture
    root = str(tmp_path_factory.mktemp("importance_e2e"))
    aj = _architecture_json()
    aj["model_directory"] = "model"
    arch = Architecture(aj, device="cpu")
    source = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    target = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    colour = sorted(n for n in target if source.get(n) == 3)
    assert colour == ["Diffuse Color", "Diffuse Direct", "Diffuse Indirect"]
    rng = np.random.default_rng(5)
    written = {}
    for name, h, w in SCENES:
        written[name] = U.write_scene(root, name, [SPP], list(source), target, h, w, rng, sources=2, target_spp=BEST)
        for index in range(2):
            for p in colour:
                img = written[name][(BEST, 0)][p].copy()
                if name == "scene_a":
                    img[QUADRANT] = np.abs(img[QUADRANT] + 3.0 * rng.standard_normal(img[QUADRANT].shape).astype(np.float32))
                openexr.write_image(os.path.join(root, "OpenEXR", name, U.rendering_name(name, SPP, index), "render_%s_0001.exr" % p), img)
                written[name][(SPP, index)][p] = img
    frames_json = U.write_json(root, {"training": [n for n, _, _ in SCENES]}, T2, [SPP], 2, list(source), target)
    tj = configs.training(learning_rate=1e-3, batch_size=B2, image_mean=0.0)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "no_such_directory", "modes": ["training"],
               "number_of_source_index_tuples": 2})
    json.dump(aj, open(os.path.join(root, "architecture.json"), "w"))
    json.dump(tj, open(os.path.join(root, "training.json"), "w"))
    # the reference's cell means, computed once
    planes = [[written[name][key][p] for name, _, _ in SCENES for key in ((SPP, 0), (SPP, 1), (BEST, 0))] for p in colour]
    means = []
    for s, (name, h, w) in enumerate(SCENES):
        cells = np.array([(3 * s, 3 * s + 2, cy * G2, cx * G2) for cy in range(h // G2) for cx in range(w // G2)], dtype=np.int32)
        sums, terms = R.cell_sums_ref(planes, cells, G2, 2, 1e-2)
        assert (terms == G2 * G2 * 3 * len(colour) * 2).all()
        means.append((sums / (G2 * G2 * 3 * len(colour) * 2)).reshape(h // G2, w // G2))
    return {"root": root, "aj": aj, "tj": tj, "frames_json": frames_json, "colour": colour, "means": means, "terms": G2 * G2 * 3 * len(colour) * 2}


@pytest.fixture(scope="module")
def resident(dataset):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.frame_bank import FrameBank, FrameSet
    from deepdenoiser_amd.frame_importance import ImportanceMap
    arch = Architecture(dataset["aj"], device="cuda", dtype="f32", seed=2)
    bank = FrameBank(arch, FrameSet.from_json(dataset["frames_json"], "training", log=lambda m: None), SPP, "cuda", threads=2, log=lambda m: None)
    return bank, ImportanceMap(bank, cell=G2)


def _noisy(s, y0, x0):
    return s == 0 and y0 + T2 > QUADRANT[0].start and x0 + T2 > QUADRANT[1].start


def test_map_matches_the_reference_cell_means(dataset, resident):
    bank, imap = resident
    assert imap.passes == dataset["colour"] and imap.cell == G2 and imap.floor == 0.25
    worst = 0.0
    for have, want in zip(imap.cells, dataset["means"]):
        assert have.shape == want.shape and have.dtype == np.float64
        assert (have[want == 0] == 0).all()
        nz = want != 0
        if nz.any():
            worst = max(worst, float((np.abs(have[nz] - want[nz]) / want[nz]).max()))
    print("cell means: worst relative error %.3e (gate %.3e)" % (worst, dataset["terms"] * 2.0 ** -52))
    assert worst <= dataset["terms"] * 2.0 ** -52
    a, b = imap.cells
    assert (b == 0).all() and (a[:3] == 0).all() and (a[:, :5] == 0).all() and (a[3:, 5:] > 0.1).all() and a.max() <= 1.0


def test_draws_land_where_the_noise_is(dataset, resident):
    from deepdenoiser_amd.frame_bank import TileRecords
    from deepdenoiser_amd.frame_importance import ImportanceMap
    bank, imap = resident
    tuples = [[0], [1]]
    greedy = ImportanceMap.from_cells(bank, imap.cells, cell=G2, floor=0.0)
    rng = random.Random(3)
    for _ in range(200):
        s, y0, x0, tup = greedy.draw(rng, tuples)
        assert _noisy(s, y0, x0), (s, y0, x0)
    rng = random.Random(4)
    drawn = [imap.draw(rng, tuples)[:3] for _ in range(2000)]
    in_b = sum(1 for s, _, _ in drawn if s == 1)
    noisy = sum(1 for s, y0, x0 in drawn if _noisy(s, y0, x0))
    lattice = [(s, i * G2, j * G2) for s, W in enumerate(imap.weights) for i in range(W.shape[0]) for j in range(W.shape[1])]
    share = sum(1 for w in lattice if _noisy(*w)) / len(lattice)
    print("2000 draws: %d in scene_b (expected 250), %d in the noisy windows (%.3f of the lattice)" % (in_b, noisy, share))
    assert len(lattice) == 45 + 9 and in_b >= 1 and noisy / 2000.0 > share
    rec = TileRecords(bank, 4)
    rec.set_importance(imap)
    rec.validate(rec.draw(random.Random(5), "importance", tuples))


def test_train_cli_with_importance_crops(dataset, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd import train
    root = dataset["root"]
    pngs = os.path.join(root, "pngs")
    args = train.parser().parse_args([os.path.join(root, "training.json"), "--frames", dataset["frames_json"], "--frames_crops", "importance",
                                      "--frames_importance_cell", str(G2), "--frames_importance_png", pngs,
                                      "--train_epochs", "1", "--dtype", "f32", "--summary_steps", "0", "--threads", "2"])
    train.main(args)
    out = capsys.readouterr().out
    m = re.search(r"epoch 1: global_step (\d+), loss ([-+.\deinfa]+) ", out)
    assert m is not None, out
    assert int(m.group(1)) == (3 * 5 + 2 * 2) * 2 // B2 == 2 and np.isfinite(float(m.group(2))), out
    line = re.search(r"frames: importance crops -- cells of 4, 54 lattice windows, passes Diffuse Color, Diffuse Direct, Diffuse Indirect, "
                     r"floor 0.25, the heaviest tenth of the windows holds ([\d.]+) % of the weight", out)
    assert line is not None and float(line.group(1)) > 10.0, out
    assert sorted(os.listdir(pngs)) == ["scene_a_importance.png", "scene_b_importance.png"]
    a = summaries.decode_png(open(os.path.join(pngs, "scene_a_importance.png"), "rb").read())
    b = summaries.decode_png(open(os.path.join(pngs, "scene_b_importance.png"), "rb").read())
    assert a.shape == (5, 9) and b.shape == (3, 3) and a.max() == 255 and (b == 0).all()
    i, j = np.unravel_index(int(np.argmax(a)), a.shape)
    assert i * G2 >= QUADRANT[0].start and j * G2 >= QUADRANT[1].start, (i, j)
