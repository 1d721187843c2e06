"""-m gpu: training tiles cut from frames kept on the device (csrc/dd_tile_sampler.hip, deepdenoiser_amd/frame_bank.py).

Op level: dd_sample_tiles against tests/sampler_ref.py (a numpy crop, then the oracle's augmentation of one example) -- bit-equal for every
pass whose augmentation moves data or flips signs, atol 2e-6 for the world-space normal's 3x3 rotation (the gate tests/test_augment.py sets
for this arithmetic).  End to end: the frames path fills the program's buffers with exactly the bytes the .tfrecords path does, and
`train.main --frames` trains an epoch and writes its checkpoint."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import frames_util as U
import sampler_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, tf_checkpoint, tfrecords
from deepdenoiser_amd.data_augmentation import DataAugmentation, DataAugmentationUsage
from deepdenoiser_amd.naming import Naming

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- op level
B = 24
SIZES = [(40, 56), (33, 47), (64, 64)]      # odd sizes: scenes differ, and a row pitch (47 * 12, 33 * 4 bytes) that is no multiple of 16 bytes
SOURCES = 2
SENTINEL = -7.5
SOURCE_PASSES = {"Diffuse Color": 3, "Depth": 1, "Screen Space Normal": 3, "Motion Vector": 3, "Normal": 3}
TARGET_PASSES = {"Diffuse Color": 3, "Alpha": 1}
_PLANES = {}


def _planes():
    """{pass: [9 host planes]}: scene s owns planes 3 s + 0, 1 (sources) and 3 s + 2 (target).  Made once, never modified."""
    if not _PLANES:
        rng = np.random.default_rng(11)
        for name, ch in {**SOURCE_PASSES, **TARGET_PASSES}.items():
            _PLANES[name] = [rng.standard_normal((h, w, ch)).astype(np.float32) for (h, w) in SIZES for _ in range(SOURCES + 1)]
    return _PLANES


def _records(T):
    """Every scene and both source indices occur; origins (0, 0), (h-T, w-T) and odd x0 among them."""
    rng = random.Random(T)
    rec = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        s, index = b % 3, (b // 3) % SOURCES
        h, w = SIZES[s]
        y0, x0 = rng.randint(0, h - T), rng.randint(0, w - T)
        if b < 3:
            y0, x0 = 0, 0
        elif b < 6:
            y0, x0 = h - T, w - T
        elif b % 2:
            x0 = rng.choice(range(1, w - T + 1, 2))
        rec[b] = (3 * s + index, 3 * s + SOURCES, y0, x0)
    assert (rec[:, 3] % 2 == 1).any()
    return rec


@pytest.mark.parametrize("mode", ["flip_off", "flip_on", "crop"])
@pytest.mark.parametrize("T", [20, 32])      # 20: no multiple of the 32-pixel staging block (one partial block); 32: exactly one
def test_sample_tiles_matches_reference(lib, T, mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.frame_bank import RECORD_DTYPE
    planes = _planes()
    flip_on = mode == "flip_on"
    usage = DataAugmentationUsage(True, flip_on, True, True) if mode != "crop" else DataAugmentationUsage(False, False, False, False)
    g = torch.Generator().manual_seed(5)
    draws = DataAugmentation.draw(B, generator=g)
    draws["flip"] = (np.arange(B) % 2).astype(np.int32)                  # as tests/test_augment.py: every (flip, rotate, permute) combination
    draws["rotate"] = ((np.arange(B) // 2) % 4).astype(np.int32)
    draws["permute"] = ((np.arange(B) // 4) % 6).astype(np.int32)
    records = _records(T)
    sources = [n for n in SOURCE_PASSES if not (flip_on and n == "Normal")]      # the reference refuses to flip world-space normals
    jobs = [(n, SOURCE_PASSES[n], SOURCE_PASSES[n], False) for n in sources] + [("Diffuse Color", 3, 3, True), ("Alpha", 1, 3, True)]

    dev = {n: [torch.from_numpy(p).cuda() for p in ps] for n, ps in planes.items()}
    ptrs = {n: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).cuda() for n, ts in dev.items()}
    hw = torch.tensor([hw for hw in SIZES for _ in range(SOURCES + 1)], dtype=torch.int32).cuda()
    outs = [torch.full((B, T, T, ld), SENTINEL, dtype=torch.float32, device="cuda") for _, _, ld, _ in jobs]
    desc = L.TileSamplerDesc()
    desc.n_passes, desc.n_planes, desc.plane_hw = len(jobs), len(SIZES) * (SOURCES + 1), hw.data_ptr()
    for en, (name, ch, ld, from_target), out in zip(desc.pass_, jobs, outs):
        en.planes, en.dst, en.C, en.kind, en.ld_dst, en.from_target = ptrs[name].data_ptr(), out.data_ptr(), ch, DataAugmentation._kind(name, ch), ld, int(from_target)
    table = np.zeros(B, dtype=RECORD_DTYPE)
    for k, key in enumerate(("source_plane", "target_plane", "y0", "x0")):
        table[key] = records[:, k]
    for key in ("flip", "rotate", "permute"):
        table[key] = draws[key]
    table["normal_rotation"] = draws["normal_rotation"].reshape(B, 9)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    L.check(lib.dd_sample_tiles(ctypes.byref(desc), table_dev.data_ptr(), B, T, int(usage.use_flip_left_right), int(usage.use_rotate_90),
                                int(usage.use_rgb_permutation), int(usage.use_normal_rotation), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for (name, ch, ld, from_target), out in zip(jobs, outs):
        want = R.sample_batch(name, planes[name], records, from_target, T, None if mode == "crop" else draws, usage)
        have = out.cpu().numpy()
        assert want.shape == (B, T, T, ch)
        if name == "Normal" and mode != "crop":
            err = float(np.abs(have - want).max())
            print("T=%d %s Normal: max abs error %.3e (gate 2e-6)" % (T, mode, err))
            assert np.allclose(have, want, rtol=0, atol=2e-6), err
        else:
            bad = np.argwhere(have[..., :ch] != want)
            assert bad.size == 0, (name, from_target, T, mode, bad[:4].tolist())
        if ld > ch:      # channels C .. ld_dst-1 are not written: the sentinel stands
            assert (have[..., ch:] == SENTINEL).all(), name


# ---------------------------------------------------------------------------------------------------- end to end
T2, SPP, BEST, B2 = 16, 4, 16, 4
SCENES = ("scene_a", "scene_b")


def _architecture_json():
    return configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE",
                                combined={"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
                                          "Alpha": {"Color": "Alpha", "Direct": "", "Indirect": ""}})


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Two scenes of 32 x 48 pixels as EXR renderings (spp 4 twice, spp 16 once), and the SAME grid tiles as .tfrecords.gz with the reference's
    key names (TFRecordsCreator.py:136-160): per scene, `for i: for j:` one record with both source indices and the target."""
    from deepdenoiser_amd.architecture import Architecture
    root = str(tmp_path_factory.mktemp("frames_e2e"))
    aj = _architecture_json()
    aj["model_directory"] = "model"
    arch = Architecture(aj, device="cpu")
    source = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    target = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    rng = np.random.default_rng(3)
    base = os.path.join(root, "TFRecords")
    os.makedirs(os.path.join(base, "training"))
    h, w = 32, 48
    for n, scene in enumerate(SCENES):
        written = U.write_scene(root, scene, [SPP], list(source), target, h, w, rng, sources=2, target_spp=BEST)
        records = []
        for i in range(h // T2):
            for j in range(w // T2):
                win = (slice(i * T2, (i + 1) * T2), slice(j * T2, (j + 1) * T2))
                feats = {Naming.source_feature_name(name, samples_per_pixel=SPP, index=index): np.ascontiguousarray(written[(SPP, index)][name][win]).tobytes()
                         for index in range(2) for name in source}
                feats.update({Naming.target_feature_name(name): np.ascontiguousarray(written[(BEST, 0)][name][win]).tobytes() for name in target})
                records.append(tfrecords.serialize_example(feats))
        tfrecords.write_records(os.path.join(base, "training", "training_%d.tfrecords.gz" % n), records)
    frames_json = U.write_json(root, {"training": SCENES, "validation": SCENES[:1]}, T2, [SPP], 2, list(source), target)
    tj = configs.training(learning_rate=1e-3, batch_size=B2, image_mean=0.0)      # (no combined image: that needs all four combined features)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "no_such_directory", "modes": ["training", "validation"],
               "number_of_source_index_tuples": 2})
    json.dump(aj, open(os.path.join(root, "architecture.json"), "w"))
    json.dump(tj, open(os.path.join(root, "training.json"), "w"))
    return {"root": root, "aj": aj, "tj": tj, "frames_json": frames_json, "tfrecords": base, "grid": len(SCENES) * (h // T2) * (w // T2) * 2}


def test_frames_path_fills_the_buffers_like_the_tfrecords_path(dataset):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.frame_bank import FrameBank, FrameSet, TileSampler
    from deepdenoiser_amd.train import TileStream
    arch = Architecture(dataset["aj"], device="cuda", dtype="f32", seed=2)
    prog = arch.program(B2, T2, T2, training_json=dataset["tj"])
    tuples = [[0], [1]]
    stream = TileStream(os.path.join(dataset["tfrecords"], "training"), "training", arch, B2, T2, SPP, tuples, rng=None, threads=2)
    want = []
    for feats, labels in stream:
        prog.set_inputs({k: v.cuda() for k, v in feats.items()}, {k: v.cuda() for k, v in labels.items()})
        want.append(({k: v.clone() for k, v in prog.input.raw.items()}, prog.targets[0].clone()))
    assert len(want) == dataset["grid"] // B2 == 6
    for v in prog.input.raw.values():      # nothing of the first path is left behind
        v.fill_(SENTINEL)
    prog.targets[0].zero_()
    bank = FrameBank(arch, FrameSet.from_json(dataset["frames_json"], "training"), SPP, "cuda", threads=2)
    sampler = TileSampler(prog, bank, DataAugmentationUsage(True, False, True, True))
    records = sampler.grid_records(tuples)
    assert len(records) == dataset["grid"]
    for k, (raw, targets) in enumerate(want):
        sampler.sample(records[k * B2:(k + 1) * B2])                     # no draws: no augmentation
        torch.cuda.synchronize()
        for name, t in raw.items():
            assert torch.equal(prog.input.raw[name], t), (k, name)
        assert torch.equal(prog.targets[0], targets), k
    with pytest.raises(ValueError, match="origin"):
        bad = records[:B2].copy()
        bad[2, 3] = 48 - T2 + 1
        sampler.sample(bad)


def test_train_cli_from_frames(dataset, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd import train
    root = dataset["root"]
    args = train.parser().parse_args([os.path.join(root, "training.json"), "--frames", dataset["frames_json"], "--frames_crops", "random",
                                      "--train_epochs", "1", "--dtype", "f32", "--summary_steps", "0", "--threads", "2"])
    train.main(args)
    out = capsys.readouterr().out
    steps = dataset["grid"] // B2
    m = re.search(r"epoch 1: global_step (\d+), loss ([-+.\deinfa]+) ", out)
    assert m is not None, out
    assert int(m.group(1)) == steps and np.isfinite(float(m.group(2))), out
    assert "cut from resident frames" in out and "frames: training -- 2 scene(s), 6 planes" in out
    v = re.search(r"epoch 1: validation loss ([-+.\deinfa]+) over (\d+) batches", out)
    assert v is not None and np.isfinite(float(v.group(1))) and int(v.group(2)) == (32 // T2) * (48 // T2) * 2, out
    latest = tf_checkpoint.latest_checkpoint(os.path.join(root, "model"))
    assert latest is not None
    assert int(np.asarray(tf_checkpoint.read_checkpoint(latest)["global_step"]).reshape(-1)[0]) == steps
    assert not os.path.exists(os.path.join(root, "no_such_directory"))
