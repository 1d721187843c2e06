"""Training from frames kept on the device, host side (deepdenoiser_amd/frame_bank.py; no GPU): scene discovery after OpenEXRDirectories.py:18-29
and OpenEXRDirectory.py:20, the five reasons a scene is skipped, the grid records in the loop order of TFRecordsCreator.py:125-133, the draws,
the record validation in front of the launch and the memory limit."""
import random

import numpy as np
import pytest
import torch

import frames_util as U
from deepdenoiser_amd import configs
from deepdenoiser_amd.architecture import Architecture
from deepdenoiser_amd.frame_bank import FrameBank, FrameSet, TileRecords

T, SPP, BEST, S = 16, 4, 16, 2


@pytest.fixture(scope="module")
def arch():
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE",
                              combined={"Diffuse": {"Color": "Diffuse Color", "Direct": "Diffuse Direct", "Indirect": "Diffuse Indirect"},
                                        "Alpha": {"Color": "Alpha", "Direct": "", "Indirect": ""}})
    return Architecture(aj, device="cpu")


def _passes(arch):
    source = [f.name for f in arch.feature_predictions + arch.auxiliary_features if f.load_data]
    target = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    return source, target


@pytest.fixture(scope="module")
def tree(tmp_path_factory, arch):
    """Two good scenes of different sizes (the first with a third, unused source rendering) and one scene per skip cause."""
    root = str(tmp_path_factory.mktemp("frames"))
    rng = np.random.default_rng(0)
    source, target = _passes(arch)
    written = {"a_good": U.write_scene(root, "a_good", [SPP], source, target, 32, 48, rng, sources=3, target_spp=BEST),
               "b_good": U.write_scene(root, "b_good", [SPP], source, target, 40, 33, rng, sources=2, target_spp=BEST)}
    import os
    # (1) a required pass is missing
    U.write_scene(root, "c_no_pass", [SPP], source, target, 32, 32, rng, target_spp=BEST)
    os.remove(os.path.join(root, "OpenEXR", "c_no_pass", U.rendering_name("c_no_pass", SPP, 1), "render_Normal_0001.exr"))
    # (2) a required spp is missing: only the target rendering exists
    U.write_scene(root, "d_no_spp", [], source, target, 32, 32, rng, target_spp=BEST)
    # (3) sizes differ within the scene
    U.write_scene(root, "e_sizes", [SPP], source, target, 32, 32, rng, target_spp=BEST)
    from deepdenoiser_amd import openexr
    openexr.write_image(os.path.join(root, "OpenEXR", "e_sizes", U.rendering_name("e_sizes", BEST, 0), "render_Alpha_0001.exr"), U.image(rng, 32, 40, "Alpha"))
    # (4) smaller than one tile
    U.write_scene(root, "f_small", [SPP], source, target, 12, 40, rng, target_spp=BEST)
    # (5) a non-finite sample (seen when the frames are decoded)
    U.write_scene(root, "g_nan", [SPP], source, target, 32, 32, rng, target_spp=BEST)
    bad = U.image(rng, 32, 32, "Diffuse Color")
    bad[5, 7, 1] = np.inf
    openexr.write_image(os.path.join(root, "OpenEXR", "g_nan", U.rendering_name("g_nan", SPP, 0), "render_Diffuse Color_0001.exr"), bad)
    scenes = ["a_good", "c_no_pass", "d_no_spp", "b_good", "e_sizes", "f_small", "g_nan", "h_absent"]
    path = U.write_json(root, {"training": scenes, "validation": ["c_no_pass"]}, T, [SPP], S, source, target)
    return root, path, written


def test_discovery_and_skipped_scenes(tree, arch):
    import os
    root, path, written = tree
    lines = []
    fs = FrameSet.from_json(path, "training", log=lines.append)
    assert (fs.tile, fs.number_of_sources_per_example, fs.source_spps) == (T, S, [SPP])
    # the scenes that pass the header checks, in the JSON's order (g_nan is found out when it is decoded)
    assert [os.path.basename(s.directory) for s in fs.scenes] == ["a_good", "b_good", "g_nan"]
    a = fs.scenes[0]
    # spp from the directory name, the renderings of one spp sorted by path, the first S of them are the sources; "best" = the largest spp
    assert FrameSet.renderings(a.directory).keys() == {SPP, BEST}
    assert [os.path.basename(p) for p in a.sources[SPP]] == [U.rendering_name("a_good", SPP, 0), U.rendering_name("a_good", SPP, 1)]
    assert os.path.basename(a.target) == U.rendering_name("a_good", BEST, 0) and a.target_spp == BEST
    assert (a.height, a.width) == (32, 48) and (fs.scenes[1].height, fs.scenes[1].width) == (40, 33)
    # one line per skipped scene, naming the cause
    assert len(lines) == 5 and len(fs.skipped) == 5
    by_scene = {os.path.basename(d): msg for d, msg in fs.skipped}
    assert "does not contain an exr file for Normal" in by_scene["c_no_pass"]
    assert "no subdirectory for %d samples per pixel" % SPP in by_scene["d_no_spp"]
    assert "40x32" in by_scene["e_sizes"] and "32x32" in by_scene["e_sizes"]
    assert "smaller than one tile of %d pixels" % T in by_scene["f_small"]
    assert "does not exist" in by_scene["h_absent"]
    for line in lines:
        assert line.startswith("frames: ") and " skipped: " in line
    # a set without a usable scene raises
    with pytest.raises(ValueError, match="no usable scene"):
        FrameSet.from_json(path, "validation", log=lines.append)
    with pytest.raises(KeyError):
        FrameSet.from_json(path, "testing")


@pytest.fixture(scope="module")
def bank(tree, arch):
    lines = []
    fs = FrameSet.from_json(tree[1], "training", log=lambda m: None)
    b = FrameBank(arch, fs, SPP, "cpu", threads=2, log=lines.append)
    b.lines = lines
    return b


def test_bank_holds_the_written_planes_and_skips_nonfinite(tree, arch, bank):
    import os
    root, path, written = tree
    # the fifth cause: a non-finite sample
    assert [os.path.basename(s.directory) for s in bank.scenes] == ["a_good", "b_good"]
    assert len(bank.lines) == 1 and "g_nan" in bank.lines[0] and "not finite" in bank.lines[0] and "Diffuse Color" in bank.lines[0]
    source, target = _passes(arch)
    assert bank.n_planes == 2 * (S + 1) and bank.hw == [(32, 48)] * 3 + [(40, 33)] * 3
    assert bank.plane_hw.tolist() == [list(x) for x in bank.hw]
    for s, scene in enumerate(["a_good", "b_good"]):
        for index in range(S):
            p = bank.source_plane(s, index)
            for name in source:
                assert np.array_equal(bank.planes[name][p].numpy(), written[scene][(SPP, index)][name]), (scene, index, name)
        p = bank.target_plane(s)
        for name in target:
            assert np.array_equal(bank.planes[name][p].numpy(), written[scene][(BEST, 0)][name])
        assert bank.planes["Normal"][p] is None and int(bank.pointers["Normal"][p]) == 0      # an auxiliary pass has no target plane
    assert int(bank.pointers["Alpha"][0]) == bank.planes["Alpha"][0].data_ptr()


def test_memory_limit_names_the_bytes(tree, arch):
    fs = FrameSet.from_json(tree[1], "training", log=lambda m: None)
    source, target = _passes(arch)
    ch = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features}
    per_pixel = 4 * (S * sum(ch[n] for n in source) + sum(ch[n] for n in target))
    total = (32 * 48 + 40 * 33 + 32 * 32) * per_pixel      # (g_nan counts: the bytes are known before anything is decoded)
    with pytest.raises(MemoryError, match=r"%d bytes.*limit is %d bytes" % (total, total - 1)):
        FrameBank(arch, fs, SPP, "cpu", memory_limit_bytes=total - 1)
    with pytest.raises(ValueError, match="samples per pixel"):
        FrameBank(arch, fs, 8, "cpu")


def test_grid_records_in_the_reference_loop_order(bank):
    rec = TileRecords(bank, 4)
    tuples = [[0], [1], [1]]
    got = rec.grid_records(tuples).tolist()
    want = []
    for s, (h, w) in enumerate([(32, 48), (40, 33)]):
        for i in range(h // T):
            for j in range(w // T):
                for tup in tuples:
                    want.append([s * (S + 1) + tup[0], s * (S + 1) + S, i * T, j * T])
    assert got == want and len(want) == (2 * 3 + 2 * 2) * 3 == rec.epoch_examples(tuples)


@pytest.mark.parametrize("crops", ["random", "grid"])
def test_draws_are_deterministic_in_bounds_and_shard_over_ranks(bank, crops):
    B, world, tuples = 3, 2, [[0], [1]]
    n = TileRecords(bank, B).epoch_examples(tuples)          # 20 examples: three rounds of world * B, the remaining 2 are dropped

    def epoch(rank, world, B, seed=7):
        rec, rng, out = TileRecords(bank, B), random.Random(seed), []
        while True:
            r = rec.draw(rng, crops, tuples, rank, world)
            if r is None:
                return out
            rec.validate(r)                                   # inside [0, h-T] x [0, w-T], planes in range
            out.append(r)
    r0, r1, again = epoch(0, world, B), epoch(1, world, B), epoch(0, world, B)
    assert len(r0) == len(r1) == n // (world * B) == 3
    assert all(np.array_equal(a, b) for a, b in zip(r0, again))                       # deterministic for a seed
    assert not all(np.array_equal(a, b) for a, b in zip(r0, epoch(0, world, B, seed=8)))
    whole = epoch(0, 1, world * B)                                                     # the global draw
    for k in range(3):
        assert np.array_equal(np.concatenate([r0[k], r1[k]]), whole[k])                # disjoint slices, their union is the global draw
    flat = np.concatenate(whole)
    if crops == "grid":      # a shuffle of the grid set: every tile at most once
        grid = {tuple(r) for r in TileRecords(bank, B).grid_records(tuples).tolist()}
        assert len({tuple(r) for r in flat.tolist()}) == len(flat) and {tuple(r) for r in flat.tolist()} <= grid
    else:
        assert (flat[:, 2] % T != 0).any() and (flat[:, 3] % T != 0).any()             # not on the grid
    for sp, tp, y0, x0 in flat.tolist():
        h, w = bank.hw[sp]
        assert tp == sp // (S + 1) * (S + 1) + S and sp % (S + 1) < S and 0 <= y0 <= h - T and 0 <= x0 <= w - T
    # the next call starts the next epoch
    rec, rng = TileRecords(bank, B), random.Random(1)
    while rec.draw(rng, crops, tuples) is not None:
        pass
    assert rec.draw(rng, crops, tuples) is not None
    with pytest.raises(ValueError):
        rec.draw(rng, "spiral", tuples)


def test_record_validation(bank):
    rec = TileRecords(bank, 2)
    good = np.array([[0, 2, 16, 32], [4, 5, 24, 17]], dtype=np.int32)      # the far corners: (h-T, w-T) of 32x48 and of 40x33
    rec.validate(good)
    table = rec.pack(good, {"flip": [1, 0], "rotate": [3, 2], "permute": [5, 4], "normal_rotation": np.arange(18, dtype=np.float32).reshape(2, 3, 3)})
    assert table.tobytes()[:28] == np.array([0, 2, 16, 32, 1, 3, 5], dtype="<i4").tobytes() and table["normal_rotation"][1].tolist() == list(range(9, 18))
    for row, message in (([0, 2, 17, 32], "origin"), ([0, 2, 16, 33], "origin"), ([0, 2, -1, 0], "origin"), ([4, 5, 25, 0], "origin"),
                         ([6, 2, 0, 0], "out of range"), ([0, -1, 0, 0], "out of range"), ([0, 6, 0, 0], "out of range"),
                         ([2, 2, 0, 0], "no source plane"), ([0, 1, 0, 0], "no target plane"), ([0, 5, 0, 0], "the source plane is")):
        bad = good.copy()
        bad[1] = row
        with pytest.raises(ValueError, match=message):
            rec.validate(bad)
    with pytest.raises(ValueError, match="expected"):
        rec.validate(good[:1])


def test_synthetic_bank_and_command_line(arch):
    """FrameBank.synthetic (tools/tile_sampler_timing.py) lays its planes out like a decoded bank; the --frames flags of train.py."""
    b = FrameBank.synthetic(arch, T, [(20, 24), (17, 33)], sources=2, device="cpu", seed=1)
    source, target = _passes(arch)
    assert b.n_planes == 6 and b.hw == [(20, 24)] * 3 + [(17, 33)] * 3 and b.plane_hw.tolist() == [list(x) for x in b.hw]
    for p in range(6):
        is_target = p % 3 == 2
        for name in source:
            t = b.planes[name][p]
            assert (t is not None) == ((name in target) if is_target else True), (name, p)
            if t is not None:
                assert tuple(t.shape[:2]) == b.hw[p] and t.dtype == torch.float32 and int(b.pointers[name][p]) == t.data_ptr()
    assert b.total_bytes == sum(t.numel() * 4 for ts in b.planes.values() for t in ts if t is not None)
    TileRecords(b, 2).validate(np.array([[0, 2, 4, 8], [4, 5, 1, 17]], dtype=np.int32))
    from deepdenoiser_amd import train
    args = train.parser().parse_args(["t.json"])
    assert (args.frames, args.frames_spp, args.frames_crops, args.frame_memory_gb) == (None, None, "random", None)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_spp", "8", "--frames_crops", "grid", "--frame_memory_gb", "1.5"])
    assert (args.frames, args.frames_spp, args.frames_crops, args.frame_memory_gb) == ("f.json", 8, "grid", 1.5)
    with pytest.raises(SystemExit):
        train.parser().parse_args(["t.json", "--frames_crops", "spiral"])
