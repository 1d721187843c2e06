"""-m gpu: dd_stitch_blend through the C-ABI against tests/blend_ref.py, Predictor(tile_blend="feather"), and what the blend does to the
step along tile borders.

The op bound: a term is fl(fl(w_y) * fl(w_x)) * v added by one FMA -- three roundings of the weight (2^-24 relative each, two stored
weights and their product) and one per FMA, at most nine FMAs where three tile rows meet three tile columns: 12 * 2^-24 = 7.2e-7 of the
largest |tile value| (the weights of a pixel add up to 1).  Gated at 2e-6 * max |tile value|."""
import numpy as np
import pytest
import torch

import blend_ref as R
from deepdenoiser_amd.naming import Naming
from deepdenoiser_amd.tiling import tile_plan

pytestmark = pytest.mark.gpu

BOUND = 2e-6
OP_CASES = [(61, 45, 32, 4, 3, 3), (100, 37, 24, 3, 3, 3), (61, 45, 32, 4, 4, 4)]      # H, W, tile, overlap, ldt, ldf
NF, C = 2, 3


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _blend_on_device(lib, tiles, plan, per_launch, ldf, pad_slot=False):
    """tiles: [NF, count, T, T, ldt] device tensor.  The plan's tiles go through dd_stitch_blend `per_launch` at a time, in ascending order, into
    [NF, H, W, ldf] frames pre-filled with NaN.  pad_slot: the launch buffers hold one slot more per image than tiles (a ragged batch's
    repeated tile), filled with NaN, which must not contribute."""
    from deepdenoiser_amd.prediction import BlendTables
    tables = BlendTables(plan, "cuda")
    frames = torch.full((tiles.shape[0], plan.height, plan.width, ldf), float("nan"), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for first in range(0, plan.count, per_launch):
        n = min(per_launch, plan.count - first)
        per = n + (1 if pad_slot else 0)
        buf = torch.full((tiles.shape[0], per) + tuple(tiles.shape[2:]), float("nan"), dtype=torch.float32, device="cuda")
        buf[:, :n] = tiles[:, first:first + n]
        tables.blend(lib, buf.data_ptr(), tiles.shape[-1], per, frames, C, first, n, stream)
    torch.cuda.synchronize()
    return frames


def _single_cover(plan):
    """[H, W] bool: pixels exactly one tile covers"""
    cy = R.cover_counts(plan.rows.origins, plan.tile, plan.height)
    cx = R.cover_counts(plan.cols.origins, plan.tile, plan.width)
    return (cy[:, None] == 1) & (cx[None, :] == 1)


@pytest.mark.parametrize("case", OP_CASES, ids=["%dx%d_%d_%d_ldt%d_ldf%d" % c for c in OP_CASES])
def test_op_matches_the_reference_for_every_split(lib, case):
    """random tiles (overlapping tiles disagree), launches of 1, 3 and all tiles"""
    _need_gpu()
    H, W, T, O, ldt, ldf = case
    plan = tile_plan(H, W, T, O)
    assert (plan.tile, plan.overlap) == (T, O)
    rng = np.random.default_rng(H)
    host = rng.standard_normal((NF, plan.count, T, T, ldt)).astype(np.float32)
    host[..., C:] = np.nan                                             # a channel past C is not the kernel's business
    tiles = torch.from_numpy(host).cuda()
    whole = _blend_on_device(lib, tiles, plan, plan.count, ldf)
    got = whole.cpu().numpy()
    assert np.isfinite(got[..., :C]).all()                             # every float written, none started from the NaN that was there
    if ldf > C:
        assert np.isnan(got[..., C:]).all()                            # ... and the channel past C left alone
    bound = BOUND * float(np.abs(host[..., :C]).max())
    single = _single_cover(plan)
    assert single.any() and not single.all()
    worst = 0.0
    for f in range(NF):
        want = R.blend(host[f][..., :C], plan.rows.origins, plan.cols.origins, T, H, W, 2 * O, 2 * O)
        worst = max(worst, float(np.abs(got[f][..., :C] - want).max()))
        assert np.array_equal(got[f][..., :C][single], want[single].astype(np.float32))      # weight 1.0: the tile's value, bit for bit
    print("max |device - reference| %.3e, bound %.3e" % (worst, bound))
    assert worst <= bound
    for per_launch, pad in ((1, False), (3, False), (3, True)):
        split = _blend_on_device(lib, tiles, plan, per_launch, ldf, pad_slot=pad)
        assert torch.equal(split[..., :C], whole[..., :C]), (per_launch, pad)
        assert ldf == C or bool(torch.isnan(split[..., C:]).all())


def test_tiles_cut_from_a_frame_give_it_back(lib):
    _need_gpu()
    H, W, T, O = 100, 37, 24, 3
    plan = tile_plan(H, W, T, O)
    rng = np.random.default_rng(1)
    frame = rng.standard_normal((NF, H, W, C)).astype(np.float32)
    host = np.stack([np.stack([frame[f, y:y + T, x:x + T] for y, x in plan.windows()]) for f in range(NF)])
    got = _blend_on_device(lib, torch.from_numpy(host).cuda(), plan, 4, C).cpu().numpy()
    worst = float(np.abs(got - frame).max())
    print("max |blend of a frame's own tiles - frame| %.3e" % worst)
    assert worst <= BOUND * float(np.abs(frame).max())
    # a one-tile frame: weight 1.0 everywhere, the tile bit for bit
    plan = tile_plan(16, 16, 128, 14)
    assert plan.count == 1 and plan.tile == 16
    one = rng.standard_normal((NF, 1, 16, 16, C)).astype(np.float32)
    got = _blend_on_device(lib, torch.from_numpy(one).cuda(), plan, 1, C).cpu().numpy()
    assert np.array_equal(got.view(np.int32), one[:, 0].view(np.int32))


# ---------------------------------------------------------------------------------------------------- Predictor
H, W, T, O = 61, 77, 32, 4                                             # 3 x 3 tiles; the last tile row overlaps both rows above it


@pytest.fixture(scope="module")
def network():
    """the seam architecture on the device with the float64 oracle's weights, and the oracle"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import Predictor
    from oracle.model import OracleArchitecture
    aj = R.seam_architecture()
    oracle = OracleArchitecture(aj, dtype=torch.float64, seed=R.SEAM_SEED)
    arch = Architecture(aj, device="cuda", dtype="f32")
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(H, W)                           # builds a tile program => creates the parameters
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():                                                                     # the oracle creates its variables on first use
        oracle.predict({Naming.source_feature_name(f.name, index=0): torch.randn(1, 16, 16, f.channels, generator=g).abs()
                        for f in oracle.features + oracle.auxiliary})
    assert [p.name for p in arch.params.params] == list(oracle.vs.vars.keys())
    arch.params.load_list(list(oracle.vs.vars.values()))
    return arch, oracle


def _frame(oracle, seed):
    g = torch.Generator().manual_seed(seed)
    frame = {}
    for f in oracle.features + oracle.auxiliary:
        v = torch.randn(H, W, f.channels, generator=g)
        frame[Naming.source_feature_name(f.name, index=0)] = v if "Normal" in f.name else v.abs()
    return frame


def _outputs(pred, frame):
    out = {k: v.clone() for k, v in pred.predict_frame(frame).items()}
    torch.cuda.synchronize()
    return out


def test_crop_is_the_default_and_unchanged(network):
    from deepdenoiser_amd.prediction import Predictor
    arch, oracle = network
    frame = _frame(oracle, 3)
    kw = dict(tile_size=T, tile_overlap_size=O, tiles_per_batch=5)
    plain, crop = Predictor(arch, **kw), Predictor(arch, tile_blend="crop", **kw)
    assert plain.tile_blend == "crop" and plain._blends == {}
    a, b = _outputs(plain, frame), _outputs(crop, frame)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert crop._blends == {}
    feather = _outputs(Predictor(arch, tile_blend="feather", **kw), frame)
    assert set(feather) == set(a) and not all(torch.equal(a[k], feather[k]) for k in a)      # (the tiles do disagree)


@pytest.mark.parametrize("use_graph", [True, False])
def test_feather_does_not_depend_on_the_batching(network, use_graph):
    from deepdenoiser_amd.prediction import Predictor
    arch, oracle = network
    frames = [_frame(oracle, 3), _frame(oracle, 4)]
    want = None
    for per_batch in (1, 5, 64):
        pred = Predictor(arch, tile_size=T, tile_overlap_size=O, tiles_per_batch=per_batch, use_graph=use_graph, tile_blend="feather")
        got = [_outputs(pred, fr) for fr in frames]                    # the second frame runs through the cached plan, tables and graph
        assert all(bool(torch.isfinite(v).all()) for o in got for v in o.values())
        if want is None:
            want = got
            assert not torch.equal(got[0]["prediction/Emission"], got[1]["prediction/Emission"])
        for o, w in zip(got, want):
            assert set(o) == set(w)
            for k in o:
                assert torch.equal(o[k], w[k]), (per_batch, k)


def test_feather_is_the_reference_blend_of_the_predicted_tiles(network, monkeypatch):
    from deepdenoiser_amd.prediction import Predictor
    from gpu_util import read
    arch, oracle = network
    frame = _frame(oracle, 3)
    pred = Predictor(arch, tile_size=T, tile_overlap_size=O, tiles_per_batch=5, tile_blend="feather")
    plan, prog, chunks = pred._frame_plan(H, W)
    assert plan.count == 9 and len(chunks) == 2 and prog.NF == 1      # 5 + 4: the second batch carries a repeated tile
    batches = []
    forward = pred._forward

    def recording(p):
        forward(p)
        torch.cuda.synchronize()
        batches.append(read(p.predictions[0]).numpy().copy())          # [NF * Bt, T, T, 3] of this batch

    monkeypatch.setattr(pred, "_forward", recording)
    out = _outputs(pred, frame)
    assert len(batches) == 2
    tiles = np.concatenate([batches[0], batches[1][:4]])                 # (slot 4 of the second batch is the repeated tile: not blended in)
    want = R.blend(tiles, plan.rows.origins, plan.cols.origins, T, H, W, 2 * O, 2 * O)
    got = out["prediction/Emission"].cpu().numpy()
    worst, bound = float(np.abs(got - want).max()), BOUND * float(np.abs(tiles).max())
    print("max |Predictor - reference blend of its own tiles| %.3e, bound %.3e" % (worst, bound))
    assert worst <= bound
    # blend_width reaches the tables: 0 is the plain average
    flat = Predictor(arch, tile_size=T, tile_overlap_size=O, tiles_per_batch=5, tile_blend="feather", blend_width=0)
    got = _outputs(flat, frame)["prediction/Emission"].cpu().numpy()
    assert float(np.abs(got - R.blend(tiles, plan.rows.origins, plan.cols.origins, T, H, W, 0, 0)).max()) <= bound


def test_feather_removes_the_step_along_tile_borders(network):
    """out - (the untiled prediction) keeps the tiling error alone; its pixel-to-pixel difference across the crop plan's interior seams
    against the same statistic of the crop.  The ramp spreads a disagreement A - B over 12 pixels: expected ~1/12 plus the drift of the
    error inside a tile.  Measured (columns, rows): float64 oracle crop 1.30e-2, 1.13e-2, feather 1.26e-3, 1.11e-3; device: see DESIGN 3.21."""
    from deepdenoiser_amd.prediction import Predictor
    arch, oracle = network
    n = R.SEAM_FRAME
    frame = R.seam_frame([(f.name, f.channels) for f in oracle.features + oracle.auxiliary])
    key = "prediction/Emission"
    whole = _outputs(Predictor(arch, tile_size=n, tile_overlap_size=R.SEAM_OVERLAP), frame)[key].cpu().numpy()
    kw = dict(tile_size=R.SEAM_TILE, tile_overlap_size=R.SEAM_OVERLAP)
    crop = _outputs(Predictor(arch, **kw), frame)[key].cpu().numpy()
    feather = _outputs(Predictor(arch, tile_blend="feather", **kw), frame)[key].cpu().numpy()
    plan = tile_plan(n, n, R.SEAM_TILE, R.SEAM_OVERLAP)
    assert tile_plan(n, n, n, R.SEAM_OVERLAP).count == 1 and plan.count == 9
    seams = plan.cols.offsets[1:], plan.rows.offsets[1:]
    s_crop, s_feather = R.seam_statistic(crop - whole, *seams), R.seam_statistic(feather - whole, *seams)
    print("seam statistic (columns, rows): crop %.3e %.3e, feather %.3e %.3e" % (s_crop + s_feather))
    for c, f in zip(s_crop, s_feather):
        assert c > 0
        assert f <= R.SEAM_FACTOR * c


# ---------------------------------------------------------------------------------------------------- command line
def test_predict_tile_blend_feather_with_a_target(tmp_path, capsys):
    """python -m deepdenoiser_amd.predict --tile_blend feather --target: the recombined passes and the scores are those of the blended frames,
    quality.json says which blend it scored."""
    _need_gpu()
    import json
    from deepdenoiser_amd import configs, openexr, predict, quality, tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import Predictor
    FH, FW = 40, 72
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(FH, FW)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    rng = np.random.default_rng(5)
    src, tgt = tmp_path / "frame_0001_16_0_0", tmp_path / "frame_0001_target"
    src.mkdir()
    tgt.mkdir()
    for f in arch.feature_predictions + arch.auxiliary_features:
        if not f.load_data:
            continue
        clean = rng.random((FH, FW, 3)).astype(np.float32)
        if f.number_of_channels == 1:
            clean[...] = clean[..., :1]
        openexr.write_image(str(src / ("render_%s_0001.exr" % f.name)), (clean * (1.0 + 0.3 * rng.standard_normal((FH, FW, 1)))).astype(np.float32))
        openexr.write_image(str(tgt / ("target_%s_0001.exr" % f.name)), clean)
    names = quality.target_names(arch)
    assert "Combined" in names
    base = [str(tmp_path / "architecture.json"), "--input", str(src), "--tile_size", str(T), "--tile_overlap_size", str(O), "--dtype", "f32",
            "--target", str(tgt)]
    written = {}
    for mode in ("crop", "feather"):
        predict.main(predict.parser().parse_args(base + ([] if mode == "crop" else ["--tile_blend", "feather"])))
        document = json.load(open(src / "quality.json"))
        assert document["tile_blend"] == mode
        assert (document["tile_size"], document["tile_overlap_size"], document["dtype"], document["nonfinite"], document["exposure"]) == (T, O, "f32", "keep", 1.0)
        assert list(document["quality"]) == names
        written[mode] = {n: np.load(src / (n.split("/", 1)[-1] + ".npy")) for n in names}
        again = quality.FrameQuality("cuda").measure({n: torch.from_numpy(v) for n, v in written[mode].items()}, quality.targets_of_frame(str(tgt), arch))
        assert again == document["quality"]
    assert all(np.isfinite(v).all() for v in written["feather"].values())
    assert not np.array_equal(written["crop"]["Combined"], written["feather"]["Combined"])
    # 'Combined' is the recombination of the BLENDED passes (Prediction.py:469-481 in fp32, as dd_recombine rounds it)
    w = written["feather"]
    want = None
    for c in ("Diffuse", "Glossy", "Subsurface", "Transmission"):
        v = w["prediction/" + c + " Color"] * (w["prediction/" + c + " Direct"] + w["prediction/" + c + " Indirect"])
        assert np.array_equal(v, w["prediction/" + c])
        want = v if want is None else want + v
    for s in ("Volume Direct", "Volume Indirect", "Environment", "Emission"):
        want = want + w["prediction/" + s]
    assert np.array_equal(want, w["Combined"])
