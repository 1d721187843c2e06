"""dd_sequence_quality on the device against tests/sequence_quality_ref.py (numpy float64), SequenceQuality over a short sequence, and
predict.main with --input_sequence / --target_sequence.

Tolerances.  The three pixel counts are exact: they hang on the previous position (the reference takes it in fp32, as the header states it)
and on the bits of the values read.  Every sum: |device - reference| <= 2e-6 * S, S the reference's sum over valid pixels and channels of
|p| + bil(|taps of pred_previous|) + |t| + bil(|taps of target_previous|) (in bytes for the ldr sums).  Derivation: a term is formed by at most
13 fp32 roundings (1 - fx, 1 - fy, the nine operations of a bilinear sample, the difference with it, the difference of differences) of 2^-24
each on operands bounded by S's summands: 13 * 2^-24 = 7.8e-7 of S; the gate leaves 2.5 x over that bound.  The bytes themselves are exact (an
fp32 product against the fp32 table on both sides).  A mean is gated by the same bound divided as the mean is."""
import json
import os

import numpy as np
import pytest
import torch

import sequence_quality_ref as R
from deepdenoiser_amd import _lib, metrics

pytestmark = pytest.mark.gpu

GATE = 2e-6
SENTINEL = 77.0
RECORD = 72
WORST = {"ratio": 0.0}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frame(values, layout):
    """values [H,W,C] -> (the device tensor of the pass, the whole device frame behind it): "dense" [H,W,C]; "view": the [..., :C] view of a
    frame two channels wider, sentinels in the unused channels (C 1: ld 3; C 3: ld 5)"""
    if layout == "dense":
        whole = torch.from_numpy(np.ascontiguousarray(values)).cuda()
        return whole, whole
    H, W, C = values.shape
    wide = np.full((H, W, C + 2), np.float32(SENTINEL), dtype=np.float32)
    wide[..., :C] = values
    whole = torch.from_numpy(wide).cuda()
    return whole[..., :C], whole


def _launch(lib, case, layouts, exposure=1.0, sx=-1.0, sy=1.0):
    """one dd_sequence_quality call -> (the records, their bytes); asserts that no input changed"""
    preds, pred_previouses, targets, target_previouses, motion = case
    H, W = motion.shape[:2]
    n = len(preds)
    wholes, before = [], []
    table = (_lib.SequenceQualityPair * n)()
    for k, layout in enumerate(layouts):
        four = [_frame(v[k], layout if j % 2 == 0 or k % 2 == 0 else "dense") for j, v in enumerate((preds, pred_previouses, targets, target_previouses))]
        wholes += [w for _, w in four]
        p, pp, t, tp = (v for v, _ in four)
        table[k] = _lib.SequenceQualityPair(p.data_ptr(), pp.data_ptr(), t.data_ptr(), tp.data_ptr(), p.stride(1), pp.stride(1), t.stride(1), tp.stride(1),
                                            preds[k].shape[2])
    mv = torch.from_numpy(motion).cuda()
    thr = torch.from_numpy(metrics.preview_thresholds()).cuda()
    wholes += [mv, thr]
    before = [w.cpu().numpy().tobytes() for w in wholes]
    records = torch.full((n * RECORD,), 0xA5, dtype=torch.uint8, device="cuda")
    nbytes = lib.dd_sequence_quality_scratch_bytes(n, H, W)
    assert nbytes > 0
    scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
    _lib.check(lib.dd_sequence_quality(table, n, H, W, mv.data_ptr(), mv.stride(1), sx, sy, thr.data_ptr(), exposure, records.data_ptr(), scratch.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    raw = records.cpu().numpy().tobytes()
    assert [w.cpu().numpy().tobytes() for w in wholes] == before                    # the inputs, sentinels included, bit for bit
    return (_lib.SequenceQualityRecord * n).from_buffer_copy(raw), raw


def _reference(case, exposure=1.0, sx=-1.0, sy=1.0):
    preds, pred_previouses, targets, target_previouses, motion = case
    thr = metrics.preview_thresholds()
    return [R.record(p, pp, t, tp, motion, sx, sy, thr, exposure) for p, pp, t, tp in zip(preds, pred_previouses, targets, target_previouses)]


def _compare(record, want, name):
    H, W = want["valid"].shape
    for k in R.COUNTS:
        assert getattr(record, k) == want[k], (name, k, getattr(record, k), want[k])
    assert sum(getattr(record, k) for k in R.COUNTS) == H * W, name
    worst = 0.0
    for k in R.SUMS + R.LDR_SUMS:
        have, S = getattr(record, k), want["S"][k]
        error = abs(have - want[k])
        worst = max(worst, error / S if S else 0.0)
        print("%s %s: device %.9g reference %.9g, |difference| / S = %.3g" % (name, k, have, want[k], error / S if S else 0.0))
        assert np.isfinite(have) and error <= GATE * S, (name, k, have, want[k], S)
    WORST["ratio"] = max(WORST["ratio"], worst)
    print("%s: worst |difference| / S = %.3g (gate %.1g); over all cases so far %.3g" % (name, worst, GATE, WORST["ratio"]))


MIX = ([3, 1, 3], ["dense", "view", "view"])        # a dense RGB pair, [..., :1] views of 3-wide frames (ld 3, nch 1), RGB at ld 5
CASES = [
    # H, W, (channels, layouts), sprinkle, exposure
    (45, 70, MIX, False, 1.0),
    (33, 37, MIX, False, 0.5),
    (1, 1, MIX, False, 1.0),
    (1, 40, MIX, False, 1.0),
    (40, 1, MIX, False, 1.0),
    (45, 70, MIX, True, 1.0),
    (33, 37, MIX, True, 2.0),
    (1, 4097, MIX, False, 1.0),               # 257 tiles: the second round of the finalize kernel's strided add
]


@pytest.mark.parametrize("H,W,mix,sprinkle,exposure", CASES)
def test_records_equal_the_reference(lib, H, W, mix, sprinkle, exposure):
    _need_gpu()
    channels, layouts = mix
    case = R.make_case(H, W, channels, seed=H * 1000 + W + int(sprinkle), sprinkle=sprinkle)
    want = _reference(case, exposure)
    first, first_raw = _launch(lib, case, layouts, exposure)
    second, second_raw = _launch(lib, case, layouts, exposure)
    for k in range(len(channels)):
        _compare(first[k], want[k], "%dx%d pair %d" % (H, W, k))
    assert first_raw == second_raw                                                  # two runs give the same bits
    if H * W > 1000:
        assert want[0]["pixels_valid"] > H * W // 2 and want[0]["pixels_offscreen"] > 0
        assert all(w[k] > 0 for w in want for k in R.SUMS + R.LDR_SUMS)
    if sprinkle:
        assert want[0]["pixels_nonfinite"] > 0 and want[-1]["pixels_nonfinite"] > 0 and want[0]["pixels_nonfinite"] != want[1]["pixels_nonfinite"]
    else:
        assert all(w["pixels_nonfinite"] == 0 for w in want)


def test_thirty_two_pairs_and_a_pair_alone(lib):
    """32 pairs at 33 x 37 in one call; the last and the first of them give the same bytes alone"""
    _need_gpu()
    H, W = 33, 37
    channels = [3 if k % 3 else 1 for k in range(32)]
    layouts = ["dense" if k % 2 else "view" for k in range(32)]
    case = R.make_case(H, W, channels, seed=32, sprinkle=True)
    want = _reference(case)
    records, raw = _launch(lib, case, layouts)
    for k in range(32):
        _compare(records[k], want[k], "pair %d of 32" % k)
    assert _launch(lib, case, layouts)[1] == raw
    alone = lambda k: _launch(lib, tuple(v[k:k + 1] for v in case[:4]) + (case[4],), layouts[k:k + 1])[1]      # noqa: E731
    assert alone(31) == raw[-RECORD:] and alone(0) == raw[:RECORD] and alone(17) == raw[17 * RECORD:18 * RECORD]


# ---------------------------------------------------------------------------------------------------- the host layer
def _sequence(H, W, frames, seed):
    """per frame ({name: prediction}, {name: target}, motion): noisy versions of one image"""
    rng = np.random.default_rng(seed)
    base = {"prediction/A": np.abs(rng.standard_normal((H, W, 3))), "prediction/Depth": np.abs(rng.standard_normal((H, W, 1)))}
    out = []
    for k in range(frames):
        targets = {n: (v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32) for n, v in base.items()}
        predictions = {n: (v + 0.2 * rng.standard_normal(v.shape)).astype(np.float32) for n, v in targets.items()}
        motion = R.make_case(H, W, [3], seed=seed + 10 + k)[4]
        out.append((predictions, targets, motion))
    return out


def _device_frame(frame):
    predictions, targets, motion = frame
    return ({"prediction/A": torch.from_numpy(predictions["prediction/A"]).cuda(), "prediction/Depth": _frame(predictions["prediction/Depth"], "view")[0]},
            {"prediction/Depth": _frame(targets["prediction/Depth"], "view")[0], "prediction/A": torch.from_numpy(targets["prediction/A"]).cuda(),
             "unused": torch.zeros(1)}, torch.from_numpy(motion).cuda())


def _check_figures(have, want_record, channels, name):
    want = R.figures(want_record, channels)
    values = want["pixels_valid"] * channels
    for k in R.COUNTS:
        assert have[k] == want[k], (name, k)
    for k in R.SUMS + R.LDR_SUMS:
        bound = GATE * want_record["S"][k] / values / (255.0 if k.startswith("ldr_") else 1.0)
        print("%s %s: %.9g reference %.9g (bound %.3g)" % (name, k, have[k], want[k], bound))
        assert abs(have[k] - want[k]) <= bound, (name, k, have[k], want[k])


def test_sequence_quality_over_frames_a_reset_and_a_size_change(lib):
    _need_gpu()
    from deepdenoiser_amd.sequence_quality import SequenceQuality
    thr = metrics.preview_thresholds()
    scorer = SequenceQuality("cuda", exposure=1.5, motion_scale=(-1.0, 1.0))
    assert scorer.summary() == {}
    frames = _sequence(33, 37, 4, seed=7) + _sequence(17, 20, 2, seed=9)            # a reset before frame 2, the size changes at frame 4
    measured = {n: [] for n in frames[0][0]}
    launches = []
    for k, frame in enumerate(frames):
        if k == 2:
            scorer.reset()
        predictions, targets, motion = _device_frame(frame)
        clones = {n: v.clone() for n, v in predictions.items()}
        result = scorer.measure(predictions, targets, motion)
        launches.append(scorer.launches)
        for n in predictions:                                                       # the history is the scorer's own copy: the caller's buffers are free again
            predictions[n].fill_(float("nan"))
            targets[n].fill_(float("nan"))
        if k in (0, 2, 4):
            assert result is None
            continue
        assert list(result) == list(clones)
        for n, p in frame[0].items():
            want = R.record(p, frames[k - 1][0][n], frame[1][n], frames[k - 1][1][n], frame[2], -1.0, 1.0, thr, 1.5)
            measured[n].append(want)
            _check_figures(result[n], want, p.shape[2], "frame %d %s" % (k, n))
    assert launches == [0, 1, 1, 2, 2, 3]
    summary = scorer.summary()
    assert list(summary) == list(measured)
    for n, records in measured.items():
        assert summary[n]["frames"] == 3
        _check_figures(summary[n], R.add_records(records), frames[0][0][n].shape[2], "summary %s" % n)
    # a changed key set: the frame becomes the history with no launch
    predictions, targets, motion = _device_frame(frames[5])
    only = {"prediction/A": predictions["prediction/A"]}
    assert scorer.measure(only, targets, motion) is None and scorer.launches == 3
    # what it refuses
    with pytest.raises(ValueError, match="no target for prediction/A, prediction/Depth"):
        scorer.measure(predictions, {}, motion)
    with pytest.raises(ValueError):
        scorer.measure(only, targets, motion.cpu())
    with pytest.raises(ValueError):
        scorer.measure(only, targets, motion[..., :1])
    with pytest.raises(ValueError):
        scorer.measure({"prediction/A": predictions["prediction/A"].double()}, targets, motion)
    with pytest.raises(ValueError):
        scorer.measure({"prediction/A": predictions["prediction/A"][:, ::2]}, targets, motion)
    with pytest.raises(ValueError):
        scorer.measure(only, {"prediction/A": targets["prediction/A"][..., :1]}, motion)
    for bad in (dict(exposure=float("nan")), dict(motion_scale=(1.0, float("inf"))), dict(motion_scale=(1.0,))):
        with pytest.raises(ValueError):
            SequenceQuality("cuda", **bad)


# ---------------------------------------------------------------------------------------------------- command line
FH, FW, T, O = 40, 56, 32, 4


def _run_main(tmp_path, extra):
    from deepdenoiser_amd import predict
    predict.main(predict.parser().parse_args([str(tmp_path / "architecture.json"), "--tile_size", str(T), "--tile_overlap_size", str(O), "--dtype", "f32"] + extra))


def _hwc(a):
    a = np.asarray(a, dtype=np.float32)
    return a[..., None] if a.ndim == 2 else a


def test_predict_target_sequence_end_to_end(tmp_path, capsys):
    _need_gpu()
    import frames_util
    from deepdenoiser_amd import configs, openexr, quality, tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import Predictor
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(FH, FW)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    loaded = [f.name for f in arch.feature_predictions + arch.auxiliary_features if f.load_data]
    members = [f.name for f in arch.feature_predictions if f.is_target and f.load_data]
    rng = np.random.default_rng(11)
    order = ["f1", "f2", "f10"]
    thr = metrics.preview_thresholds()
    motions = {}
    roots = {kind: tmp_path / kind for kind in ("single", "plain", "temporal", "refused", "targets", "incomplete")}
    for k, name in enumerate(["f2", "f10", "f1"]):                                  # written in this order; denoised as f1, f2, f10
        frames_util.write_rendering(str(roots["single"] / name), loaded, FH, FW, rng)
        frames_util.write_rendering(str(roots["targets"] / name), members, FH, FW, rng)
        motions[name] = R.make_case(FH, FW, [3], seed=60 + k)[4]
        for kind in ("plain", "temporal", "refused"):
            os.makedirs(roots[kind] / name)
            for n in os.listdir(roots["single"] / name):
                with open(roots["single"] / name / n, "rb") as f, open(roots[kind] / name / n, "wb") as g:
                    g.write(f.read())
            openexr.write_image(str(roots[kind] / name / "render_Motion Vector_0001.exr"), motions[name])
        if name != "f2":                                                            # `incomplete`: the targets without f2's
            os.makedirs(roots["incomplete"] / name)
            for n in os.listdir(roots["targets"] / name):
                with open(roots["targets"] / name / n, "rb") as f, open(roots["incomplete"] / name / n, "wb") as g:
                    g.write(f.read())
    os.makedirs(roots["incomplete"] / "f2")                                         # (there, but without .exr files)

    # a missing target directory ends the run before any frame is denoised
    with pytest.raises(SystemExit) as e:
        _run_main(tmp_path, ["--input_sequence", str(roots["refused"]), "--target_sequence", str(roots["incomplete"])])
    assert str(roots["incomplete"] / "f2") in str(e.value)
    assert not [n for name in order for n in os.listdir(roots["refused"] / name) if n.endswith(".npy") or n.endswith(".json")]

    # --input --target per frame: what the per-frame figures of a sequence run must equal
    for name in order:
        _run_main(tmp_path, ["--input", str(roots["single"] / name), "--target", str(roots["targets"] / name)])

    for kind, extra in (("plain", []), ("temporal", ["--temporal"])):
        capsys.readouterr()
        _run_main(tmp_path, ["--input_sequence", str(roots[kind]), "--target_sequence", str(roots["targets"])] + extra)
        printed = capsys.readouterr().out
        path = roots[kind] / "sequence_quality.json"
        assert str(path) in printed and "temporal_error" in printed
        document = json.load(open(path))
        assert set(document) == {"exposure", "motion_scale", "tile_size", "tile_overlap_size", "dtype", "nonfinite", "tile_blend", "temporal", "frames", "summary"}
        assert (document["exposure"], document["motion_scale"], document["tile_size"], document["tile_overlap_size"], document["dtype"]) == (1.0, [-1.0, 1.0], T, O, "f32")
        if kind == "plain":
            assert document["temporal"] is None and not os.path.exists(roots[kind] / "temporal.json")
        else:
            assert document["temporal"] == {"alpha": 0.8, "gamma": 1.0, "motion_scale": [-1.0, 1.0], "guides": []}
        assert [f["directory"] for f in document["frames"]] == order
        assert document["frames"][0]["temporal_quality"] is None
        keys = quality.target_names(arch)
        assert "Combined" in keys and all("prediction/" + m in keys for m in members)
        previous = None
        sums = {n: [] for n in keys}
        for k, name in enumerate(order):
            frame = document["frames"][k]
            assert set(frame) == {"directory", "quality", "temporal_quality"} and list(frame["quality"]) == keys
            per_frame = json.load(open(roots[kind] / name / "quality.json"))
            assert per_frame["quality"] == frame["quality"]
            if kind == "plain":                                                     # the frames are those of the --input runs: so are the figures
                assert per_frame == json.load(open(roots["single"] / name / "quality.json"))
            targets = {n: _hwc(v.cpu().numpy()) for n, v in quality.targets_of_frame(str(roots["targets"] / name), arch, device="cuda").items()}
            written = {n: _hwc(np.load(roots[kind] / name / ((n.split("/", 1)[1] if n.startswith("prediction/") else n) + ".npy"))) for n in keys}
            if k > 0:
                assert list(frame["temporal_quality"]) == keys
                for n in keys:
                    want = R.record(written[n], previous[0][n], targets[n], previous[1][n], motions[name], -1.0, 1.0, thr, 1.0)
                    sums[n].append(want)
                    _check_figures(frame["temporal_quality"][n], want, written[n].shape[2], "%s %s %s" % (kind, name, n))
                    assert want["pixels_valid"] > FH * FW // 2 and want["temporal_error"] > 0.0
            previous = (written, targets)
        assert list(document["summary"]) == keys
        for n in keys:
            s = document["summary"][n]
            assert set(s) == {"temporal_quality", "quality"} and s["temporal_quality"]["frames"] == 2
            _check_figures(s["temporal_quality"], R.add_records(sums[n]), written[n].shape[2], "%s summary %s" % (kind, n))
            for key, value in s["quality"].items():
                values = [f["quality"][n][key] for f in document["frames"] if f["quality"][n][key] is not None]
                assert value == (sum(values) / len(values) if values else None), (n, key)
    # the stabiliser changed what was scored
    plain, stable = (json.load(open(roots[kind] / "sequence_quality.json")) for kind in ("plain", "temporal"))
    assert plain["frames"][0]["quality"] == stable["frames"][0]["quality"]          # the first frame passes through
    assert plain["frames"][1]["temporal_quality"] != stable["frames"][1]["temporal_quality"]
    # --sequence_quality_json and --motion_scale without --temporal
    other = tmp_path / "elsewhere.json"
    _run_main(tmp_path, ["--input_sequence", str(roots["plain"]), "--target_sequence", str(roots["targets"]), "--motion_scale", "1", "1",
                         "--sequence_quality_json", str(other)])
    document = json.load(open(other))
    assert document["motion_scale"] == [1.0, 1.0] and document["frames"][1]["quality"] == plain["frames"][1]["quality"]
    assert document["frames"][1]["temporal_quality"] != plain["frames"][1]["temporal_quality"]
