"""dd_temporal_stabilize on the device against tests/temporal_ref.py (numpy float64), TemporalStabilizer over a short sequence against the
reference chained over it, and predict.main with --input_sequence / --temporal.

Tolerances.  out: atol = rtol = 1e-5 -- under twenty fp32 roundings on values of magnitude <= 4 (an fp32 restatement of the reference differs
from float64 by 6e-7 at most).  The four pixel counts are exact: the inputs of these tests put the previous positions on multiples of 1/8
pixel and the guides on multiples of 0.5 (tolerance 0.25), so no decision hangs on a rounding.  values_clamped may differ by the number of
channels the reference calls ambiguous (h within 1e-4 of a clamp bound), and every case asserts on the reference alone that those are at
most 0.5 % of its channels.  The three sums: 1e-5 relative."""
import json
import os

import numpy as np
import pytest
import torch

import temporal_ref as R
from deepdenoiser_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(123.25)
TOL = 1e-5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frame(values, layout, fill=77.0):
    """values [H,W,C] -> the device tensor of the pass: "dense" [H,W,C]; "view": the [..., :C] view of a frame two channels wider"""
    if layout == "dense":
        return torch.from_numpy(np.ascontiguousarray(values)).cuda()
    H, W, C = values.shape
    wide = np.full((H, W, C + 2), np.float32(fill), dtype=np.float32)
    wide[..., :C] = values
    return torch.from_numpy(wide).cuda()[..., :C]


def _launch(lib, currents, histories, motion, guides, alpha, gamma, layouts, sx=-1.0, sy=1.0):
    """one dd_temporal_stabilize call -> ([the WHOLE out frame of every pass as numpy, sentinel channels included], the records, their bytes)"""
    H, W = motion.shape[:2]
    n = len(currents)
    keep, outs = [], []
    table = (_lib.TemporalPass * n)()
    for k, (c, h, layout) in enumerate(zip(currents, histories, layouts)):
        cur, his = _frame(c, layout), _frame(h, "dense" if layout == "dense" else "view", fill=55.0)
        out = _frame(np.full(c.shape, SENTINEL, dtype=np.float32), layout, fill=float(SENTINEL))
        keep += [cur, his]
        outs.append(out)
        table[k] = _lib.TemporalPass(cur.data_ptr(), his.data_ptr(), out.data_ptr(), cur.stride(1), his.stride(1), out.stride(1), c.shape[2])
    gtable = (_lib.TemporalGuide * max(len(guides), 1))()
    for k, (gc, gp, tolerance) in enumerate(guides):
        a, b = _frame(gc, "dense"), _frame(gp, "view" if k % 2 else "dense")
        keep += [a, b]
        gtable[k] = _lib.TemporalGuide(a.data_ptr(), b.data_ptr(), a.stride(1), b.stride(1), gc.shape[2], tolerance)
    mv = torch.from_numpy(motion).cuda()
    records = torch.full((n * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    nbytes = lib.dd_temporal_scratch_bytes(n, H, W)
    assert nbytes > 0
    scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device="cuda")
    _lib.check(lib.dd_temporal_stabilize(table, n, gtable, len(guides), H, W, mv.data_ptr(), mv.stride(1), sx, sy, alpha, gamma, records.data_ptr(),
                                         scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
    raw = records.cpu().numpy().tobytes()
    whole = []
    for out, c in zip(outs, currents):
        base = out if out.is_contiguous() else torch.as_strided(out, (H, W, c.shape[2] + 2), (out.stride(0), out.stride(1), 1))
        whole.append(base.cpu().numpy())
    return whole, (_lib.TemporalRecord * n).from_buffer_copy(raw), raw


def _compare(have, record, want, current, name):
    C = current.shape[2]
    out = have[..., :C]
    for k in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended"):
        assert getattr(record, k) == want[k], (name, k, getattr(record, k), want[k])
    assert (have[..., C:] == SENTINEL).all(), name                                   # channels nch .. ld-1 are not touched
    rejected = ~want["blended"]
    assert np.array_equal(out[rejected].view(np.uint32), current[rejected].view(np.uint32)), name      # bit for bit, NaN payloads included
    a, b = out[want["blended"]].astype(np.float64), want["out"][want["blended"]].astype(np.float64)
    assert np.isfinite(a).all(), name
    error = np.abs(a - b) - TOL * np.abs(b)
    print("%s: max |out - reference| %.3g, clamped %d (reference %d, ambiguous %d)" % (name, np.abs(a - b).max() if a.size else 0.0, record.values_clamped,
                                                                                       want["values_clamped"], want["ambiguous"].sum()))
    assert (error <= TOL).all(), (name, float(np.abs(a - b).max()))
    assert want["ambiguous"].sum() <= 0.005 * current.size, name                    # the condition, on the reference alone
    assert abs(int(record.values_clamped) - want["values_clamped"]) <= want["ambiguous"].sum(), name
    for k in ("change", "flicker_before", "flicker_after"):
        assert abs(getattr(record, k) - want[k]) <= TOL * abs(want[k]), (name, k, getattr(record, k), want[k])


MIX = ([3, 1, 3], ["dense", "view", "view"])        # a dense RGB pass, a [..., :1] view of a 3-wide frame (ld 3, nch 1), RGB at ld 5
CASES = [
    # H, W, (channels, layouts), guides, sprinkle, alpha, gamma
    (45, 70, MIX, 2, False, 0.8, 1.0),
    (45, 70, ([3], ["dense"]), 0, False, 1.0, 0.5),
    (33, 37, MIX, 0, False, 0.0, 0.5),
    (33, 37, MIX, 2, False, 1.0, 1.0),
    (1, 1, MIX, 2, False, 0.8, 1.0),
    (1, 40, MIX, 2, False, 0.8, 1.0),
    (40, 1, MIX, 0, False, 0.8, 0.5),
    (45, 70, MIX, 2, True, 0.8, 1.0),
    (33, 37, MIX, 0, True, 1.0, 0.5),
    (1, 4097, MIX, 2, False, 0.8, 1.0),       # 257 tiles: the second round of the finalize kernel's strided add
]


@pytest.mark.parametrize("H,W,mix,guides,sprinkle,alpha,gamma", CASES)
def test_stabilize_equals_the_reference(lib, H, W, mix, guides, sprinkle, alpha, gamma):
    _need_gpu()
    channels, layouts = mix
    currents, histories, motion, guide_list = R.make_case(H, W, channels, seed=H * 1000 + W + guides, guides=guides, sprinkle=sprinkle)
    want = R.stabilize(list(zip(currents, histories)), motion, -1.0, 1.0, alpha, gamma, guide_list)
    first = _launch(lib, currents, histories, motion, guide_list, alpha, gamma, layouts)
    second = _launch(lib, currents, histories, motion, guide_list, alpha, gamma, layouts)
    for k, current in enumerate(currents):
        _compare(first[0][k], first[1][k], want[k], current, "%dx%d pass %d" % (H, W, k))
        assert first[0][k].tobytes() == second[0][k].tobytes()                      # two runs give the same bits
    assert first[2] == second[2]
    if H * W > 1000:
        assert want[0]["pixels_blended"] > H * W // 4 and want[0]["pixels_offscreen"] > 0 and (guides == 0 or want[0]["pixels_guide"] > 0)
    if sprinkle:
        assert want[0]["pixels_nonfinite"] > 0 and want[-1]["pixels_nonfinite"] > 0 and want[0]["pixels_nonfinite"] != want[1]["pixels_nonfinite"]


def test_thirty_two_passes_and_a_pass_alone(lib):
    """32 passes at 33 x 37 in one call; the last of them gives the same bytes alone"""
    _need_gpu()
    H, W = 33, 37
    channels = [3 if k % 3 else 1 for k in range(32)]
    layouts = ["dense" if k % 2 else "view" for k in range(32)]
    currents, histories, motion, guide_list = R.make_case(H, W, channels, seed=32, guides=2)
    want = R.stabilize(list(zip(currents, histories)), motion, -1.0, 1.0, 0.8, 1.0, guide_list)
    outs, records, raw = _launch(lib, currents, histories, motion, guide_list, 0.8, 1.0, layouts)
    for k, current in enumerate(currents):
        _compare(outs[k], records[k], want[k], current, "pass %d of 32" % k)
    alone_out, _, alone_raw = _launch(lib, currents[-1:], histories[-1:], motion, guide_list, 0.8, 1.0, layouts[-1:])
    assert alone_out[0].tobytes() == outs[-1].tobytes() and alone_raw == raw[-64:]
    first_out, _, first_raw = _launch(lib, currents[:1], histories[:1], motion, guide_list, 0.8, 1.0, layouts[:1])
    assert first_out[0].tobytes() == outs[0].tobytes() and first_raw == raw[:64]


# ---------------------------------------------------------------------------------------------------- the host layer
def _sequence(H, W, frames, seed):
    """per frame: ({name: [H,W,C]} predictions, motion, guide) in the generators' form; consecutive frames are noisy versions of one image"""
    rng = np.random.default_rng(seed)
    base = {"prediction/A": np.abs(rng.standard_normal((H, W, 3))), "prediction/Depth": np.abs(rng.standard_normal((H, W, 1)))}
    out = []
    for k in range(frames):
        predictions = {n: (v + 0.3 * rng.standard_normal(v.shape)).astype(np.float32) for n, v in base.items()}
        _, _, motion, guide_list = R.make_case(H, W, [3], seed=seed + 10 + k, guides=1)
        out.append((predictions, motion, guide_list[0][0]))
    return out


def _chain(frames, alpha=0.8, gamma=1.0, tolerance=0.25, restart=()):
    """the reference over the sequence: frame 0 (and every frame of `restart`) passes through; -> [{name: out}], [{name: result or None}]"""
    outs, results = [], []
    for k, (predictions, motion, guide) in enumerate(frames):
        if k == 0 or k in restart:
            outs.append(dict(predictions))
            results.append({n: None for n in predictions})
            continue
        names = list(predictions)
        r = R.stabilize([(predictions[n], outs[-1][n]) for n in names], motion, -1.0, 1.0, alpha, gamma, [(guide, frames[k - 1][2], tolerance)])
        outs.append({n: r[i]["out"] for i, n in enumerate(names)})
        results.append(dict(zip(names, r)))
    return outs, results


def _device_frame(frame):
    predictions, motion, guide = frame
    wide = _frame(predictions["prediction/Depth"], "view")                           # the 1-channel pass as the Predictor hands it over: a view
    return ({"prediction/A": torch.from_numpy(predictions["prediction/A"]).cuda(), "prediction/Depth": wide}, torch.from_numpy(motion).cuda(),
            {"Normal": torch.from_numpy(guide).cuda()})


def _check_frame(stable, report, want_out, want_result, frame):
    for n, current in frame[0].items():
        have = stable[n].cpu().numpy()
        if want_result[n] is None:
            assert np.array_equal(have.view(np.uint32), current.view(np.uint32)), n
            assert report[n] == dict({k: 0 for k in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended", "values_clamped")},
                                     change=None, flicker_before=None, flicker_after=None)
            continue
        w = want_result[n]
        assert np.abs(have.astype(np.float64) - want_out[n]).max() <= TOL * (1.0 + np.abs(want_out[n]).max()), n
        assert np.allclose(have, want_out[n], rtol=TOL, atol=TOL), n
        for k in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended"):
            assert report[n][k] == w[k], (n, k)
        values = w["pixels_blended"] * current.shape[2]
        for k in ("change", "flicker_before", "flicker_after"):
            assert abs(report[n][k] - w[k] / values) <= 1e-4 * w[k] / values, (n, k)      # (the history is the device's own: 1e-6 away from the chain's)


def test_stabilizer_over_three_frames_and_its_resets(lib):
    _need_gpu()
    from deepdenoiser_amd.temporal import TemporalStabilizer
    frames = _sequence(33, 37, 5, seed=7)
    want_outs, want_results = _chain(frames, restart=(3,))
    stabilizer = TemporalStabilizer("cuda", guides=(("Normal", 0.25),))
    assert stabilizer.parameters() == {"alpha": 0.8, "gamma": 1.0, "motion_scale": [-1.0, 1.0], "guides": [["Normal", 0.25]]}
    launches = []
    for k, frame in enumerate(frames):
        if k == 3:
            stabilizer.reset()
        predictions, motion, guides = _device_frame(frame)
        stable = stabilizer.stabilize(predictions, motion, guides)
        launches.append(stabilizer.launches)
        assert list(stable) == list(predictions) and all(tuple(stable[n].shape) == tuple(predictions[n].shape) for n in stable)
        _check_frame(stable, stabilizer.report(), want_outs[k], want_results[k], frame)
    assert launches == [0, 1, 2, 2, 3]                                              # the first frame and the one after reset(): no launch
    # a size change resets: the frame passes through and becomes the history of the next
    small = _sequence(17, 20, 2, seed=9)
    small_outs, small_results = _chain(small)
    for k, frame in enumerate(small):
        predictions, motion, guides = _device_frame(frame)
        stable = stabilizer.stabilize(predictions, motion, guides)
        _check_frame(stable, stabilizer.report(), small_outs[k], small_results[k], frame)
    assert stabilizer.launches == 4
    # a changed key set resets too
    predictions, motion, guides = _device_frame(small[1])
    only = {"prediction/A": predictions["prediction/A"]}
    stable = stabilizer.stabilize(only, motion, guides)
    assert stabilizer.launches == 4 and torch.equal(stable["prediction/A"], only["prediction/A"])
    # what it refuses
    with pytest.raises(ValueError):
        stabilizer.stabilize(only, motion.cpu(), guides)
    with pytest.raises(ValueError):
        stabilizer.stabilize(only, motion[..., :1], guides)
    with pytest.raises(ValueError):
        stabilizer.stabilize(only, motion, {})
    with pytest.raises(ValueError):
        stabilizer.stabilize({"prediction/A": predictions["prediction/A"].double()}, motion, guides)
    with pytest.raises(ValueError):
        stabilizer.stabilize({"prediction/A": predictions["prediction/A"][:, ::2]}, motion, guides)
    for bad in (dict(alpha=1.5), dict(gamma=-1.0), dict(motion_scale=(1.0, float("nan"))), dict(guides=[("Normal", -1.0)]), dict(guides=[("N", 1.0)] * 5)):
        with pytest.raises(ValueError):
            TemporalStabilizer("cuda", **bad)


# ---------------------------------------------------------------------------------------------------- command line
FH, FW, T, O = 40, 56, 32, 4


def _run_main(tmp_path, extra):
    from deepdenoiser_amd import predict
    predict.main(predict.parser().parse_args([str(tmp_path / "architecture.json"), "--tile_size", str(T), "--tile_overlap_size", str(O), "--dtype", "f32"] + extra))


def test_predict_sequence_and_temporal_end_to_end(tmp_path, capsys):
    _need_gpu()
    import frames_util
    from deepdenoiser_amd import configs, openexr, tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import _COMBINED, _SINGLES, Predictor
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(FH, FW)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    loaded = [f.name for f in arch.feature_predictions + arch.auxiliary_features if f.load_data]
    members = [f.name for f in arch.feature_predictions if f.is_target and f.load_data]
    assert "Normal" in loaded and "Motion Vector" not in loaded
    rng = np.random.default_rng(5)
    names = ["f2", "f10", "f1"]                                                     # written in this order; denoised as f1, f2, f10
    order = ["f1", "f2", "f10"]
    motions, normals = {}, {}
    roots = {kind: tmp_path / kind for kind in ("single", "plain", "alpha0", "temporal")}
    for name in names:
        frames_util.write_rendering(str(roots["single"] / name), loaded, FH, FW, rng)
        _, _, motions[name], guide_list = R.make_case(FH, FW, [3], seed=len(motions) + 40, guides=1)
        normals[name] = guide_list[0][0]
        openexr.write_image(str(roots["single"] / name / "render_Normal_0001.exr"), normals[name])
        for kind in ("plain", "alpha0", "temporal"):
            os.makedirs(roots[kind] / name)
            for n in os.listdir(roots["single"] / name):
                with open(roots["single"] / name / n, "rb") as f, open(roots[kind] / name / n, "wb") as g:
                    g.write(f.read())
            if kind != "plain":
                openexr.write_image(str(roots[kind] / name / "render_Motion Vector_0001.exr"), motions[name])
    inputs = set(os.listdir(roots["single"] / "f1"))
    for name in order:
        _run_main(tmp_path, ["--input", str(roots["single"] / name)])
    written = sorted(set(os.listdir(roots["single"] / "f1")) - inputs)
    assert "Combined.npy" in written and all(m + ".npy" in written for m in members)
    # --input_sequence alone: the bytes of three --input runs
    _run_main(tmp_path, ["--input_sequence", str(roots["plain"])])
    assert not os.path.exists(roots["plain"] / "temporal.json")
    for name in order:
        assert sorted(set(os.listdir(roots["plain"] / name)) - inputs) == written
        for n in written:
            assert open(roots["plain"] / name / n, "rb").read() == open(roots["single"] / name / n, "rb").read(), (name, n)
    # --temporal --temporal_alpha 0: the same values
    _run_main(tmp_path, ["--input_sequence", str(roots["alpha0"]), "--temporal", "--temporal_alpha", "0"])
    for name in order:
        for n in written:
            assert np.array_equal(np.load(roots["alpha0"] / name / n), np.load(roots["single"] / name / n)), (name, n)
    # --temporal at the defaults, with one guide
    capsys.readouterr()
    _run_main(tmp_path, ["--input_sequence", str(roots["temporal"]), "--temporal", "--temporal_guide", "Normal:0.25"])
    printed = capsys.readouterr().out
    document = json.load(open(roots["temporal"] / "temporal.json"))
    assert (document["alpha"], document["gamma"], document["motion_scale"], document["guides"]) == (0.8, 1.0, [-1.0, 1.0], [["Normal", 0.25]])
    assert [f["directory"] for f in document["frames"]] == order
    single = {name: {m: np.load(roots["single"] / name / (m + ".npy")) for m in members} for name in order}
    history = single["f1"]
    for k, name in enumerate(order):
        have = {n[:-4]: np.load(roots["temporal"] / name / n) for n in written}
        report = document["frames"][k]["passes"]
        assert list(report) == ["prediction/" + m for m in members] and str(roots["temporal"] / name) in printed
        if k == 0:
            for m in members:
                assert np.array_equal(have[m], single[name][m]), m                  # the first frame is unchanged
                assert report["prediction/" + m]["pixels_blended"] == 0 and report["prediction/" + m]["flicker_before"] is None
        else:
            want = R.stabilize([(single[name][m], history[m]) for m in members], motions[name], -1.0, 1.0, 0.8, 1.0,
                               [(normals[name], normals[order[k - 1]], 0.25)])
            for w, m in zip(want, members):
                assert np.allclose(have[m], w["out"], rtol=TOL, atol=TOL), (name, m)
                r = report["prediction/" + m]
                assert [r[c] for c in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended")] == \
                    [w[c] for c in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended")], (name, m)
                assert r["pixels_blended"] > FH * FW // 4 and r["flicker_after"] <= r["flicker_before"], (name, m)
            history = {m: w["out"] for w, m in zip(want, members)}
            assert not np.array_equal(have["Combined"], np.load(roots["single"] / name / "Combined.npy"))
        # what is written stays consistent with its parts
        f64 = {n: v.astype(np.float64) for n, v in have.items()}
        image = sum(f64[c + " Color"] * (f64[c + " Direct"] + f64[c + " Indirect"]) for c in _COMBINED) + sum(f64[s] for s in _SINGLES)
        scale = sum(np.abs(f64[c + " Color"]) * (np.abs(f64[c + " Direct"]) + np.abs(f64[c + " Indirect"])) for c in _COMBINED) + sum(np.abs(f64[s]) for s in _SINGLES)
        assert (np.abs(f64["Combined"] - image) <= 1e-5 * scale + 1e-7).all(), name           # (fp32 sums of about twenty terms)
        for c in _COMBINED:
            assert np.allclose(f64[c], f64[c + " Color"] * (f64[c + " Direct"] + f64[c + " Indirect"]), rtol=1e-5, atol=1e-7), (name, c)
    # a frame without its Motion Vector file
    os.remove(roots["temporal"] / "f2" / "render_Motion Vector_0001.exr")
    with pytest.raises(openexr.ExrError) as e:
        _run_main(tmp_path, ["--input_sequence", str(roots["temporal"]), "--temporal"])
    assert str(roots["temporal"] / "f2") in str(e.value) and "Motion Vector" in str(e.value)
