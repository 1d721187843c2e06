"""-m gpu: dd_frame_quality through the C-ABI and quality.FrameQuality against tests/quality_ref.py, and `predict --target` end to end.

Inputs are seeded radiances with a wide dynamic range (quality_ref.radiance_pair).  Every image lies between guard floats inside a buffer
whose unused channels (ld > C) and guards are NaN: a read of either would make the pixel invalid and show in the counts.  Every SSIM map
lies between guard floats of a sentinel value that must come back untouched.

Gates.  The integer fields (pixels_valid, windows_valid, ldr_sq_err) and max_abs must be EQUAL: that is what catches a dropped, duplicated or
halo-shifted pixel.  The four scene-referred sums and the SSIM sum are compared with the float64 reference at the project's fp32 gate for a
loss, 1e-4 relative (tests/test_gpu_msssim.py); the SSIM map by rel-L2 at the same 1e-4, NaN positions identical.  Every comparison goes
through gpu_util.gate / check and lands in the parity file."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import quality_ref as R
from deepdenoiser_amd import _lib, configs, openexr, quality
from deepdenoiser_amd import metrics as M
from gpu_util import check, gate

pytestmark = pytest.mark.gpu

THR = M.preview_thresholds()
TH = TW = quality.TILE                        # the kernel's own output tile
GATE = 1e-4
GUARD = 64
MAP_SENTINEL = -7.25
SUMS = ("se", "ae", "rse", "smape", "ssim_sum")
INTEGERS = ("pixels_valid", "windows_valid", "ldr_sq_err")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Pair:
    """One (prediction, target) pair of a launch: fp32 [H,W,C] arrays and the leading dimensions they are stored with."""

    def __init__(self, pred, target, pred_ld=None, target_ld=None, want_map=True):
        self.pred, self.target = pred, target
        self.C = pred.shape[2]
        self.pred_ld, self.target_ld, self.want_map = pred_ld or self.C, target_ld or self.C, want_map

    _refs = {}

    def reference(self, exposure=1.0):
        """computed once per (arrays, exposure) and shared (never modified)"""
        key = (id(self.pred), id(self.target), exposure)
        if key not in Pair._refs:
            Pair._refs[key] = (R.record(self.pred, self.target, THR, exposure), self.pred, self.target)      # (the arrays are kept alive: ids stay unique)
        return Pair._refs[key][0]


_inputs = {}


def radiance(H, W, C, seed):
    key = (H, W, C, seed)
    if key not in _inputs:
        _inputs[key] = R.radiance_pair(H, W, C, seed)
    return _inputs[key]


def _device_image(a, ld):
    """[H,W,C] -> (device buffer with NaN guards and NaN in the channels past C, data pointer of the image)"""
    H, W, Cn = a.shape
    buf = np.full(GUARD + H * W * ld + GUARD, np.nan, dtype=np.float32)
    buf[GUARD:GUARD + H * W * ld].reshape(H, W, ld)[..., :Cn] = a
    dev = torch.from_numpy(buf).cuda()
    return dev, dev.data_ptr() + 4 * GUARD


def launch(lib, pairs, exposure=1.0, epsilon=R.EPSILON, maps=True):
    """One dd_frame_quality call -> (list of record dicts, the raw record bytes per pair, the maps (None where not asked for))."""
    H, W = pairs[0].pred.shape[:2]
    n = len(pairs)
    table = (_lib.QualityPair * n)()
    keep = []
    for i, p in enumerate(pairs):
        dp, pp = _device_image(p.pred, p.pred_ld)
        dt, tp = _device_image(p.target, p.target_ld)
        keep += [dp, dt]
        table[i] = _lib.QualityPair(pp, tp, p.pred_ld, p.target_ld, p.C)
    nbytes = lib.dd_frame_quality_scratch_bytes(n, H, W)
    assert nbytes > 0
    scratch = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")
    rec_bytes = ctypes.sizeof(_lib.QualityRecord)
    records = torch.full(((n + 2) * rec_bytes,), 0xAB, dtype=torch.uint8, device="cuda")      # a guard record either side
    thr = torch.from_numpy(THR).cuda()
    mh, mw = max(H - 10, 0), max(W - 10, 0)
    map_bufs = [torch.full((GUARD + mh * mw + GUARD,), MAP_SENTINEL, dtype=torch.float32, device="cuda") for _ in pairs]
    ptrs = None
    if maps:
        ptrs = (ctypes.c_void_p * n)(*[(b.data_ptr() + 4 * GUARD) if p.want_map else None for b, p in zip(map_bufs, pairs)])
    _lib.check(lib.dd_frame_quality(table, n, H, W, thr.data_ptr(), exposure, epsilon, ptrs, records.data_ptr() + rec_bytes, scratch.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw = records.cpu().numpy()
    assert (raw[:rec_bytes] == 0xAB).all() and (raw[(n + 1) * rec_bytes:] == 0xAB).all(), "bytes outside the records were written"
    recs = (_lib.QualityRecord * n).from_buffer_copy(raw[rec_bytes:(n + 1) * rec_bytes].tobytes())
    out, out_maps = [], []
    for i, p in enumerate(pairs):
        out.append({k: getattr(recs[i], k) for k in INTEGERS + SUMS + ("max_abs", "reserved")})
        m = map_bufs[i].cpu().numpy()
        assert (m[:GUARD] == MAP_SENTINEL).all() and (m[GUARD + mh * mw:] == MAP_SENTINEL).all(), "guard floats around map %d were written" % i
        body = m[GUARD:GUARD + mh * mw].reshape(mh, mw)
        if maps and p.want_map and mh and mw:
            out_maps.append(body)
        else:
            assert (body == MAP_SENTINEL).all(), "map %d was not asked for but written" % i
            out_maps.append(None)
    return out, [raw[(i + 1) * rec_bytes:(i + 2) * rec_bytes].tobytes() for i in range(n)], out_maps


def compare(tag, got, want, got_map=None):
    for k in INTEGERS:
        assert got[k] == want[k], "%s %s: %d != %d" % (tag, k, got[k], want[k])
    assert got["max_abs"] == want["max_abs"], "%s max_abs: %r != %r" % (tag, got["max_abs"], want["max_abs"])
    assert got["reserved"] == 0.0
    for k in SUMS:
        if want[k] == 0.0:
            assert got[k] == 0.0, (tag, k, got[k])
        else:
            gate("%s %s" % (tag, k), abs(got[k] - want[k]) / abs(want[k]), GATE)
    if got_map is not None:
        wm = want["map"]
        assert wm is not None and got_map.shape == wm.shape
        nan = np.isnan(wm)
        assert np.array_equal(np.isnan(got_map), nan), tag + ": NaN positions of the map"
        if (~nan).any():
            check(tag + " ssim map", torch.from_numpy(got_map[~nan]), torch.from_numpy(wm[~nan]), GATE)


def _pairs_of(H, W, specs):
    return [Pair(*radiance(H, W, C, seed), pred_ld=pld, target_ld=tld) for C, pld, tld, seed in specs]


SHAPES = [
    ("11x11_one_window", 11, 11, [(3, 3, 3, 1)]),
    ("10x64_no_window", 10, 64, [(3, 3, 3, 2), (1, 1, 1, 3)]),
    ("12x75", 12, 75, [(3, 3, 3, 4)]),
    ("45x77_C3", 45, 77, [(3, 3, 3, 5)]),
    ("64x64_C1_ld3", 64, 64, [(1, 3, 3, 6)]),
    ("33x130_three_mixed", 33, 130, [(3, 3, 3, 7), (1, 3, 1, 8), (3, 4, 3, 9)]),
    ("one_tile", TH + 10, TW + 10, [(3, 3, 3, 10)]),
    ("tile_plus_11_by_plus_9", TH + 11, TW + 9, [(3, 3, 3, 11), (1, 1, 2, 12)]),
    ("two_tiles_and_a_row", 2 * TH + 10 + 1, TW + 10 - 1, [(3, 3, 3, 13)]),
    ("257_tiles", 11, 8193, [(3, 3, 3, 30), (1, 3, 1, 31)]),      # the second round of the finalize kernel's strided add
]


@pytest.mark.parametrize("name,H,W,specs", SHAPES, ids=[s[0] for s in SHAPES])
def test_records_and_maps_match_the_reference(lib, name, H, W, specs):
    _need_gpu()
    pairs = _pairs_of(H, W, specs)
    got, _, maps = launch(lib, pairs)
    for i, p in enumerate(pairs):
        want = p.reference()
        compare("%s pair %d" % (name, i), got[i], want, maps[i])
        assert want["pixels_valid"] == H * W and want["windows_valid"] == max(H - 10, 0) * max(W - 10, 0)
        if H < 11 or W < 11:
            assert got[i]["windows_valid"] == 0 and got[i]["ssim_sum"] == 0.0 and maps[i] is None
            assert quality.figures(_as_record(got[i]), H, W, p.C)["ssim"] is None
    # the same pairs without any map: the same records, no map buffer touched (launch() asserts that)
    again, _, none = launch(lib, pairs, maps=False)
    assert all(m is None for m in none)
    for a, b in zip(again, got):
        assert a == b


def _as_record(d):
    r = _lib.QualityRecord()
    for k, v in d.items():
        setattr(r, k, v)
    return r


def test_a_map_that_is_not_asked_for_is_not_written(lib):
    _need_gpu()
    H, W = 33, 130
    pairs = _pairs_of(H, W, [(3, 3, 3, 7), (1, 3, 1, 8), (3, 4, 3, 9)])
    pairs[1].want_map = False
    got, _, maps = launch(lib, pairs)
    assert maps[0] is not None and maps[1] is None and maps[2] is not None
    for i, p in enumerate(pairs):
        compare("33x130 map %d" % i, got[i], p.reference(), maps[i])


def test_25_pairs_of_270x480(lib):
    """Many workgroups per pair (9 x 15 tiles) and 25 pairs in the launch: the sum across workgroups.  The 25 pairs are five distinct ones (one of
    them 1-channel, one with ld 4), each at five places of the table: the float64 reference is computed five times, not 25."""
    _need_gpu()
    H, W = 270, 480
    distinct = _pairs_of(H, W, [(3, 3, 3, 20), (1, 3, 3, 21), (3, 4, 3, 22), (3, 3, 3, 23), (1, 1, 1, 24)])
    order = [(7 * i + 3) % 5 for i in range(25)]
    got, raw, maps = launch(lib, [distinct[k] for k in order])
    first = {}
    for i, k in enumerate(order):
        if k not in first:
            first[k] = i
            compare("270x480 pair %d" % k, got[i], distinct[k].reference(), maps[i])
        else:
            assert raw[i] == raw[first[k]] and np.array_equal(maps[i], maps[first[k]], equal_nan=True), (i, k)


def test_flat_bright_region(lib):
    """A target of constant 0.9 and a prediction within +-1 byte of it: mu^2 is ~0.8 and the variance ~1e-5, the case in which E[x^2] - mu^2
    formed in fp32 would lose the window's variance."""
    _need_gpu()
    p, t = R.flat_bright_pair(45, 77, 3, 31, THR)
    p1, t1 = R.flat_bright_pair(45, 77, 1, 32, THR)
    pairs = [Pair(p, t), Pair(p1, t1, pred_ld=3)]
    got, _, maps = launch(lib, pairs)
    for i, pair in enumerate(pairs):
        want = pair.reference()
        assert 0 < want["ldr_sq_err"] <= 45 * 77 * pair.C
        compare("flat bright %d" % i, got[i], want, maps[i])


def test_identical_images(lib):
    _need_gpu()
    p, _ = radiance(45, 77, 3, 5)
    got, _, maps = launch(lib, [Pair(p, p.copy())])
    g = got[0]
    assert g["se"] == 0.0 and g["ae"] == 0.0 and g["rse"] == 0.0 and g["smape"] == 0.0 and g["max_abs"] == 0.0 and g["ldr_sq_err"] == 0
    assert g["pixels_valid"] == 45 * 77 and g["windows_valid"] == 35 * 67
    gate("identical images |1 - ssim|", abs(1.0 - g["ssim_sum"] / g["windows_valid"]), 1e-6)
    assert np.abs(maps[0] - 1.0).max() <= 1e-6
    f = quality.figures(_as_record(g), 45, 77, 3)
    assert f["mse"] == 0.0 and f["psnr_8bit"] == float("inf")


def test_non_finite_pixels(lib):
    _need_gpu()
    H, W = 45, 77
    p, t = (a.copy() for a in radiance(H, W, 3, 5))
    p[0, 0, :] = np.nan                       # a corner: one window
    t[H // 2, W // 2, 1] = np.inf             # the centre: 121 windows
    p[H - 1, W - 1, 2] = np.nan               # the last pixel, one channel only
    p1, t1 = (a.copy() for a in radiance(H, W, 1, 41))
    t1[3, 40, 0] = -np.inf
    bad_p, bad_t = (a.copy() for a in radiance(H, W, 3, 42))
    bad_p[...] = np.nan                       # every pixel invalid
    pairs = [Pair(p, t), Pair(p1, t1, pred_ld=3), Pair(bad_p, bad_t)]
    got, _, maps = launch(lib, pairs)
    want = pairs[0].reference()
    assert want["pixels_valid"] == H * W - 3 and want["windows_valid"] == 35 * 67 - 1 - 121 - 1
    for i in range(2):
        compare("non-finite %d" % i, got[i], pairs[i].reference(), maps[i])
    assert pairs[1].reference()["pixels_valid"] == H * W - 1
    g = got[2]
    assert all(g[k] == 0 for k in INTEGERS + SUMS) and g["max_abs"] == 0.0
    assert np.isnan(maps[2]).all()
    f = quality.figures(_as_record(g), H, W, 3)
    assert f["valid_pixels"] == 0 and f["valid_windows"] == 0 and f["pixels"] == H * W
    assert all(f[k] is None for k in ("mse", "mae", "rel_mse", "smape", "max_abs", "psnr_8bit", "ssim"))


def test_determinism_order_and_exposure(lib):
    _need_gpu()
    H, W = 33, 130
    pairs = _pairs_of(H, W, [(3, 3, 3, 7), (1, 3, 1, 8), (3, 4, 3, 9)])
    _, raw, maps = launch(lib, pairs)
    _, raw2, maps2 = launch(lib, pairs)
    assert raw == raw2 and all(np.array_equal(a, b) for a, b in zip(maps, maps2))
    perm = [2, 0, 1]
    _, raw3, maps3 = launch(lib, [pairs[k] for k in perm])
    assert [raw3[i] for i in range(3)] == [raw[k] for k in perm]
    assert all(np.array_equal(maps3[i], maps[k]) for i, k in enumerate(perm))
    _, alone, _ = launch(lib, [pairs[1]])
    assert alone[0] == raw[1]
    # exposure changes the display-referred fields alone
    got_e, raw_e, maps_e = launch(lib, pairs, exposure=0.37)
    scene = slice(24, 56)      # se, ae, rse, smape
    for i, p in enumerate(pairs):
        assert raw_e[i][:16] == raw[i][:16] and raw_e[i][scene] == raw[i][scene] and raw_e[i][64:] == raw[i][64:], i
        assert raw_e[i][16:24] != raw[i][16:24] and raw_e[i][56:64] != raw[i][56:64], i
        compare("exposure 0.37 pair %d" % i, got_e[i], p.reference(0.37), maps_e[i])


# ---------------------------------------------------------------------------------------------------- the host module
def test_frame_quality_measure():
    _need_gpu()
    H, W = 45, 77
    p3, t3 = radiance(H, W, 3, 5)
    p1, t1 = radiance(H, W, 1, 41)
    wide = torch.from_numpy(np.repeat(p1, 3, axis=2)).cuda()
    wide[..., 1:] = float("nan")                                     # a [..., :1] view of a 3-wide frame: the other channels are not looked at
    fq = quality.FrameQuality("cuda", exposure=1.5)
    predictions = {"prediction/A": torch.from_numpy(p3).cuda(), "prediction/Depth": wide[..., :1], "Combined": torch.from_numpy(p3)}
    targets = {"Combined": torch.from_numpy(t3).cuda(), "prediction/Depth": torch.from_numpy(t1), "prediction/A": t3, "unused": t3}
    result, maps = fq.measure(predictions, targets, ssim_maps=True)
    assert list(result) == list(predictions) and list(maps) == list(predictions)
    for name, (p, t) in {"prediction/A": (p3, t3), "prediction/Depth": (p1, t1), "Combined": (p3, t3)}.items():
        want = R.measure(p, t, THR, exposure=1.5)
        got = result[name]
        assert set(got) == set(want)
        for k in ("pixels", "valid_pixels", "windows", "valid_windows", "max_abs"):
            assert got[k] == want[k], (name, k)
        for k in ("mse", "mae", "rel_mse", "smape", "ssim"):
            gate("measure %s %s" % (name, k), abs(got[k] - want[k]) / abs(want[k]), GATE)
        assert abs(got["psnr_8bit"] - want["psnr_8bit"]) <= 1e-9 * want["psnr_8bit"]      # (an exact integer under one log10)
        assert tuple(maps[name].shape) == (H - 10, W - 10) and maps[name].is_cuda
    assert fq.measure(predictions, targets) == result                # the buffers of a frame size are reused
    assert len(fq._buffers) == 1
    with pytest.raises(ValueError, match="no target"):
        fq.measure({"nothing": p3}, targets)
    small = fq.measure({"a": p3[:10]}, {"a": t3[:10]}, ssim_maps=True)
    assert small[0]["a"]["ssim"] is None and small[1] == {}


# ---------------------------------------------------------------------------------------------------- predict --target
FH, FW, T, O = 40, 72, 32, 4


def _write_frames(tmp_path, arch, seed):
    """source and target .exr files of every loaded pass -> (source directory, target directory)"""
    rng = np.random.default_rng(seed)
    passes = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    src, tgt = tmp_path / "frame_0001_16_0_0", tmp_path / "frame_0001_target"
    src.mkdir()
    tgt.mkdir()
    for name, ch in passes.items():
        clean = rng.random((FH, FW, 3)).astype(np.float32)
        if ch == 1:
            clean[...] = clean[..., :1]
        noisy = (clean * (1.0 + 0.3 * rng.standard_normal(clean.shape))).astype(np.float32)
        if ch == 1:
            noisy[...] = noisy[..., :1]
        openexr.write_image(str(src / ("render_%s_0001.exr" % name)), noisy)
        openexr.write_image(str(tgt / ("target_%s_0001.exr" % name)), clean)
    return src, tgt


def _predict_setup(tmp_path, combined=None):
    from deepdenoiser_amd import tf_checkpoint
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.prediction import Predictor
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", combined=combined)
    aj["model_directory"] = "model"
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    arch = Architecture(aj, device="cuda", dtype="f32", seed=2)
    Predictor(arch, tile_size=T, tile_overlap_size=O).prepare(FH, FW)              # (creates the parameters)
    tf_checkpoint.save_variables(arch, str(tmp_path / "model"), global_step=1)
    return arch


def _main(tmp_path, src, extra):
    from deepdenoiser_amd import predict
    args = predict.parser().parse_args([str(tmp_path / "architecture.json"), "--input", str(src), "--tile_size", str(T), "--tile_overlap_size", str(O),
                                        "--dtype", "f32"] + extra)
    predict.main(args)


def test_predict_with_a_target_end_to_end(tmp_path, capsys):
    _need_gpu()
    from deepdenoiser_amd.summaries import decode_png
    arch = _predict_setup(tmp_path)
    src, tgt = _write_frames(tmp_path, arch, seed=5)
    names = quality.target_names(arch)
    assert "Combined" in names and "prediction/Diffuse" in names
    _main(tmp_path, src, ["--target", str(tgt), "--ssim_png", "--exposure", "0.8"])
    printed = capsys.readouterr().out
    document = json.load(open(src / "quality.json"))
    assert (document["tile_size"], document["tile_overlap_size"], document["dtype"], document["nonfinite"], document["exposure"]) == (T, O, "f32", "keep", 0.8)
    assert list(document["quality"]) == names
    # the figures are those of FrameQuality.measure on the written .npy files against the loaded targets ...
    targets = quality.targets_of_frame(str(tgt), arch)
    assert list(targets) == names
    written = {n: np.load(src / (n.split("/", 1)[-1] + ".npy")) for n in names}
    again = quality.FrameQuality("cuda", exposure=0.8).measure({n: torch.from_numpy(v) for n, v in written.items()}, targets)
    assert again == document["quality"]
    # ... and agree with the reference
    for n in names:
        short = n.split("/", 1)[-1]
        assert short in printed
        t = targets[n].cpu().numpy()
        want = R.measure(written[n], np.ascontiguousarray(t), THR, exposure=0.8)
        got = document["quality"][n]
        for k in ("pixels", "valid_pixels", "windows", "valid_windows", "max_abs"):
            assert got[k] == want[k], (n, k)
        for k in ("mse", "mae", "rel_mse", "smape", "ssim"):
            gate("predict --target %s %s" % (short, k), abs(got[k] - want[k]) / abs(want[k]), GATE)
        assert abs(got["psnr_8bit"] - want["psnr_8bit"]) <= 1e-9 * want["psnr_8bit"]
        png = decode_png(open(src / (short + "_ssim.png"), "rb").read())
        assert png.shape == (FH - 10, FW - 10, 3)
    with_target = {n: v.copy() for n, v in written.items()}
    # a second run without --target: no quality.json, the same .npy bits
    os.remove(src / "quality.json")
    for n in names:
        os.remove(src / (n.split("/", 1)[-1] + ".npy"))
    _main(tmp_path, src, [])
    assert not os.path.exists(src / "quality.json")
    for n in names:
        assert np.array_equal(np.load(src / (n.split("/", 1)[-1] + ".npy")).view(np.int32), with_target[n].view(np.int32)), n


def test_combined_is_scored_only_when_every_member_exists(tmp_path):
    _need_gpu()
    combined = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Transmission"}
    arch = _predict_setup(tmp_path, combined=combined)
    src, tgt = _write_frames(tmp_path, arch, seed=6)
    names = quality.target_names(arch)
    assert "Combined" not in names and "prediction/Diffuse" not in names and "prediction/Diffuse Color" in names
    _main(tmp_path, src, ["--target", str(tgt), "--quality_json", str(tmp_path / "q.json")])
    assert not os.path.exists(src / "quality.json")
    document = json.load(open(tmp_path / "q.json"))
    assert list(document["quality"]) == names == list(quality.targets_of_frame(str(tgt), arch))
    assert not [n for n in os.listdir(src) if n.endswith("_ssim.png")]


def test_compare_command_line(tmp_path, capsys):
    _need_gpu()
    from deepdenoiser_amd import compare
    p, t = radiance(45, 77, 3, 5)
    openexr.write_image(str(tmp_path / "a.exr"), p)
    np.save(tmp_path / "b.npy", t)
    result = compare.main(compare.parser().parse_args([str(tmp_path / "a.exr"), str(tmp_path / "b.npy"), "--exposure", "1.5"]))
    (got,) = result.values()
    want = R.measure(p, t, THR, exposure=1.5)
    for k in ("pixels", "valid_pixels", "windows", "valid_windows", "max_abs"):
        assert got[k] == want[k], k
    for k in ("mse", "mae", "rel_mse", "smape", "ssim"):
        gate("compare %s" % k, abs(got[k] - want[k]) / abs(want[k]), GATE)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 2 and "psnr_8bit" in out[0] and str(tmp_path / "a.exr") in out[1]
