"""-m gpu: data-set statistics reduced on the device (csrc/dd_frame_statistics.hip, deepdenoiser_amd/statistics.py).

Op level: the rows of dd_tile_statistics against tests/statistics_ref.rows_ref (numpy float64).  Minima, maxima, pivots, counts and mask sums
must be equal; the sums agree at rtol 1e-10: double arithmetic, at most 67 * 67 * 3 < 2^14 summands, the sequential-sum bound
n * 2^-53 ~ 2e-12 relative to sum |term|, and the shifted terms of the test data carry no cancellation beyond a factor 10 (asserted on the
reference sums: the data are ramps that grow away from the window's first sample, so x - K keeps its sign but for a few samples).

End to end: `python -m deepdenoiser_amd.statistics` (as a function call) on a tiny EXR tree against tests/statistics_ref.statistics_ref -- the
two-sweep reference without the :132 / :185 slip -- fed with the same tiles cut by numpy, at rtol 1e-9: the row tolerance 1e-10 times the
conditioning of the join on this data.  The join recovers sum (x - mean)^2 from sum (x - K)^2 - 2 (mean - K) sum (x - K) + n (mean - K)^2; with
frames_util's images (standard normal samples, |.| for radiance, so |x - K|, |mean - K| <= ~6 and a variance about the global mean of
order 1) the three terms are each below ~10 times the result, and means of windows are sums of values of order 1 with at most the same
cancellation: a factor 10 in all."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import frames_util as U
import statistics_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import openexr
from deepdenoiser_amd.naming import Naming

pytestmark = pytest.mark.gpu
F = {name: k for k, name in enumerate(L.STAT_FIELD_NAMES)}
EXACT = ("present", "min", "max", "min_log1p", "max_log1p", "pivot", "count", "mask_sum")
SUMS = ("sum", "sum_sq", "sum_log1p", "sum_sq_log1p", "masked_sum", "masked_sum_sq", "masked_sum_log1p", "masked_sum_sq_log1p")

# ---------------------------------------------------------------------------------------------------- op level
# planes 0 .. 3 are 70 x 90, planes 4 and 5 are 67 x 67.  The mask pass: zero everywhere in plane 2, in a part of planes 1 and 5, nowhere else.
SIZES = [(70, 90)] * 4 + [(67, 67)] * 2
PASSES = [("c1", 1, False, False), ("c3", 3, False, True), ("alpha", 1, True, False), ("absent", 3, False, True), ("big", 3, False, True)]
ABSENT_PLANE = 4
_PLANES = {}


def _ramp(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    return 1.0 + 0.05 * y + 0.03 * x + 0.01 * rng.standard_normal((h, w))


def _planes():
    """{pass: [host planes]} and the mask planes.  Made once, never modified."""
    if not _PLANES:
        rng = np.random.default_rng(23)
        out = {name: [] for name, *_ in PASSES}
        out["mask"] = []
        for p, (h, w) in enumerate(SIZES):
            out["c1"].append(_ramp(rng, h, w)[..., None].astype(np.float32))
            out["c3"].append(np.stack([-_ramp(rng, h, w), -2.0 * _ramp(rng, h, w), -3.0 * _ramp(rng, h, w)], axis=2).astype(np.float32))      # negative: sign(x) log1p(|x|)
            alpha = (10.0 - _ramp(rng, h, w))[..., None].astype(np.float32)      # falls away from a window's first sample, stays above 1
            alpha[rng.random((h, w)) < 0.3] = 1.0           # exact 1.0 and 0.0 samples: not covered, covered
            alpha[rng.random((h, w)) < 0.05] = 0.0
            out["alpha"].append(alpha)
            out["absent"].append(None if p == ABSENT_PLANE else np.stack([_ramp(rng, h, w)] * 3, axis=2).astype(np.float32))
            big = (1.0 + 0.01 * rng.standard_normal((h, w, 3))).astype(np.float32)
            big[0::3] = 1e10                                # a third of every window
            out["big"].append(big)
            mask = np.abs(rng.standard_normal((h, w, 3))).astype(np.float32) + 0.1
            if p == 2:
                mask[...] = 0.0
            elif p in (1, 5):
                mask[rng.random((h, w)) < 0.5] = 0.0
                mask[: h // 2, : w // 3] = 0.0
                mask[h // 2, w // 2] = (0.0, 0.0, 0.25)      # not zero in one channel only
            out["mask"].append(mask)
        _PLANES.update(out)
    return _PLANES


def _windows(T):
    """(plane, mask plane, y0, x0): origins 0, interior and (h - T, w - T) in both plane sizes, every kind of mask."""
    out = []
    for plane, masks in ((0, (1, 2, 3)), (3, (1,)), (4, (5,)), (5, (4,))):
        h, w = SIZES[plane]
        origins = [(0, 0), (h - T, w - T)] + ([(1, 2), ((h - T) // 2, w - T)] if h > T else [])
        out += [(plane, m, y0, x0) for m in masks for (y0, x0) in origins]
    return np.array(out, dtype=np.int32).reshape(-1, 4)


def _launch(lib, T, windows):
    planes = _planes()
    dev = {n: [None if p is None else torch.from_numpy(p).cuda() for p in ps] for n, ps in planes.items()}
    ptrs = {n: torch.tensor([0 if t is None else t.data_ptr() for t in ts], dtype=torch.int64).cuda() for n, ts in dev.items()}
    hw = torch.tensor(SIZES, dtype=torch.int32).cuda()
    desc = L.StatDesc()
    desc.n_passes, desc.n_planes, desc.plane_hw = len(PASSES), len(SIZES), hw.data_ptr()
    for en, (name, ch, is_alpha, masked) in zip(desc.pass_, PASSES):
        en.planes, en.mask_planes, en.C, en.is_alpha = ptrs[name].data_ptr(), (ptrs["mask"].data_ptr() if masked else None), ch, int(is_alpha)
    table = torch.from_numpy(np.ascontiguousarray(windows)).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((len(windows), len(PASSES), L.STAT_FIELDS), -7.5, dtype=torch.float64, device="cuda")
        L.check(lib.dd_tile_statistics(ctypes.byref(desc), table.data_ptr(), len(windows), T, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.parametrize("T", [5, 32, 67])      # no multiple of a wave; one row of waves (32 * 32 = 4 pixels per thread); odd and larger
def test_rows_match_numpy_float64_and_repeat(lib, T):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    planes, windows = _planes(), _windows(T)
    assert (windows[:, 2] > 0).any() and (windows[:, 2] == 0).any() and len({(p, m) for p, m, _, _ in windows.tolist()}) == 6
    first, second = _launch(lib, T, windows)
    assert first.tobytes() == second.tobytes()                 # repeatability: two launches, the same bytes
    have = first
    worst = {}
    mismatches = []
    for n, (plane, mplane, y0, x0) in enumerate(windows.tolist()):
        cut = (slice(y0, y0 + T), slice(x0, x0 + T))
        for k, (name, ch, is_alpha, masked) in enumerate(PASSES):
            frame = planes[name][plane]
            want = R.rows_ref(None if frame is None else frame[cut], planes["mask"][mplane][cut] if masked else None, is_alpha, L.STAT_FIELD_NAMES)
            row = have[n, k]
            if frame is None:
                assert plane == ABSENT_PLANE and name == "absent" and (row == 0).all()
                continue
            for key in EXACT:
                if row[F[key]] != want[F[key]]:
                    mismatches.append((n, name, key, float(row[F[key]]), float(want[F[key]])))
            if masked:      # the three kinds of mask
                assert want[F["mask_sum"]] == {1: want[F["mask_sum"]], 2: 0, 3: T * T, 4: T * T, 5: want[F["mask_sum"]]}[mplane]
                assert mplane not in (1, 5) or 0 < want[F["mask_sum"]] < T * T or T == 5
            for key in SUMS + ("pivot_log1p",):
                u, v = row[F[key]], want[F[key]]
                err = abs(u - v) / abs(v) if v != 0 else (0.0 if u == 0 else np.inf)
                worst[key] = max(worst.get(key, 0.0), err)
    print("T=%d: %d windows x %d passes; worst relative error of the sums: %s" % (T, len(windows), len(PASSES),
                                                                               ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    print("T=%d: %d mismatches among the exact fields%s" % (T, len(mismatches), "".join("\n  %r" % (m,) for m in mismatches[:12])))
    assert not mismatches
    assert max(worst.values()) <= 1e-10, worst


def test_test_data_carry_no_cancellation_beyond_a_factor_10():
    """The premise of the rtol above, on the reference side (no device): sum |term| <= 10 |sum term| for every compared sum."""
    planes = _planes()
    for T in (5, 32, 67):
        for plane, mplane, y0, x0 in _windows(T).tolist():
            cut = (slice(y0, y0 + T), slice(x0, x0 + T))
            for name, ch, is_alpha, masked in PASSES:
                if planes[name][plane] is None:
                    continue
                x = planes[name][plane][cut].astype(np.float64)
                m = R.non_zero_mask(planes["mask"][mplane][cut].astype(np.float64))[:, :, None] if masked else np.zeros((T, T, 1))
                for values in (x, R.signed_log1p(x)):
                    d = values - values.reshape(-1)[0]
                    for terms in (d, d * m):
                        assert np.abs(terms).sum() <= 10.0 * abs(terms.sum()) or not terms.any(), (T, plane, mplane, y0, x0, name)


# ---------------------------------------------------------------------------------------------------- end to end
T2, SPPS, BEST, S2 = 8, [4, 16], 64, 2
SOURCE = ["Alpha", "Depth", "Normal", "Diffuse Color", "Diffuse Direct", "Glossy Indirect", "Volume Direct"]
TARGET = ["Alpha", "Depth", "Diffuse Color", "Diffuse Direct", "Glossy Indirect", "Volume Direct"]
SCENES = (("scene_a", 24, 40), ("scene_b", 16, 16))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Two scenes (24 x 40 and 16 x 16) and one with a NaN sample, as EXR renderings: spp 4 and 16 twice each, spp 64 once.  In scene_a the
    target colour passes the masks come from are black in the first grid tile and in the upper half of the second."""
    root = str(tmp_path_factory.mktemp("statistics_e2e"))
    rng = np.random.default_rng(7)
    written = {}
    for name, h, w in SCENES + (("scene_nan", 24, 40),):
        written[name] = U.write_scene(root, name, SPPS, SOURCE, TARGET, h, w, rng, sources=S2, target_spp=BEST)
    for color in ("Diffuse Color", "Glossy Indirect"):
        img = written["scene_a"][(BEST, 0)][color]
        img[:T2, :T2] = 0.0
        img[: T2 // 2, T2:2 * T2] = 0.0
        openexr.write_image(os.path.join(root, "OpenEXR", "scene_a", U.rendering_name("scene_a", BEST, 0), "render_%s_0001.exr" % color), img)
    bad = U.image(rng, 24, 40, "Normal")
    bad[3, 5, 2] = np.nan
    nan_path = os.path.join(root, "OpenEXR", "scene_nan", U.rendering_name("scene_nan", 16, 1), "render_Normal_0001.exr")
    openexr.write_image(nan_path, bad)
    names = ["scene_a", "scene_nan", "scene_b"]
    paths = {}
    for group in (False, True):
        path = U.write_json(root, {"training": names, "validation": names[:1]}, T2, SPPS, S2, SOURCE, TARGET, target_spp=BEST,
                            name="tfrecords_%d.json" % group)
        j = json.load(open(path))
        j["modes"]["training"]["group_by_samples_per_pixel"] = group
        j["base_tfrecords_directory"] = "TFRecords_%d" % group
        json.dump(j, open(path, "w"))
        paths[group] = path
    tiles = []
    for name, h, w in SCENES:
        for i in range(h // T2):
            for j in range(w // T2):
                cut = (slice(i * T2, (i + 1) * T2), slice(j * T2, (j + 1) * T2))
                tiles.append(({Naming.source_feature_name(p, samples_per_pixel=spp, index=k): written[name][(spp, k)][p][cut]
                               for spp in SPPS for k in range(S2) for p in SOURCE},
                              {Naming.target_feature_name(p): written[name][(BEST, 0)][p][cut] for p in TARGET}))
    return {"root": root, "json": paths, "tiles": tiles, "nan_path": nan_path}


def _run(dataset, group, extra=()):
    from deepdenoiser_amd import statistics
    lines = []
    args = statistics.parser().parse_args([dataset["json"][group], "--mode", "training", "--threads", "2"] + list(extra))
    written = statistics.main(args, log=lines.append)
    return written, lines


@pytest.mark.parametrize("group", [False, True])
def test_statistics_cli_matches_the_reference(dataset, group):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    written, lines = _run(dataset, group)
    base = os.path.join(dataset["root"], "TFRecords_%d" % group)
    names = ["training_statistics_%d.json" % s for s in SPPS] if group else ["training_statistics.json"]
    assert written == [os.path.join(base, n) for n in names]
    assert len(dataset["tiles"]) == 3 * 5 + 2 * 2
    for path, spps in zip(written, [[s] for s in SPPS] if group else [SPPS]):
        have = json.load(open(path))
        want = R.statistics_ref(dataset["tiles"], SOURCE, TARGET, spps, S2, target_from_last_source=False)
        assert sorted(have) == sorted(want)
        bad = R.entries_differ(have, want, 1e-9)
        for name in bad:
            print(name, have[name], want[name])
        assert bad == []
        assert open(path).read() == json.dumps(have, sort_keys=True, indent=2)
        masked = have[Naming.source_feature_name("Diffuse Direct", masked=True)]["statistics"]
        assert 0 < masked["coverage"] and masked["mean"] > 0      # the black tile contributes nothing, the others do
    # the scene with the NaN sample is skipped with the line FrameBank prints
    nan_dir = os.path.join(dataset["root"], "OpenEXR", "scene_nan")
    assert "frames: %s skipped: there is at least one value in %s which is not finite" % (nan_dir, dataset["nan_path"]) in lines
    # one table line per entry
    assert sum(line.startswith(("source_image/", "target_image/")) for line in lines) == len(names) * len(have)


def test_one_scene_per_chunk_gives_the_same_bytes(dataset):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    whole, _ = _run(dataset, False, ["--output", os.path.join(dataset["root"], "whole")])
    per_pixel = 4 * (len(SPPS) * S2 * 17 + 14)                  # the source passes hold 17 channels, the target passes 14
    limit = 24 * 40 * per_pixel                                 # a 24 x 40 scene fits, no two scenes together do
    from deepdenoiser_amd import statistics
    chunks = statistics.chunk_scenes([type("Scene", (), {"height": h, "width": w}) for h, w in ((24, 40), (24, 40), (16, 16))], per_pixel, limit)
    assert [len(c) for c in chunks] == [1, 1, 1]
    parts, lines = _run(dataset, False, ["--output", os.path.join(dataset["root"], "parts"), "--frame_memory_gb", repr(limit / 2 ** 30)])
    assert open(parts[0], "rb").read() == open(whole[0], "rb").read()
    assert any("scene_nan skipped" in line for line in lines)
