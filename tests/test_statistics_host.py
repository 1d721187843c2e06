"""The host side of deepdenoiser_amd/statistics.py without a device: the join fed with rows that numpy computes in the kernel's layout
(tests/statistics_ref.rows_ref), window enumeration, chunking, file names and JSON shape.

Tolerance of the join against the two-sweep reference (tests/statistics_ref.statistics_ref, float64, no shifted sums): rtol 1e-10.  Both
sides are float64; a window has at most 6 * 6 * 3 = 108 samples (n * 2^-53 ~ 1e-14 per sum), and the identity
sum (x - mean)^2 = sum (x - K)^2 - 2 (mean - K) sum (x - K) + n (mean - K)^2 cancels by at most
(|x - K| + |mean - K|)^2 / (x - mean)^2 summed over a window, which for these data -- values of order 1, or 1e10 in a third of the samples with
a mean of order 1e9..1e10 -- stays below 1e3: 1e-14 * 1e3 = 1e-11."""
import json
import os
import types

import numpy as np
import pytest

import statistics_ref as R
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import statistics as S
from deepdenoiser_amd.naming import Naming
from deepdenoiser_amd.render_passes import RenderPasses

RTOL = 1e-10
HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "statistics_golden.json")) as f:
    CASES = {c["name"]: c for c in json.load(f)["cases"]}


def frame_set_of(case, scenes=()):
    return types.SimpleNamespace(tile=case["tile"], number_of_sources_per_example=case["sources"], source_spps=list(case["spps"]),
                                 source_passes=list(case["source_passes"]), target_passes=list(case["target_passes"]), skipped=[], scenes=list(scenes))


def rows_of(stats, tiles):
    """The table the kernel would write for `tiles`, one scene of one tile each, in window_table's order."""
    rows, index = [], []
    for source, target in tiles:
        def mask_window(name):
            return target[Naming.target_feature_name(stats.mask_of[name])] if name in stats.mask_of else None
        for k, spp in enumerate(stats.spps):
            for i in range(stats.sources):
                rows.append([R.rows_ref(source.get(Naming.source_feature_name(p, samples_per_pixel=spp, index=i)), mask_window(p), p == "Alpha",
                                        L.STAT_FIELD_NAMES) for p in stats.passes])
                index.append(k)
        rows.append([R.rows_ref(target.get(Naming.target_feature_name(p)), mask_window(p), p == "Alpha", L.STAT_FIELD_NAMES) for p in stats.passes])
        index.append(S.TARGET)
    return np.asarray(rows), np.asarray(index)


def joined(case, tiles, group):
    stats = S.FrameStatistics(frame_set_of(case), group)
    rows, index = rows_of(stats, tiles)
    assert rows.shape == (len(tiles) * (len(case["spps"]) * case["sources"] + 1), len(stats.passes), L.STAT_FIELDS)
    stats.add_rows([rows], [index])
    return stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_join_equals_the_two_sweep_reference(name):
    case = CASES[name]
    tiles = R.make_tiles(case)
    stats = joined(case, tiles, case["group"])
    results = stats.results()
    assert [spp for spp, _ in results] == (case["spps"] if case["group"] else [None])
    for spp, have in results:
        want = R.statistics_ref(tiles, case["source_passes"], case["target_passes"], case["spps"] if spp is None else [spp], case["sources"])
        assert sorted(have) == sorted(want)
        assert R.entries_differ(have, want, RTOL) == []
        # the same as the reference wrote, but for the entries of its :132 / :185 slip
        golden = case["results"]["all" if spp is None else str(spp)]
        assert R.entries_differ(have, golden, RTOL) == sorted(Naming.target_feature_name(p) for p in case["target_passes"])


def test_join_with_a_pass_offset_by_1e10_in_part_of_a_tile():
    """Depth already holds 1e10 in a part of every tile; here a MASKED pass does too, the pivot (the first sample) included."""
    case = CASES["ungrouped"]
    tiles = R.make_tiles(case)
    T = case["tile"]
    for key in (Naming.source_feature_name("Diffuse Direct", samples_per_pixel=4, index=1), Naming.source_feature_name("Normal", samples_per_pixel=16, index=0)):
        tiles[0][0][key][:T // 3] += np.float32(1e10)
    tiles[2][1][Naming.target_feature_name("Glossy Indirect")][T // 2:, : T // 2] += np.float32(1e10)
    have = joined(case, tiles, False).statistics()
    want = R.statistics_ref(tiles, case["source_passes"], case["target_passes"], case["spps"], case["sources"])
    assert have[Naming.source_feature_name("Diffuse Direct")]["statistics"]["maximum"] >= 1e10
    assert have[Naming.source_feature_name("Diffuse Direct", masked=True)]["statistics"]["variance"] > 1e17
    assert R.entries_differ(have, want, RTOL) == []


def test_absent_rows_and_empty_lists():
    """A pass that is only a source has absent rows in the target windows; an entry whose windows are all black gives 0 (:148-149, :199-200)."""
    case = dict(CASES["grouped"], tiles=1, black_tile=0, partly_black_tile=-1)
    tiles = R.make_tiles(case)
    stats = joined(case, tiles, False)
    normal = stats.passes.index("Normal")
    assert (stats.rows[stats.spp_index == S.TARGET, normal, 0] == 0).all() and (stats.rows[stats.spp_index != S.TARGET, normal, 0] == 1).all()
    have = stats.statistics()
    entry = have[Naming.source_feature_name("Diffuse Direct", masked=True)]
    assert entry["statistics"]["mean"] == entry["statistics"]["variance"] == entry["statistics"]["coverage"] == 0.0
    assert entry["statistics_log1p"]["mean"] == entry["statistics_log1p"]["variance"] == 0.0
    assert np.isfinite(entry["statistics"]["minimum"]) and entry["statistics"]["maximum"] > 0
    assert R.entries_differ(have, R.statistics_ref(tiles, case["source_passes"], case["target_passes"], case["spps"], case["sources"]), RTOL) == []


def test_chunks_give_the_same_result_as_one_chunk():
    case = CASES["ungrouped"]
    tiles = R.make_tiles(case)
    whole = joined(case, tiles, False)
    parts = S.FrameStatistics(frame_set_of(case), False)
    for chunk in (tiles[:2], tiles[2:3], tiles[3:]):
        rows, index = rows_of(parts, chunk)
        parts.add_rows([rows], [index])
    assert np.array_equal(parts.rows, whole.rows) and np.array_equal(parts.spp_index, whole.spp_index)
    assert json.dumps(parts.statistics(), sort_keys=True) == json.dumps(whole.statistics(), sort_keys=True)


def test_chunk_scenes():
    scenes = [types.SimpleNamespace(height=h, width=w) for h, w in ((10, 10), (10, 20), (30, 10), (5, 5), (100, 100), (2, 2))]
    sizes = lambda chunks: [[s.height * s.width for s in c] for c in chunks]      # noqa: E731
    assert sizes(S.chunk_scenes(scenes, 4, None)) == [[100, 200, 300, 25, 10000, 4]]
    assert sizes(S.chunk_scenes(scenes, 4, 4 * 300)) == [[100, 200], [300], [25], [10000], [4]]      # (a scene over the limit stands alone)
    assert sizes(S.chunk_scenes(scenes, 4, 1)) == [[100], [200], [300], [25], [10000], [4]]
    assert sizes(S.chunk_scenes(scenes, 4, 4 * 20000)) == [[100, 200, 300, 25, 10000, 4]]
    assert S.chunk_scenes([], 4, None) == []


def test_window_enumeration_drops_remainders():
    T, n_spps, sources = 8, 2, 2
    windows, index = S.window_table([(24, 40), (16, 16), (19, 9)], T, n_spps, sources)
    per_tile = n_spps * sources + 1
    assert len(windows) == len(index) == (3 * 5 + 2 * 2 + 2 * 1) * per_tile
    assert windows.dtype.itemsize == 16
    k = 0
    for s, (h, w) in enumerate([(24, 40), (16, 16), (19, 9)]):
        target = s * per_tile + per_tile - 1
        for i in range(h // T):
            for j in range(w // T):
                for spp in range(n_spps):
                    for src in range(sources):
                        assert tuple(windows[k]) == (s * per_tile + spp * sources + src, target, i * T, j * T) and index[k] == spp
                        k += 1
                assert tuple(windows[k]) == (target, target, i * T, j * T) and index[k] == S.TARGET
                k += 1
    assert k == len(windows)
    assert windows["y0"].max() == 16 and windows["x0"].max() == 32      # 19 // 8 = 2 rows, 9 // 8 = 1 column: the remainders are dropped
    empty, none = S.window_table([], T, n_spps, sources)
    assert len(empty) == len(none) == 0


@pytest.mark.parametrize("group", [False, True])
def test_files_and_json_shape(tmp_path, group):
    case = CASES["grouped"]
    stats = joined(case, R.make_tiles(case), group)
    written = stats.write(str(tmp_path / "made" / "here"), "validation")      # the directory is created
    names = ["validation_statistics_4.json", "validation_statistics_16.json"] if group else ["validation_statistics.json"]
    assert [os.path.basename(p) for p, _, _ in written] == names and sorted(os.listdir(str(tmp_path / "made" / "here"))) == sorted(names)
    for path, spp, entries in written:
        text = open(path, encoding="utf-8").read()
        assert text == json.dumps(entries, sort_keys=True, indent=2)
        loaded = json.loads(text)
        golden = case["results"][str(spp)] if group else None
        assert golden is None or sorted(loaded) == sorted(golden)
        for name, entry in loaded.items():
            assert sorted(entry) == ["number_of_channels", "statistics", "statistics_log1p"]
            assert entry["number_of_channels"] == RenderPasses.number_of_channels(name.split("/")[-1].replace(" Masked", ""))
            for section in ("statistics", "statistics_log1p"):
                assert sorted(entry[section]) == ["coverage", "maximum", "mean", "minimum", "variance"]
                assert all(isinstance(v, float) for v in entry[section].values())
            assert entry["statistics"]["coverage"] == entry["statistics_log1p"]["coverage"]
        assert "statistics" in os.path.basename(path)      # train.py's JSON listing skips such names
    lines = S.table_lines(written[0][2])
    assert len(lines) == 1 + len(written[0][2]) and lines[0].split()[:2] == ["name", "mean"]


def test_bank_for_passes_lays_out_every_count(tmp_path):
    """FrameBank.for_passes without an Architecture, on the CPU device: a scene owns len(spps) * S source planes, the first count first, then
    its target plane -- the planes window_table names."""
    import frames_util as U
    from deepdenoiser_amd.frame_bank import FrameBank, FrameSet
    source, target, spps = ["Depth", "Diffuse Direct"], ["Diffuse Color", "Diffuse Direct"], [4, 16]
    rng = np.random.default_rng(5)
    written = {name: U.write_scene(str(tmp_path), name, spps, source, target, h, w, rng, sources=2, target_spp=64) for name, h, w in (("a", 16, 24), ("b", 8, 8))}
    path = U.write_json(str(tmp_path), {"training": ["a", "b"]}, 8, spps, 2, source, target, target_spp=64)
    frame_set = FrameSet.from_json(path, "training", log=lambda m: None)
    stats = S.FrameStatistics(frame_set)
    assert stats.passes == ["Depth", "Diffuse Direct", "Diffuse Color"] and stats.mask_of == {"Diffuse Direct": "Diffuse Color"}
    bank = FrameBank.for_passes(frame_set, stats.source_channels, stats.target_channels, spps, device="cpu", threads=2, log=lambda m: None)
    assert (bank.S, bank.n_planes, bank.hw) == (4, 10, [(16, 24)] * 5 + [(8, 8)] * 5)
    assert bank.total_bytes == (16 * 24 + 8 * 8) * stats.bytes_per_pixel
    for s, name in enumerate(("a", "b")):
        for k, spp in enumerate(spps):
            for i in range(2):
                plane = bank.source_plane(s, k * 2 + i)
                assert np.array_equal(bank.planes["Depth"][plane].numpy(), written[name][(spp, i)]["Depth"])
                assert np.array_equal(bank.planes["Diffuse Direct"][plane].numpy(), written[name][(spp, i)]["Diffuse Direct"])
                assert bank.planes["Diffuse Color"][plane] is None
        plane = bank.target_plane(s)
        assert bank.planes["Depth"][plane] is None
        assert np.array_equal(bank.planes["Diffuse Color"][plane].numpy(), written[name][(64, 0)]["Diffuse Color"])
    windows, index = S.window_table([(sc.height, sc.width) for sc in bank.scenes], 8, len(spps), 2)
    assert set(windows["mask_plane"].tolist()) == {bank.target_plane(0), bank.target_plane(1)} and len(windows) == (2 * 3 + 1) * 5
    only_b = FrameBank.for_passes(frame_set, stats.source_channels, stats.target_channels, [16], scenes=frame_set.scenes[1:], device="cpu", log=lambda m: None)
    assert (only_b.S, only_b.n_planes, only_b.spp) == (2, 3, 16)
    with pytest.raises(ValueError, match="samples per pixel"):
        FrameBank.for_passes(frame_set, stats.source_channels, stats.target_channels, [4, 8], device="cpu")


def test_a_masked_pass_needs_its_colour_pass_among_the_targets():
    case = dict(CASES["grouped"], target_passes=["Alpha", "Diffuse Direct"])
    with pytest.raises(ValueError, match="Diffuse Color"):
        S.FrameStatistics(frame_set_of(case), False)
