"""Importance crops, host side (deepdenoiser_amd/frame_importance.py through ImportanceMap.from_cells; no GPU, no library): the lattice windows'
probabilities against tests/importance_ref.py, the draws (deterministic, valid, sharded over ranks like the other modes), the frequencies of
40 000 draws, the command line, and the records of 'random' and 'grid' against values recorded from the commit before this mode existed
(tests/golden/frame_draws_parent.json)."""
import json
import math
import os
import random

import numpy as np
import pytest

import importance_ref as R
from deepdenoiser_amd.frame_bank import TileRecords
from deepdenoiser_amd.frame_importance import ImportanceMap, resolve_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, G, S = 8, 4, 2
SIZES = [(24, 40), (18, 20)]      # (18 - 8) % 4 != 0: the last lattice row of the second scene ends 2 pixels above the last origin
TUPLES = [[0], [1]]


class _Scene:
    def __init__(self, h, w):
        self.height, self.width = h, w


class _Bank:
    """What TileRecords and ImportanceMap.from_cells read of a FrameBank."""

    def __init__(self, sizes=SIZES, tile=T):
        self.tile, self.S, self.scenes = tile, S, [_Scene(h, w) for h, w in sizes]
        self.hw = [hw for hw in sizes for _ in range(S + 1)]
        self.n_planes = len(self.hw)

    def source_plane(self, s, k):
        return s * (S + 1) + k

    def target_plane(self, s):
        return s * (S + 1) + S


def _cells(seed=1):
    """Cell means in [0, 1], most of them small, a few large; one block of exact zeros."""
    rng = np.random.default_rng(seed)
    out = [rng.random((h // G, w // G)) ** 4 for h, w in SIZES]
    out[0][:2, :3] = 0.0
    return out


def _lattice_sizes():
    return [((h - T) // G + 1, (w - T) // G + 1) for h, w in SIZES]


def test_probabilities_match_the_reference_and_sum_to_one():
    assert _lattice_sizes() == [(5, 9), (3, 4)]                # 57 lattice windows
    for floor in (0.0, 0.25, 0.6, 1.0):
        m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G, floor=floor)
        have, want = m.probabilities(), R.probabilities_ref(_cells(), SIZES, T, G, floor)
        assert [p.shape for p in have] == _lattice_sizes() and all(p.dtype == np.float64 for p in have)
        assert abs(sum(float(p.sum()) for p in have) - 1.0) <= 1e-12
        for p, q, W, c, (h, w) in zip(have, want, m.weights, _cells(), SIZES):
            assert np.allclose(p, q, rtol=1e-12, atol=1e-15)
            assert np.allclose(W, R.window_weights_ref(c, h, w, T, G), rtol=1e-12, atol=1e-15)
        assert m.cdf.dtype == np.float64 and len(m.cdf) == 57 and (np.diff(m.cdf) >= 0).all()
    # floor = 1: exactly what 'random' crops give a lattice window
    m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G, floor=1.0)
    for p, (ni, nj) in zip(m.probabilities(), _lattice_sizes()):
        assert (p == 1.0 / (2 * ni * nj)).all()
    # every source equals its target: the same, whatever the floor
    for floor in (0.0, 0.25, 1.0):
        m = ImportanceMap.from_cells(_Bank(), [np.zeros_like(c) for c in _cells()], cell=G, floor=floor)
        for p, (ni, nj) in zip(m.probabilities(), _lattice_sizes()):
            assert (p == 1.0 / (2 * ni * nj)).all()
        assert m.heaviest_tenth_share() == 0.0 and (m.picture(0) == 0).all()


def test_one_nonzero_cell_without_a_floor():
    cells = [np.zeros((6, 10)), np.zeros((4, 5))]
    cells[0][3, 6] = 0.5
    m = ImportanceMap.from_cells(_Bank(), cells, cell=G, floor=0.0)
    p = m.probabilities()
    covering = {(i, j) for i in (2, 3) for j in (5, 6)}        # a window spans T / G = 2 cells: rows i, i + 1 and columns j, j + 1
    assert {(int(i), int(j)) for i, j in np.argwhere(p[0] > 0)} == covering and (p[1] == 0).all()
    assert np.allclose(p[0][p[0] > 0], 0.25, rtol=1e-15)
    rng = random.Random(2)
    for _ in range(200):
        s, y0, x0, tup = m.draw(rng, TUPLES)
        assert s == 0 and (y0 // G, x0 // G) in covering and tup in TUPLES
    picture = m.picture(0)
    assert picture.dtype == np.uint8 and picture.shape == (5, 9) and picture.max() == 255 and (picture > 0).sum() == 4 and (m.picture(1) == 0).all()
    assert m.heaviest_tenth_share() == 1.0                     # ceil(57 / 10) = 6 windows hold all four


def test_draws_follow_the_documented_order_of_calls():
    m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G, floor=0.25)
    ref = R.probabilities_ref(_cells(), SIZES, T, G, 0.25)
    a, b = random.Random(9), random.Random(9)
    for _ in range(300):
        s, y0, x0, tup = m.draw(a, TUPLES)
        rs, ri, rj, ry0, rx0, rtup = R.draw_ref(b, ref, SIZES, T, G, TUPLES)
        assert (s, y0, x0, tup) == (rs, ry0, rx0, rtup) and (y0 // G, x0 // G) == (ri, rj)
    assert a.random() == b.random()                            # the same number of calls on the generator


def test_draws_are_deterministic_valid_and_shard_over_ranks():
    bank = _Bank()
    m = ImportanceMap.from_cells(bank, _cells(), cell=G, floor=0.25)
    B, world = 3, 2
    n = TileRecords(bank, B).epoch_examples(TUPLES)            # (3 * 5 + 2 * 2) * 2 = 38 examples: six rounds of world * B, 2 are dropped

    def epoch(rank, world, B, seed=7):
        rec, rng, out = TileRecords(bank, B), random.Random(seed), []
        rec.set_importance(m)
        while True:
            r = rec.draw(rng, "importance", TUPLES, rank, world)
            if r is None:
                return out
            assert r.shape == (B, 4) and r.dtype == np.int32
            rec.validate(r)
            out.append(r)
    r0, r1, again = epoch(0, world, B), epoch(1, world, B), epoch(0, world, B)
    assert n == 38 and len(r0) == len(r1) == n // (world * B) == 6
    assert all(np.array_equal(a, b) for a, b in zip(r0, again))
    assert not all(np.array_equal(a, b) for a, b in zip(r0, epoch(0, world, B, seed=8)))
    whole = epoch(0, 1, world * B)
    for k in range(6):
        assert np.array_equal(np.concatenate([r0[k], r1[k]]), whole[k])
    flat = np.concatenate(whole)
    assert (flat[:, 2] % G != 0).any() and (flat[:, 3] % G != 0).any()      # the jitter: not on the lattice
    # the next call starts the next epoch
    rec, rng = TileRecords(bank, B), random.Random(1)
    rec.set_importance(m)
    while rec.draw(rng, "importance", TUPLES) is not None:
        pass
    assert rec.draw(rng, "importance", TUPLES) is not None


def test_every_origin_is_reachable():
    """Floor 1 on a small scene: all (h - T + 1) * (w - T + 1) origins occur, the last rows and columns through the clamp."""
    bank = _Bank([(18, 13)])
    m = ImportanceMap.from_cells(bank, [np.zeros((4, 3))], cell=G, floor=1.0)
    rng, seen = random.Random(3), set()
    for _ in range(4000):
        s, y0, x0, _ = m.draw(rng, TUPLES)
        assert 0 <= y0 <= 10 and 0 <= x0 <= 5
        seen.add((y0, x0))
    assert len(seen) == 11 * 6


def test_refusals():
    bank = _Bank()
    rec = TileRecords(bank, 3)
    with pytest.raises(ValueError, match="no importance map is attached"):
        rec.draw(random.Random(0), "importance", TUPLES)
    with pytest.raises(ValueError, match="not 'spiral'"):
        rec.draw(random.Random(0), "spiral", TUPLES)
    for cell in (3, 16, 0, -4, 65, 128):                       # no divisor of 8, or outside 1 .. 64
        with pytest.raises(ValueError, match="cell=%d" % cell):
            ImportanceMap.from_cells(bank, _cells(), cell=cell)
    for floor in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="floor"):
            ImportanceMap.from_cells(bank, _cells(), cell=G, floor=floor)
    with pytest.raises(ValueError, match="shape"):
        ImportanceMap.from_cells(bank, _cells(), cell=2)
    with pytest.raises(ValueError, match="other frames"):
        TileRecords(_Bank([(24, 40)]), 3).set_importance(ImportanceMap.from_cells(bank, _cells(), cell=G))
    assert [resolve_cell(t) for t in (128, 64, 24, 20, 18, 7)] == [16, 16, 8, 4, 2, 1] and resolve_cell(128, 64) == 64

    class _Passes:
        source_channels, target_channels = {"Depth": 1, "Normal": 3, "Alpha": 1}, {"Alpha": 1, "Diffuse Color": 3}
    from deepdenoiser_amd.frame_importance import colour_passes
    with pytest.raises(ValueError, match="no colour pass that is both a source and a target"):
        colour_passes(_Passes)
    _Passes.source_channels = {"Normal": 3, "Glossy Direct": 3, "Diffuse Color": 3, "Alpha": 1}
    _Passes.target_channels = {"Glossy Direct": 3, "Diffuse Color": 3, "Alpha": 1}
    assert colour_passes(_Passes) == ["Diffuse Color", "Glossy Direct"]


def test_frequencies_of_40000_draws():
    """Every lattice window's frequency within five standard deviations of a binomial count (plus one count) of its probability -- a condition on
    the seed, checked here; the probabilities are the reference's."""
    N, seed = 40000, 17
    m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G, floor=0.25)
    probabilities = R.probabilities_ref(_cells(), SIZES, T, G, 0.25)
    counts = [np.zeros(p.shape, dtype=np.int64) for p in probabilities]
    rng = random.Random(seed)
    for _ in range(N):
        s, y0, x0, _ = m.draw(rng, TUPLES)
        counts[s][y0 // G, x0 // G] += 1
    worst = 0.0
    for c, p in zip(counts, probabilities):
        bound = 5.0 * np.sqrt(p * (1.0 - p) / N) + 1.0 / N
        worst = max(worst, float((np.abs(c / N - p) / bound).max()))
        assert (np.abs(c / N - p) <= bound).all()
    print("40000 draws over %d windows: the worst deviation is %.2f of its bound" % (sum(p.size for p in probabilities), worst))
    assert sum(int(c.sum()) for c in counts) == N and math.isfinite(worst)


def test_parser():
    from deepdenoiser_amd import train
    args = train.parser().parse_args(["t.json"])
    assert (args.frames_crops, args.frames_importance_floor, args.frames_importance_cell, args.frames_importance_png) == ("random", 0.25, None, None)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_crops", "importance"])
    assert (args.frames_crops, args.frames_importance_floor, args.frames_importance_cell, args.frames_importance_png) == ("importance", 0.25, None, None)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_crops", "importance", "--frames_importance_floor", "0.5",
                                      "--frames_importance_cell", "8", "--frames_importance_png", "pictures"])
    assert (args.frames_importance_floor, args.frames_importance_cell, args.frames_importance_png) == (0.5, 8, "pictures")
    for crops in ([], ["--frames_crops", "grid"]):
        for flag, value in (("--frames_importance_floor", "0.5"), ("--frames_importance_cell", "8"), ("--frames_importance_png", "pictures")):
            with pytest.raises(SystemExit):
                train.parser().parse_args(["t.json", "--frames", "f.json"] + crops + [flag, value])
    assert "0.25" in train.parser().format_help() and "not a measured optimum" in " ".join(train.parser().format_help().split())


def test_sub_option_error_names_the_flag(capsys):
    from deepdenoiser_amd import train
    with pytest.raises(SystemExit):
        train.parser().parse_args(["t.json", "--frames_importance_cell", "8"])
    assert "--frames_importance_cell needs --frames_crops importance" in capsys.readouterr().err


@pytest.mark.parametrize("crops", ["random", "grid"])
def test_random_and_grid_draw_what_they_drew_before(crops):
    """The seeded records of the two older modes, both ranks, two epochs from one generator: equal to the recorded ones, with and without an
    attached map."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "frame_draws_parent.json")))
    bank = _Bank([tuple(hw) for hw in gold["sizes"]], gold["tile"])
    assert gold["sources"] == S
    for attached in (False, True):
        for rank in range(gold["world"]):
            rec, rng, batches = TileRecords(bank, gold["B"]), random.Random(gold["seed"]), []
            if attached:
                rec.set_importance(ImportanceMap.from_cells(bank, _cells(), cell=G))
            for _ in range(2):
                while True:
                    r = rec.draw(rng, crops, gold["index_tuples"], rank, gold["world"])
                    if r is None:
                        break
                    assert r.dtype == np.int32
                    batches.append(r.tolist())
            assert batches == gold[crops][rank] and len(batches) == 18
