"""Host side of tile_blend="feather" (no GPU): tiling.blend_weights / blend_cover against tests/blend_ref.py, the argument checks of
Predictor, the command-line options, the ctypes mirror of dd_blend_axis and the argument checks of dd_stitch_blend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blend_ref as R
from deepdenoiser_amd import _lib
from deepdenoiser_amd.tiling import blend_cover, blend_weights, tile_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(61, 45, 32, 4), (100, 37, 24, 3), (929, 1001, 128, 14), (1080, 1920, 128, 14), (45, 61, 128, 14), (16, 16, 128, 14)]
TRIPLE = CASES[:2]


def _axes(case):
    H, W, T, O = case
    plan = tile_plan(H, W, T, O)
    return plan, (plan.rows, plan.cols)


@pytest.mark.parametrize("case", CASES, ids=["%dx%d_%d_%d" % c for c in CASES])
def test_weights_are_normalised_and_match_the_reference(case):
    plan, axes = _axes(case)
    for axis in axes:
        w = blend_weights(axis)
        assert w.dtype == np.float32 and w.shape == (axis.count, axis.tile)
        want = R.axis_weights(axis.origins, axis.tile, axis.extent, 2 * axis.overlap)
        # one rounding of a value in (0, 1] to float32: half an ulp, at most 2^-25 absolute (the float64 steps before it differ by ~1e-16)
        assert np.abs(w.astype(np.float64) - want).max() <= 2.0 ** -25 + 1e-15
        total = np.zeros(axis.extent)
        for i, o in enumerate(axis.origins):
            total[o:o + axis.tile] += w[i].astype(np.float64)
        assert np.abs(total - 1.0).max() <= 1e-7
        covers = R.cover_counts(axis.origins, axis.tile, axis.extent)
        assert covers.min() >= 1
        for i, o in enumerate(axis.origins):
            single = covers[o:o + axis.tile] == 1
            assert (w[i][single] == np.float32(1.0)).all()
            assert (w[i] > 0).all()
        first, last = blend_cover(axis)
        for p in range(axis.extent):
            assert list(range(first[p], last[p] + 1)) == R.covering(axis.origins, axis.tile, p)


def test_the_cases_hold_what_they_are_there_for():
    """a triple cover in the first two cases (the last tile overlaps two predecessors), none at 1080p, shrunk tiles, a one-tile frame"""
    for case in TRIPLE:
        plan, axes = _axes(case)
        assert R.cover_counts(plan.rows.origins, plan.tile, plan.height).max() == 3, case
    assert tile_plan(61, 45, 32, 4).rows.origins == (0, 24, 29)
    assert tile_plan(929, 1001, 128, 14).rows.origins[-3:] == (700, 800, 801)
    plan, axes = _axes((1080, 1920, 128, 14))
    assert max(R.cover_counts(a.origins, a.tile, a.extent).max() for a in axes) == 2
    plan, _ = _axes((45, 61, 128, 14))
    assert (plan.tile, plan.overlap) == (45, 4) and plan.rows.count == 1 and plan.cols.count > 1
    plan, _ = _axes((16, 16, 128, 14))
    assert plan.count == 1 and (blend_weights(plan.rows) == 1.0).all() and (blend_weights(plan.cols) == 1.0).all()


def test_no_ramp_at_a_frame_border():
    axis = tile_plan(1080, 1920, 128, 14).cols
    w = blend_weights(axis)
    T, width = axis.tile, 2 * axis.overlap
    assert axis.origins[0] == 0 and axis.origins[-1] + T == axis.extent
    assert w[0][0] == 1.0 and w[-1][T - 1] == 1.0                      # a ramp would give 0.5 / width there
    assert (w[0][:axis.origins[1]] == 1.0).all() and (w[-1][axis.origins[-2] + T - axis.origins[-1]:] == 1.0).all()
    # an interior tile ramps on both sides while its neighbour ramps the other way: with width = the shared 2 * overlap pixels the two raw
    # weights add up to 1, a linear cross-fade
    assert abs(w[1][0] - 0.5 / width) < 1e-8 and abs(w[1][T - 1] - 0.5 / width) < 1e-8 and abs(w[0][axis.origins[1]] - (width - 0.5) / width) < 1e-7
    # the reference, asked for the same tile as if it did not touch the border, says something else
    assert R.raw_weight(5, 0, T, axis.extent, width) == 0.5 / width and R.raw_weight(0, 0, T, axis.extent, width) == 1.0
    assert R.raw_weight(axis.extent - T, T - 1, T, axis.extent, width) == 1.0


def test_widths():
    axis = tile_plan(100, 37, 24, 3).rows
    T = axis.tile
    avg = blend_weights(axis, 0)                                       # plain average: 1 / (number of covering tiles)
    covers = R.cover_counts(axis.origins, T, axis.extent)
    for i, o in enumerate(axis.origins):
        assert np.array_equal(avg[i], (1.0 / covers[o:o + T]).astype(np.float32))
    assert np.array_equal(blend_weights(axis, None), blend_weights(axis, 2 * axis.overlap))
    for width in (1, 5, T // 2):
        want = R.axis_weights(axis.origins, T, axis.extent, width)
        assert np.abs(blend_weights(axis, width).astype(np.float64) - want).max() <= 2.0 ** -25 + 1e-15
    for bad in (T // 2 + 1, -1, T):
        with pytest.raises(ValueError, match="width"):
            blend_weights(axis, bad)
    # a plan without overlap: the default width is 0, every weight 1
    flat = tile_plan(64, 64, 32, 0).rows
    assert flat.origins == (0, 32) and (blend_weights(flat) == 1.0).all()


def test_predictor_refuses_unknown_modes_before_it_touches_a_device():
    from deepdenoiser_amd.prediction import Predictor
    with pytest.raises(ValueError, match="tile_blend"):
        Predictor(None, tile_blend="x")
    with pytest.raises(ValueError, match="blend_width"):
        Predictor(None, tile_blend="feather", blend_width=65)
    with pytest.raises(ValueError, match="blend_width"):
        Predictor(None, tile_blend="feather", blend_width=-1)


def test_predict_parser_accepts_the_new_options_and_keeps_its_defaults():
    from deepdenoiser_amd import predict
    a = predict.parser().parse_args(["architecture.json", "--input", "frames"])
    assert a.tile_blend == "crop" and a.blend_width is None
    assert (a.tile_size, a.tile_overlap_size, a.dtype, a.tiles_per_batch, a.nonfinite) == (128, 14, "f16", 256, "keep")
    b = predict.parser().parse_args(["architecture.json", "--tile_blend", "feather", "--blend_width", "8"])
    assert b.tile_blend == "feather" and b.blend_width == 8
    with pytest.raises(SystemExit):
        predict.parser().parse_args(["architecture.json", "--tile_blend", "average"])


def test_struct_size_matches_the_header(tmp_path):
    """the method of test_abi.py::test_struct_sizes_match_header on the new struct"""
    c = tmp_path / "t.c"
    c.write_text('#include <stdio.h>\n#include "dd_hip.h"\nint main(void){ printf("%zu\\n", sizeof(dd_blend_axis)); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert int(subprocess.check_output([exe])) == ctypes.sizeof(_lib.BlendAxis)


def _axis(origins, dev=64):
    """a dd_blend_axis whose device tables are never dereferenced: validation fails first"""
    host = (ctypes.c_int * len(origins))(*origins)
    a = _lib.BlendAxis(len(origins), host, dev, dev, dev, dev)
    a._host = host
    return a


def test_bad_arguments_return_a_status_and_set_the_error(lib):
    tiles, frames = ctypes.c_void_p(64), ctypes.c_void_p(128)
    ok = _axis([0, 8, 16])                                              # tile 16 in an extent of 32

    def call(tiles=tiles, T=16, ldt=3, per=9, frames=frames, n_img=1, H=32, W=32, ldf=3, C=3, rows=ok, cols=ok, first=0, n=9):
        return lib.dd_stitch_blend(tiles, T, ldt, per, frames, n_img, H, W, ldf, C, ctypes.byref(rows) if rows is not None else None,
                                   ctypes.byref(cols) if cols is not None else None, first, n, None)

    for kw, word in (({"tiles": None}, b"null"), ({"frames": None}, b"null"), ({"n_img": 0}, b"images"), ({"C": 0}, b"channels"),
                     ({"C": 5, "ldt": 5, "ldf": 5}, b"channels"), ({"ldt": 2}, b"ldt"), ({"ldf": 2}, b"ldf"), ({"T": 0}, b"tile"),
                     ({"T": 33}, b"does not fit"), ({"rows": None}, b"axis"), ({"cols": _axis([0, 8, 17])}, b"origins"),
                     ({"rows": _axis([0, 16, 8])}, b"ascend"), ({"rows": _axis([-1, 8, 16])}, b"origins"), ({"cols": _axis([0, 8, 16], dev=None)}, b"null"),
                     ({"first": -1}, b"tiles ["), ({"n": 0}, b"tiles ["), ({"first": 1}, b"tiles ["), ({"per": 8}, b"tiles per image")):
        assert call(**kw) == -1, kw
        assert b"dd_stitch_blend" in lib.dd_last_error() and word in lib.dd_last_error(), (kw, lib.dd_last_error())


def crop_stitch(tiles, plan):
    """the crop windows of the plan copied into the frame (Prediction.py:384-441), for row-major tiles [count, T, T, C]"""
    out = np.zeros((plan.height, plan.width, tiles[0].shape[-1]), dtype=np.float64)
    for i in range(plan.count):
        hi, wi = divmod(i, plan.cols.count)
        (a, b), (c, d) = plan.rows.crops[hi], plan.cols.crops[wi]
        y, x = plan.rows.offsets[hi], plan.cols.offsets[wi]
        out[y:y + b - a, x:x + d - c] = tiles[i][a:b, c:d]
    return out


def test_the_oracle_network_satisfies_the_seam_inequality():
    """The seam measurement of tests/test_gpu_tile_blend.py on the float64 oracle alone: the same architecture, weights and frame, tiles
    predicted one by one, cropped by the plan and blended by blend_ref.  Measured: crop 0.0130 (columns) / 0.0113 (rows), feather
    0.00126 / 0.00111."""
    import torch
    from deepdenoiser_amd.naming import Naming
    from oracle.model import OracleArchitecture
    n, T, O = R.SEAM_FRAME, R.SEAM_TILE, R.SEAM_OVERLAP
    oracle = OracleArchitecture(R.seam_architecture(), dtype=torch.float64, seed=R.SEAM_SEED)
    frame = R.seam_frame([(f.name, f.channels) for f in oracle.features + oracle.auxiliary])
    key = Naming.feature_prediction_name("Emission")
    plan = tile_plan(n, n, T, O)
    assert plan.count == 9 and plan.rows.offsets[1:] == (42, 78)
    with torch.no_grad():
        whole = oracle.predict({k: v[None] for k, v in frame.items()})[0][key][0].numpy()
        tiles = [oracle.predict({k: v[None, y:y + T, x:x + T] for k, v in frame.items()})[0][key][0].numpy() for y, x in plan.windows()]
    seams = plan.cols.offsets[1:], plan.rows.offsets[1:]
    crop = R.seam_statistic(crop_stitch(tiles, plan) - whole, *seams)
    feather = R.seam_statistic(R.blend(tiles, plan.rows.origins, plan.cols.origins, T, n, n, 2 * O, 2 * O) - whole, *seams)
    print("oracle seam statistic (columns, rows): crop %.3e %.3e, feather %.3e %.3e" % (crop + feather))
    for c, f in zip(crop, feather):
        assert c > 0 and f <= R.SEAM_FACTOR * c
