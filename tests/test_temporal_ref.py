"""tests/temporal_ref.py against what the algorithm of include/dd_hip.h (dd_temporal_stabilize) implies in closed form, the ambiguity
condition of the GPU tests on their generators, and the frame order of --input_sequence.  No GPU."""
import os

import numpy as np
import pytest

import temporal_ref as R


def _image(H, W, C, seed):
    return np.abs(np.random.default_rng(seed).standard_normal((H, W, C))).astype(np.float32)


def test_zero_motion_and_equal_history_change_nothing():
    """One of nine values lies at most sqrt(8) standard deviations from their mean, so from gamma = 3 on the clamp cannot touch a history that
    equals the current frame; at gamma = 1 it does touch the pixels that stand out of their own window, and only those."""
    current = _image(9, 11, 3, 1)
    r = R.stabilize([(current, current)], np.zeros((9, 11, 2), np.float32), -1.0, 1.0, 0.8, 3.0)[0]
    assert np.array_equal(r["out"], current) and r["pixels_blended"] == 99 and r["values_clamped"] == 0
    assert r["change"] == 0.0 and r["flicker_before"] == 0.0 and r["flicker_after"] == 0.0
    r = R.stabilize([(current, current)], np.zeros((9, 11, 2), np.float32), -1.0, 1.0, 0.8, 1.0)[0]
    outside = np.abs(current.astype(np.float64) - r["m"]) > r["s"]
    assert np.array_equal(r["out"] != current, outside) and r["values_clamped"] == outside.sum() > 0 and r["flicker_before"] == 0.0


def test_alpha_zero_keeps_the_current_frame():
    currents, histories, motion, _ = R.make_case(13, 17, [3, 1], 2)
    for r, current in zip(R.stabilize(list(zip(currents, histories)), motion, -1.0, 1.0, 0.0, 1.0), currents):
        assert np.array_equal(r["out"], current) and r["change"] == 0.0 and r["pixels_blended"] > 0


def test_large_gamma_and_integer_motion_give_the_exact_blend():
    H, W, alpha = 12, 15, 0.75
    current = _image(H, W, 3, 3)
    previous = _image(H, W, 3, 4)
    motion = np.zeros((H, W, 2), np.float32)
    motion[..., 0], motion[..., 1] = 2.0, 1.0                    # sx = -1, sy = +1: the pixel was at (x - 2, y + 1)
    r = R.stabilize([(current, previous)], motion, -1.0, 1.0, alpha, 1e6)[0]
    shifted = previous[2:H, 0:W - 3].astype(np.float64)          # previous[y + 1, x - 2] for y in 1 .. H-2, x in 2 .. W-2
    want = current[1:H - 1, 2:W - 1] + alpha * (shifted - current[1:H - 1, 2:W - 1])
    assert np.array_equal(r["out"][1:H - 1, 2:W - 1], want.astype(np.float32)) and r["values_clamped"] == 0
    assert r["offscreen"][:, :2].all() and r["offscreen"][H - 1].all() and not r["offscreen"][:H - 1, 2:].any()
    assert np.array_equal(r["out"][:, :2], current[:, :2])


def test_gamma_zero_blends_towards_the_window_mean():
    currents, histories, motion, _ = R.make_case(10, 14, [3], 5)
    r = R.stabilize([(currents[0], histories[0])], motion, -1.0, 1.0, 0.8, 0.0)[0]
    c = currents[0].astype(np.float64)
    want = (c + np.float64(np.float32(0.8)) * (r["m"] - c)).astype(np.float32)
    assert np.array_equal(r["out"][r["blended"]], want[r["blended"]]) and r["blended"].sum() > 40
    padded = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    assert np.allclose(r["m"][0, 0], (padded[0:3, 0:3].sum(axis=(0, 1))) / 9.0, rtol=1e-14)
    assert np.allclose(r["s"][4, 5], padded[4:7, 5:8].reshape(9, 3).std(axis=0), rtol=1e-9)


def test_rejection_categories_and_their_precedence():
    H, W = 6, 8
    current, history = _image(H, W, 3, 6), _image(H, W, 3, 7)
    motion = np.zeros((H, W, 2), np.float32)
    motion[0, 0, 0] = 1.0                        # (0,0) came from x = -1: offscreen
    motion[0, 1, 1] = np.nan                     # not finite: offscreen
    motion[0, 2, 0] = -np.inf                    # offscreen
    motion[5, 7, 1] = 0.125                      # y = 5.125 > H - 1: offscreen
    guide_previous = np.zeros((H, W, 1), np.float32)
    guide_current = guide_previous.copy()
    guide_current[0, 0] = guide_current[2, 2] = 1.0      # (0,0) is offscreen AND differs: offscreen takes precedence
    guide_current[2, 3] = 0.25                            # exactly the tolerance: kept
    guide_current[2, 4] = np.nan                          # a non-finite difference rejects
    current[4, 4, 1] = np.inf                             # the nine windows around it are nonfinite
    current[2, 2, 0] = np.nan                             # guide-rejected (2,2) stays `guide`; its neighbours are nonfinite
    history[1, 6, 2] = np.nan                             # h of (1,6) only (zero motion, weights 1 0 0 0 ... but 0 * NaN is NaN at the clamped taps)
    r = R.stabilize([(current, history)], motion, -1.0, 1.0, 0.8, 1.0, [(guide_current, guide_previous, 0.25)])[0]
    want_offscreen = np.zeros((H, W), bool)
    want_offscreen[0, 0] = want_offscreen[0, 1] = want_offscreen[0, 2] = want_offscreen[5, 7] = True
    assert np.array_equal(r["offscreen"], want_offscreen)
    want_guide = np.zeros((H, W), bool)
    want_guide[2, 2] = want_guide[2, 4] = True
    assert np.array_equal(r["guide"], want_guide)
    want_nonfinite = np.zeros((H, W), bool)
    want_nonfinite[3:6, 3:6] = True
    want_nonfinite[1:4, 1:4] = True
    want_nonfinite[1, 6] = True
    want_nonfinite[0, 6] = want_nonfinite[1, 5] = want_nonfinite[0, 5] = True      # their taps (y0+1, x0+1 with weight 0) touch the NaN: 0 * NaN
    want_nonfinite &= ~want_offscreen & ~want_guide
    assert np.array_equal(r["nonfinite"], want_nonfinite)
    assert r["pixels_offscreen"] + r["pixels_guide"] + r["pixels_nonfinite"] + r["pixels_blended"] == H * W
    assert (r["pixels_offscreen"], r["pixels_guide"]) == (4, 2) and r["pixels_blended"] == (~want_offscreen & ~want_guide & ~want_nonfinite).sum()
    rejected = ~r["blended"]
    assert np.array_equal(r["out"][rejected].view(np.uint32), current[rejected].view(np.uint32))      # bit for bit, NaN included
    assert np.isfinite(r["out"][r["blended"]]).all()


@pytest.mark.parametrize("shape", [(45, 70), (33, 37), (1, 1), (1, 40), (40, 1)])
@pytest.mark.parametrize("sprinkle", [False, True])
def test_counts_add_up_and_few_channels_are_ambiguous(shape, sprinkle):
    """The condition the GPU tests assert on their cases: at most 0.5 % of the channels lie within 1e-4 of a clamp bound."""
    H, W = shape
    currents, histories, motion, guides = R.make_case(H, W, [3, 1, 3], 11, guides=2, sprinkle=sprinkle)
    for gamma in (0.5, 1.0):
        for r, current in zip(R.stabilize(list(zip(currents, histories)), motion, -1.0, 1.0, 0.8, gamma, guides), currents):
            assert r["pixels_offscreen"] + r["pixels_guide"] + r["pixels_nonfinite"] + r["pixels_blended"] == H * W
            assert r["ambiguous"].sum() <= 0.005 * current.size
            if H * W > 1000:
                assert r["pixels_blended"] > H * W // 4 and r["pixels_offscreen"] > 0 and r["pixels_guide"] > 0
                assert 0 < r["values_clamped"] < r["pixels_blended"] * current.shape[2]
                assert r["flicker_after"] < r["flicker_before"]


def test_sequence_frames_are_ordered_by_their_numbers(tmp_path):
    from deepdenoiser_amd import temporal
    for name in ("f10", "f2", "f1", "shot2_frame003", "shot2_frame0010", "shot10_frame001", "notes", "empty9"):
        os.makedirs(tmp_path / name)
        if name not in ("notes", "empty9"):
            open(tmp_path / name / "render_Normal_0001.exr", "wb").close()
    open(tmp_path / "notes" / "readme.txt", "w").close()
    open(tmp_path / "f3.exr", "wb").close()                      # a file, not a frame directory
    have = [os.path.basename(p) for p in temporal.frame_directories(str(tmp_path))]
    assert have == ["f1", "f2", "shot2_frame003", "shot2_frame0010", "f10", "shot10_frame001"]      # (1) (2) (2,3) (2,10) (10) (10,1)
    assert have.index("f2") < have.index("f10")
    assert temporal.parse_guide("Normal:0.25") == ("Normal", 0.25) and temporal.parse_guide("Screen Space Normal:1") == ("Screen Space Normal", 1.0)
    for bad in ("Normal", "Normal:", ":0.5", "Normal:-1", "Normal:nan", "Normal:x"):
        with pytest.raises(ValueError):
            temporal.parse_guide(bad)
