"""`python -m deepdenoiser_amd.nan_highlighter` against what the reference's TensorFlow/NaNHighlighter.py:40-42 computed on the same arrays
(tests/golden/nan_highlighter_golden.npz, written by tests/golden/make_nan_highlighter_golden.py), and the mask of tests/nonfinite_ref.py
against the same fixture."""
import os

import numpy as np
import pytest

from deepdenoiser_amd import nan_highlighter, openexr
from deepdenoiser_amd.summaries import decode_png

import nonfinite_ref as R

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nan_highlighter_golden.npz"))
CASES = sorted(int(k.split("_")[1]) for k in GOLDEN.files if k.startswith("input_"))


def test_the_fixture_holds_bad_and_clean_cases():
    assert len(CASES) >= 3
    assert any(GOLDEN["output_%d" % i].any() for i in CASES) and any(not GOLDEN["output_%d" % i].any() for i in CASES)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_output", [False, True])
def test_module_writes_the_reference_picture(case, with_output, tmp_path):
    image, want = GOLDEN["input_%d" % case], GOLDEN["output_%d" % case]
    exr = tmp_path / "frame.exr"
    openexr.write_image(str(exr), image)
    argv = [str(exr)] + (["--output", str(tmp_path / "elsewhere.png")] if with_output else [])
    written = nan_highlighter.main(nan_highlighter.parser().parse_known_args(argv)[0])
    assert written == str(tmp_path / ("elsewhere.png" if with_output else "frame.png")) and os.path.exists(written)
    got = decode_png(open(written, "rb").read())
    assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES)
def test_reference_mask_agrees_with_the_golden(case):
    image, want = GOLDEN["input_%d" % case], GOLDEN["output_%d" % case]
    mask, values, pixels = R.scan(image[None])
    for c in range(3):
        assert np.array_equal(((mask[0] >> c) & 1) == 1, want[..., c] == 255)
    assert values == int((want == 255).sum()) and pixels == int((want == 255).any(axis=-1).sum())
