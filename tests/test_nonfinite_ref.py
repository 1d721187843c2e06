"""tests/nonfinite_ref.py -- the numpy restatement the GPU tests of dd_nonfinite_scan / dd_nonfinite_repair compare against -- on cases small
enough to compute by hand."""
import numpy as np

import nonfinite_ref as R

NAN = np.float32(np.nan)


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def test_bit_patterns():
    bad = _bits(0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff)      # +-inf, quiet / signalling NaNs
    fine = _bits(0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x80000000, 0x00000000, 0x3f800000)                  # +-FLT_MAX, denormals, -0, 0, 1
    assert R.nonfinite(bad).all() and not R.nonfinite(fine).any()
    plane = np.concatenate([bad, fine]).reshape(1, 1, 15, 1)
    mask, values, pixels = R.scan(plane)
    assert mask.tolist() == [[[1] * 8 + [0] * 7]] and (values, pixels) == (8, 8)


def test_3x3_nan_centre():
    plane = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3, 1)
    plane[0, 1, 1, 0] = NAN
    mask, values, pixels = R.scan(plane)
    assert mask[0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and (values, pixels) == (1, 1)
    out = R.repair(plane, mask, 1)
    assert out[0, 1, 1, 0] == np.float32(40.0 / 8.0)      # 1 + 2 + 3 + 4 + 6 + 7 + 8 + 9 = 40 over 8
    keep = mask == 0
    assert np.array_equal(out[..., 0][keep], plane[..., 0][keep])


def test_nan_corner_radius_1():
    plane = np.arange(1, 17, dtype=np.float32).reshape(1, 4, 4, 1)
    plane[0, 0, 0, 0] = np.float32(np.inf)
    mask, _, _ = R.scan(plane)
    out = R.repair(plane, mask, 1)
    assert out[0, 0, 0, 0] == np.float32((2.0 + 5.0 + 6.0) / 3.0)      # the clipped window is 2 x 2, three usable values
    plane[0, 3, 3, 0] = -np.float32(np.inf)
    mask, values, pixels = R.scan(plane)
    assert (values, pixels) == (2, 2)
    assert R.repair(plane, mask, 1)[0, 3, 3, 0] == np.float32((11.0 + 12.0 + 15.0) / 3.0)


def test_5x5_block_radius_2_centre_is_zero_and_the_rim_uses_outside_values_only():
    plane = np.ones((1, 9, 9, 1), dtype=np.float32) * np.float32(2.0)
    plane[0, 2:7, 2:7, 0] = NAN
    plane[0, 0, 0, 0] = np.float32(10.0)
    mask, values, pixels = R.scan(plane)
    assert (values, pixels) == (25, 25)
    out = R.repair(plane, mask, 2)
    assert out[0, 4, 4, 0] == 0.0 and np.signbit(out[0, 4, 4, 0]) == False      # noqa: E712  (its window is the block itself)
    # the block's corner (2, 2): window rows / columns 0 .. 4, 25 - 9 = 16 usable values: 15 twos and the ten
    assert out[0, 2, 2, 0] == np.float32((15 * 2.0 + 10.0) / 16.0)
    # (3, 3): window 1 .. 5, usable: row 1 and column 1 = 9 twos
    assert out[0, 3, 3, 0] == np.float32(2.0)
    assert np.isfinite(out).all()
    assert np.array_equal(out[0, :, :, 0][mask[0] == 0], plane[0, :, :, 0][mask[0] == 0])


def test_no_value_crosses_from_one_image_of_a_batch_into_the_next():
    plane = np.zeros((2, 3, 4, 1), dtype=np.float32)
    plane[0] = 1.0
    plane[1] = 100.0
    plane[0, 1, 3, 0] = NAN      # last column of image 0 ...
    plane[1, 1, 0, 0] = NAN      # ... faces the first column of image 1 in memory
    plane[0, 2, 3, 0] = NAN      # last pixel of image 0: the next floats are image 1's first row
    mask, values, pixels = R.scan(plane)
    assert (values, pixels) == (3, 3)
    out = R.repair(plane, mask, 1)
    assert out[0, 1, 3, 0] == 1.0 and out[0, 2, 3, 0] == 1.0 and out[1, 1, 0, 0] == 100.0


def test_only_channel_1_bad():
    plane = np.arange(27, dtype=np.float32).reshape(1, 3, 3, 3)
    plane[0, 1, 1, 1] = NAN
    mask, values, pixels = R.scan(plane)
    assert mask[0, 1, 1] == 2 and int(mask.sum()) == 2 and (values, pixels) == (1, 1)
    out = R.repair(plane, mask, 2)
    others = [float(plane[0, y, x, 1]) for y in range(3) for x in range(3) if (y, x) != (1, 1)]
    assert out[0, 1, 1, 1] == np.float32(sum(others) / 8.0)      # (small integers: the sum is exact in any order)
    assert out[0, 1, 1, 0] == plane[0, 1, 1, 0] and out[0, 1, 1, 2] == plane[0, 1, 1, 2]
    # a neighbour that is bad in ANOTHER channel is still usable in this one
    plane[0, 0, 0, 0] = NAN
    mask, values, pixels = R.scan(plane)
    assert mask[0, 0, 0] == 1 and (values, pixels) == (2, 2)
    assert R.repair(plane, mask, 2)[0, 1, 1, 1] == out[0, 1, 1, 1]


def test_sums_are_sequential_float32_in_row_major_order():
    plane = np.zeros((1, 1, 5, 1), dtype=np.float32)
    plane[0, 0, :, 0] = [2.0 ** 24, 1.0, NAN, 1.0, -(2.0 ** 24)]
    mask, _, _ = R.scan(plane)
    # ((2^24 + 1) + 1) - 2^24 in fp32 = 0 (each + 1 is lost), not the exact 2
    assert R.repair(plane, mask, 2)[0, 0, 2, 0] == 0.0
