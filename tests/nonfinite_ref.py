"""numpy restatement of dd_nonfinite_scan / dd_nonfinite_repair (include/dd_hip.h), the reference of tests/test_gpu_nonfinite.py.

Planes are [N,H,W,C] float32 arrays (the first C channels of a wider tensor are what the kernels look at).  The mask comes from the bit
pattern (all eight exponent bits set); the window sums are sequential np.float32 additions in row-major window order followed by ONE
np.float32 division, the order the kernel states."""
import numpy as np


def nonfinite(a):
    """bool array: all eight exponent bits of the float32 set (+-inf, any NaN)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def scan(plane):
    """[N,H,W,C] float32 -> (uint8 mask [N,H,W] with bit c set where channel c is non-finite, non-finite values, pixels with at least one)."""
    bad = nonfinite(plane)
    assert bad.ndim == 4 and bad.shape[3] in (1, 3), bad.shape
    mask = np.zeros(bad.shape[:3], dtype=np.uint8)
    for c in range(bad.shape[3]):
        mask |= (bad[..., c].astype(np.uint8) << c).astype(np.uint8)
    return mask, int(bad.sum()), int((mask != 0).sum())


def repair(plane, mask, radius):
    """-> a repaired copy of `plane`: every value whose mask bit is set becomes the mean of the values of the same channel and image in the
    (2 radius + 1)^2 window, clipped to the image, whose mask bit is clear; 0 when there is none.  Unmasked values are copied untouched.

    Vectorised over the masked values, never over the window: every running sum receives its window's values one after the other in row-major
    window order, each addition rounded to float32, and is divided once."""
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    out = plane.copy()
    N, H, W, C = plane.shape
    for c in range(C):
        n, y, x = np.nonzero((mask >> c) & 1)
        if n.size == 0:
            continue
        total, count = np.zeros(n.size, dtype=np.float32), np.zeros(n.size, dtype=np.int32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                yy, xx = y + dy, x + dx
                inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
                usable = inside & (((mask[n, yc, xc] >> c) & 1) == 0)
                with np.errstate(all="ignore"):
                    added = total + plane[n, yc, xc, c]              # float32 + float32 -> one float32 rounding
                assert added.dtype == np.float32
                total = np.where(usable, added, total)
                count += usable
        with np.errstate(all="ignore"):
            mean = total / np.maximum(count, 1).astype(np.float32)
        out[n, y, x, c] = np.where(count > 0, mean, np.float32(0.0)).astype(np.float32)
    return out
