"""Numpy restatement of dd_importance_update (TEST INFRASTRUCTURE ONLY; nothing here imports deepdenoiser_amd.frame_importance):

    tile_index      where every pixel of the un-augmented window is shown in the tile -- by running the sampler's documented forward map
                    (output pixel -> window pixel) over the whole tile and inverting the table, not by an inverse formula
    whole_cells     the frame cells that lie wholly inside a window
    update_ref      what the launch adds to acc_sum / acc_count: per term the same fp32 operations in the same order on np.float32 values,
                    the terms added in float64 in the kernel's documented order -- a lane's pixels l, l + 64, ... of the cell in the FRAME's
                    row-major order, per pixel the passes in order, channels 0 .. 2, then the shift-down tree over the 64 lanes -- so the
                    integers must be EQUAL
"""
import numpy as np


def window_pixel(y, x, T, k, flip):
    """The pixel of the un-augmented T x T window that output pixel (y, x) shows: rot90(flip_left_right(.), k) inverted (dd_sample_tiles)."""
    fy, fx = y, x
    if k == 1:
        fy, fx = x, T - 1 - y
    elif k == 2:
        fy, fx = T - 1 - y, T - 1 - x
    elif k == 3:
        fy, fx = T - 1 - x, y
    if flip:
        fx = T - 1 - fx
    return fy, fx


def tile_index(T, k, flip):
    """int arrays (ty, tx) [T, T]: window pixel (fy, fx) is shown by tile pixel (ty[fy, fx], tx[fy, fx])."""
    ty, tx = np.full((T, T), -1, dtype=np.int64), np.full((T, T), -1, dtype=np.int64)
    for y in range(T):
        for x in range(T):
            fy, fx = window_pixel(y, x, T, k, flip)
            assert ty[fy, fx] == -1
            ty[fy, fx], tx[fy, fx] = y, x
    assert (ty >= 0).all()
    return ty, tx


def whole_cells(y0, x0, T, G):
    """[(cy, cx)] of the frame cells wholly inside [y0, y0 + T) x [x0, x0 + T), row-major."""
    return [(cy, cx) for cy in range(-(-y0 // G), (y0 + T) // G) for cx in range(-(-x0 // G), (x0 + T) // G)]


def cell_sum(terms):
    """terms: float32 [G * G, n_passes, 3], pixels in the frame's row-major order -> the double lane 0 holds after the tree."""
    n = terms.shape[0]
    flat = terms.astype(np.float64).reshape(n, -1)
    lanes = np.zeros(64, dtype=np.float64)
    for start in range(0, n, 64):
        block = flat[start:start + 64]
        for j in range(block.shape[1]):                        # passes in order, channels 0 .. 2
            lanes[:len(block)] = lanes[:len(block)] + block[:, j]
    delta = 32
    while delta >= 1:
        lanes = lanes[:delta] + lanes[delta:2 * delta]         # lane i += lane i + delta; lanes 0 .. delta - 1 go on
        delta //= 2
    return float(lanes[0])


def update_ref(passes, records, flips, rotates, plane_hw, cell_base, n_cells, T, G, use_flip, use_rotate, eps):
    """passes: [(pred [B, T, T, >= 3] float32, target [B, T, T, >= 3] float32)]; records: [B, 4] (source plane, target plane, y0, x0), in
    range or not (clamped as the kernel clamps); flips, rotates: the draws' fields [B]; plane_hw: [(h, w)]; cell_base: per plane.
    -> (acc_sum uint64 [n_cells], acc_count uint32 [n_cells], visited: [(b, cell index)])"""
    eps = np.float32(eps)
    acc_sum, acc_count, visited = [0] * n_cells, np.zeros(n_cells, dtype=np.uint32), []
    index = {}
    for b, (_, tp, y0, x0) in enumerate(np.asarray(records).tolist()):
        tp = min(max(tp, 0), len(plane_hw) - 1)
        h, w = plane_hw[tp]
        if h < T or w < T or cell_base[tp] < 0:
            continue
        y0, x0 = min(max(y0, 0), h - T), min(max(x0, 0), w - T)
        k = (int(rotates[b]) & 3) if use_rotate else 0
        flip = bool(use_flip) and int(flips[b]) > 0
        if (k, flip) not in index:
            index[(k, flip)] = tile_index(T, k, flip)
        ty, tx = index[(k, flip)]
        for cy, cx in whole_cells(y0, x0, T, G):
            wy, wx = cy * G - y0, cx * G - x0
            assert 0 <= wy <= T - G and 0 <= wx <= T - G
            yy, xx = ty[wy:wy + G, wx:wx + G].reshape(-1), tx[wy:wy + G, wx:wx + G].reshape(-1)
            terms = np.empty((G * G, len(passes), 3), dtype=np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                for p, (pred, target) in enumerate(passes):
                    q, t = pred[b, yy, xx, :3], target[b, yy, xx, :3]
                    assert q.dtype == np.float32 and t.dtype == np.float32
                    terms[:, p, :] = np.abs(q - t) / ((np.abs(q) + np.abs(t)) + eps)
                mean = cell_sum(terms) / (G * G * 3 * len(passes))
            if not np.isfinite(mean):
                continue
            cell = int(cell_base[tp]) + cy * (w // G) + cx
            acc_sum[cell] += int(np.rint(mean * 4294967296.0))      # (llrint: to nearest, ties to even)
            acc_count[cell] += 1
            visited.append((b, cell))
    return np.array(acc_sum, dtype=np.uint64), acc_count, visited


def cell_bases(sizes, target_planes, n_planes, G):
    """(cell_base int32 [n_planes], n_cells): scene s, of sizes[s], owns the cells from cell_base[target_planes[s]] on; -1 elsewhere."""
    base, at = np.full(n_planes, -1, dtype=np.int32), 0
    for (h, w), tp in zip(sizes, target_planes):
        base[tp] = at
        at += (h // G) * (w // G)
    return base, at
