"""The temporal stabilisation of include/dd_hip.h (dd_temporal_stabilize) in numpy float64 (TEST INFRASTRUCTURE ONLY).

    results = stabilize(passes, motion, sx, sy, alpha, gamma, guides)

passes: [(current [H,W,C], history [H,W,C])], motion [H,W,>=2], guides: [(current, previous, tolerance)].  The previous position and what
follows from it alone (offscreen, the tap indices and weights, the nearest previous pixel) are computed in float32 with one rounding per
operation, as the header states them, so those decisions are the kernel's for ANY input; everything else is float64.  Per pass a dictionary:
out (float32: the float64 blend rounded once; rejected pixels are `current` bit for bit), the four pixel counts, values_clamped, the three
sums, the category masks, and `ambiguous`: the [H,W,C] mask of blended channels whose h lies within 1e-4 of lo or hi (there fp32 and
float64 may clamp differently)."""
import numpy as np

AMBIGUOUS = 1e-4


def positions(motion, sx, sy):
    """-> offscreen [H,W] bool, x0, y0 (int), fx, fy (float64 of the float32 weights), nx, ny (int; the nearest previous pixel, clamped)"""
    motion = np.asarray(motion, dtype=np.float32)
    H, W = motion.shape[:2]
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        px = (x + np.float32(sx) * motion[..., 0]).astype(np.float32)
        py = (y + np.float32(sy) * motion[..., 1]).astype(np.float32)
        onscreen = (px >= 0) & (px <= np.float32(W - 1)) & (py >= 0) & (py <= np.float32(H - 1))      # (NaN and the infinities fail)
        px = np.where(onscreen, px, np.float32(0))
        py = np.where(onscreen, py, np.float32(0))
        xf, yf = np.floor(px), np.floor(py)
        fx, fy = (px - xf).astype(np.float32), (py - yf).astype(np.float32)
        nx = np.clip(np.floor((px + np.float32(0.5)).astype(np.float32)).astype(np.int64), 0, W - 1)
        ny = np.clip(np.floor((py + np.float32(0.5)).astype(np.float32)).astype(np.int64), 0, H - 1)
    return ~onscreen, xf.astype(np.int64), yf.astype(np.int64), fx.astype(np.float64), fy.astype(np.float64), nx, ny


def guide_rejected(guides, nx, ny):
    H, W = nx.shape
    rejected = np.zeros((H, W), dtype=bool)
    for current, previous, tolerance in guides:
        current, previous = np.asarray(current, dtype=np.float64), np.asarray(previous, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            difference = np.abs(current - previous[ny, nx])
            rejected |= ~(difference <= np.float64(np.float32(tolerance))).all(axis=2)      # (a NaN difference rejects)
    return rejected


def window_moments(current):
    """mean and population standard deviation sqrt(max(E[v^2] - m^2, 0)) of the 3 x 3 window (coordinates clamped), and whether all nine are finite"""
    c = np.asarray(current, dtype=np.float64)
    padded = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = c.shape[:2]
    windows = np.stack([padded[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    with np.errstate(invalid="ignore", over="ignore"):
        m = windows.mean(axis=0)
        s = np.sqrt(np.maximum((windows * windows).mean(axis=0) - m * m, 0.0))
    return m, s, np.isfinite(windows).all(axis=0)


def stabilize(passes, motion, sx, sy, alpha, gamma, guides=()):
    offscreen, x0, y0, fx, fy, nx, ny = positions(motion, sx, sy)
    H, W = offscreen.shape
    guide = guide_rejected(guides, nx, ny) & ~offscreen
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    alpha, gamma = np.float64(np.float32(alpha)), np.float64(np.float32(gamma))
    results = []
    for current, history in passes:
        current32 = np.asarray(current, dtype=np.float32)
        c, hist = current32.astype(np.float64), np.asarray(history, dtype=np.float64)
        wx, wy = fx[..., None], fy[..., None]
        with np.errstate(invalid="ignore", over="ignore"):
            h = (hist[y0, x0] * (1 - wx) + hist[y0, x1] * wx) * (1 - wy) + (hist[y1, x0] * (1 - wx) + hist[y1, x1] * wx) * wy
            m, s, finite = window_moments(c)
            lo, hi = m - gamma * s, m + gamma * s
            candidate = ~offscreen & ~guide
            nonfinite = candidate & ~(finite.all(axis=2) & np.isfinite(h).all(axis=2))
            blended = candidate & ~nonfinite
            hc = np.minimum(np.maximum(h, lo), hi)
            blend = c + alpha * (hc - c)
            out = current32.copy()
            out[blended] = blend[blended].astype(np.float32)
            b3 = np.broadcast_to(blended[..., None], c.shape)
            clamped = b3 & ((h < lo) | (h > hi))
            ambiguous = b3 & (np.minimum(np.abs(h - lo), np.abs(h - hi)) < AMBIGUOUS)
            change = np.abs(blend - c)[b3].sum()
            before = np.abs(c - h)[b3].sum()
            after = np.abs(blend - h)[b3].sum()
        results.append({"out": out, "pixels_offscreen": int(offscreen.sum()), "pixels_guide": int(guide.sum()), "pixels_nonfinite": int(nonfinite.sum()),
                        "pixels_blended": int(blended.sum()), "values_clamped": int(clamped.sum()), "change": float(change),
                        "flicker_before": float(before), "flicker_after": float(after), "offscreen": offscreen, "guide": guide,
                        "nonfinite": nonfinite, "blended": blended, "ambiguous": ambiguous, "h": h, "m": m, "s": s})
    return results


# ---------------------------------------------------------------------------------------------------- the generators of the GPU tests
def make_case(H, W, channels, seed, guides=0, sprinkle=False):
    """current = |N(0,1)|, history = current + 0.3 N(0,1), motion on multiples of 1/8 pixel in [-3, 3] (positions, floor and weights are exact in
    fp32), guides on multiples of 0.5 (tolerance 0.25).  channels: the channel count of every pass.  sprinkle: NaN / Inf in the motion, in the
    first pass's current and in the last pass's history.  -> (currents, histories, motion [H,W,3], [(guide current, guide previous, 0.25)])"""
    rng = np.random.default_rng(seed)
    currents = [np.abs(rng.standard_normal((H, W, c))).astype(np.float32) for c in channels]
    histories = [(cur + 0.3 * rng.standard_normal(cur.shape)).astype(np.float32) for cur in currents]
    motion = (rng.integers(-24, 25, size=(H, W, 3)) / 8.0).astype(np.float32)
    if H == 1:                                            # (a frame of one row or column: every second pixel stays on it)
        motion[:, ::2, 1] = 0
    if W == 1:
        motion[::2, :, 0] = 0
    guide_list = []
    for g in range(guides):
        c = 3 if g % 2 == 0 else 1
        yy, xx = np.mgrid[0:H, 0:W]                       # blocks of 8 x 8 pixels: most previous positions (at most 3 pixels away) lie in the pixel's block
        previous = np.repeat((((yy // 8 + xx // 8 + g) % 4) * 0.5)[..., None], c, axis=2).astype(np.float32)
        current = previous.copy()
        flip = rng.random((H, W)) < 0.15
        current[flip] += np.float32(0.5)
        guide_list.append((current, previous, 0.25))
    if sprinkle and H * W >= 16:
        bad = (np.nan, np.inf, -np.inf)
        for k in range(max(H * W // 100, 3)):
            motion[rng.integers(H), rng.integers(W), rng.integers(2)] = bad[k % 3]
            c0, h1 = currents[0], histories[-1]
            c0[rng.integers(H), rng.integers(W), rng.integers(c0.shape[2])] = bad[(k + 1) % 3]
            h1[rng.integers(H), rng.integers(W), rng.integers(h1.shape[2])] = bad[(k + 2) % 3]
        currents[0].view(np.uint32)[rng.integers(H), rng.integers(W), 0] = 0x7fc12345      # a NaN with a payload of its own
    return currents, histories, motion, guide_list
