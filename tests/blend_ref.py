"""Reference of the feathered tile blend (tile_blend="feather"), numpy float64, written from its definition and independent of
deepdenoiser_amd.tiling.blend_weights: loops over coordinates and over ALL tiles that cover them, no vectorised shortcut.

An axis is (origins, tile, extent): tile i covers the image coordinates origins[i] .. origins[i] + tile - 1.

  raw_i(t)  = min(lo, hi)
              lo = 1 if origins[i] == 0 (the tile lies at the frame border: no ramp there), else min(1, (t + 0.5) / width)
              hi = 1 if origins[i] + tile == extent,                                        else min(1, (tile - t - 0.5) / width)
              width == 0: 1
  w_i(t)    = raw_i(t) / sum of raw_k(p - origins[k]) over every tile k that covers p = origins[i] + t
  out[y, x] = sum over the covering tile rows i (ascending), columns j (ascending) of wy_i(y - oy_i) * wx_j(x - ox_j) * tile_(i, j)[y - oy_i, x - ox_j]
"""
import numpy as np


def raw_weight(origin, t, tile, extent, width):
    if width == 0:
        return 1.0
    lo = 1.0 if origin == 0 else min(1.0, (t + 0.5) / width)
    hi = 1.0 if origin + tile == extent else min(1.0, (tile - t - 0.5) / width)
    return min(lo, hi)


def covering(origins, tile, p):
    """indices of the tiles whose interval contains the image coordinate p"""
    return [k for k, o in enumerate(origins) if o <= p < o + tile]


def axis_weights(origins, tile, extent, width):
    """float64 [len(origins), tile]"""
    out = np.zeros((len(origins), tile), dtype=np.float64)
    for i, o in enumerate(origins):
        for t in range(tile):
            p = o + t
            total = sum(raw_weight(origins[k], p - origins[k], tile, extent, width) for k in covering(origins, tile, p))
            out[i, t] = raw_weight(o, t, tile, extent, width) / total
    return out


def cover_counts(origins, tile, extent):
    """how many tiles cover each image coordinate"""
    return np.array([len(covering(origins, tile, p)) for p in range(extent)])


def blend(tiles, oy, ox, tile, height, width, ramp_y, ramp_x):
    """tiles: [len(oy) * len(ox), tile, tile, C] in row-major tile order -> float64 [height, width, C]"""
    tiles = np.asarray(tiles, dtype=np.float64)
    wy, wx = axis_weights(oy, tile, height, ramp_y), axis_weights(ox, tile, width, ramp_x)
    out = np.zeros((height, width, tiles.shape[-1]), dtype=np.float64)
    for i, y0 in enumerate(oy):
        for j, x0 in enumerate(ox):
            out[y0:y0 + tile, x0:x0 + tile] += (wy[i][:, None] * wx[j][None, :])[..., None] * tiles[i * len(ox) + j]
    return out


def seam_statistic(diff, seam_columns, seam_rows):
    """diff: [H, W, C] = tiled output - untiled output.  Mean |diff[:, x] - diff[:, x - 1]| over the seam columns x (all rows and channels),
    and mean |diff[y] - diff[y - 1]| over the seam rows y: the step a tile border leaves, the image's own gradient cancelled by the difference."""
    diff = np.asarray(diff, dtype=np.float64)
    cols = np.mean([np.abs(diff[:, x] - diff[:, x - 1]).mean() for x in seam_columns])
    rows = np.mean([np.abs(diff[y] - diff[y - 1]).mean() for y in seam_rows])
    return float(cols), float(rows)


# ---- the seam measurement shared by tests/test_tile_blend_host.py (float64 oracle) and tests/test_gpu_tile_blend.py (device)
SEAM_FRAME, SEAM_TILE, SEAM_OVERLAP, SEAM_SEED, SEAM_FACTOR = 96, 48, 6, 2, 0.5


def seam_architecture():
    from deepdenoiser_amd import configs
    return configs.cfg2_unet_kpcn(filters=(16, 24, 32), convs=2)


def seam_frame(features, seed=11, cell=16):
    """features: (name, channels) pairs -> {source name: [96, 96, channels] float32 tensor}.  A SMOOTH frame: seeded noise on a grid of
    `cell`-pixel cells, bicubically enlarged (passes other than normals made non-negative).  On white noise the difference between a tile's
    prediction and the untiled one is itself white -- the kernel-prediction head weighs noisy source pixels -- and no blend can halve a
    pixel-to-pixel difference that is there on both sides of a border as well as across it (measured on the float64 oracle: 0.83 - 0.95 of
    the crop's); on a smooth frame that difference varies slowly inside a tile and jumps at the border, which is the case the blend is for."""
    import torch
    from deepdenoiser_amd.naming import Naming
    g = torch.Generator().manual_seed(seed)
    n = SEAM_FRAME
    frame = {}
    for name, channels in features:
        v = torch.randn(1, channels, n // cell, n // cell, generator=g)
        v = torch.nn.functional.interpolate(v, size=(n, n), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).contiguous()
        frame[Naming.source_feature_name(name, index=0)] = v if "Normal" in name else v.abs()
    return frame
