"""CPU reference of dd_sample_tiles (TEST INFRASTRUCTURE ONLY): a numpy crop of the window, then the oracle's augmentation of one example
(oracle/augment_ref.py, which restates the reference's DataAugmentation.py / Training.py:794-821)."""
import numpy as np

from oracle import augment_ref as A

USAGE_KEYS = ("use_flip_left_right", "use_rotate_90", "use_rgb_permutation", "use_normal_rotation")


def usage_dict(usage):
    """DataAugmentationUsage (or None: everything off) -> the dictionary augment_example takes."""
    return {k: bool(usage is not None and getattr(usage, k)) for k in USAGE_KEYS}


def draw_of(draws, b):
    return {"flip": int(draws["flip"][b]), "rotate": int(draws["rotate"][b]), "permute": int(draws["permute"][b]),
            "normal_rotation": np.asarray(draws["normal_rotation"][b], dtype=np.float32)}


def sample_tile(name, plane, y0, x0, T, draw=None, usage=None):
    """One [T, T, C] tile: plane [h, w, C] float32 cropped at (y0, x0), augmented as pass `name` (draw None: the crop alone)."""
    h, w = plane.shape[:2]
    assert 0 <= y0 <= h - T and 0 <= x0 <= w - T, (y0, x0, h, w, T)
    tile = plane[y0:y0 + T, x0:x0 + T, :]
    if draw is None:
        return np.ascontiguousarray(tile)
    return np.ascontiguousarray(A.augment_example(name, tile, draw, usage_dict(usage)), dtype=np.float32)


def sample_batch(name, planes, records, from_target, T, draws=None, usage=None):
    """[B, T, T, C]: planes = the list of [h, w, C] arrays by plane index, records [B, 4] (source plane, target plane, y0, x0)."""
    out = []
    for b, (sp, tp, y0, x0) in enumerate(np.asarray(records).tolist()):
        out.append(sample_tile(name, planes[tp if from_target else sp], y0, x0, T, None if draws is None else draw_of(draws, b), usage))
    return np.stack(out)
