"""Generates tests/golden/nan_highlighter_golden.npz by EXECUTING the reference's own lines.

TensorFlow/NaNHighlighter.py is a script that imports cv2 and reads its file at import time, so it cannot be imported; its lines 40-42 --
what it computes between reading and writing -- are pure numpy.  This script reads them out of /root/reference AT GENERATION TIME (the way
make_tiling_golden.py does), exec()s them on seeded [H,W,3] float32 arrays with planted NaN / +-inf and records what they gave.

Nothing of the reference's text is embedded here or in the .npz: the committed fixture holds inputs and the outputs the reference code
produced.  Run where /root/reference exists:
    python tests/golden/make_nan_highlighter_golden.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_tiling_golden import HERE, ref_lines  # noqa: E402

HIGHLIGHT = ref_lines("NaNHighlighter.py", 40, 42, ("isfinite", "255"))


def planted(rng, h, w, n_bad):
    image = rng.standard_normal((h, w, 3)).astype(np.float32)
    flat = image.reshape(-1).view(np.uint32)
    # +-inf, quiet and signalling NaNs of either sign; +-FLT_MAX, the smallest denormal and -0 are finite and must stay dark
    bad = np.array([0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff], dtype=np.uint32)
    fine = np.array([0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000000], dtype=np.uint32)
    where = rng.choice(flat.size, size=n_bad + fine.size, replace=False)
    flat[where[:n_bad]] = bad[np.arange(n_bad) % bad.size]
    flat[where[n_bad:]] = fine
    return image


def main():
    rng = np.random.default_rng(20)
    out = {}
    for i, (h, w, n_bad) in enumerate(((1, 2, 1), (5, 7, 9), (16, 23, 40), (9, 4, 0))):
        image = planted(rng, h, w, n_bad)
        ns = {"np": np, "image": image.copy()}
        exec(HIGHLIGHT, ns)
        result = ns["image"]
        assert result.dtype == np.float32 and result.shape == image.shape and set(np.unique(result)) <= {0.0, 255.0}
        out["input_%d" % i] = image
        out["output_%d" % i] = result.astype(np.uint8)
    path = os.path.join(HERE, "nan_highlighter_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d bytes" % (path, len(out) // 2, os.path.getsize(path)))


if __name__ == "__main__":
    main()
