"""The bytes of the files the two device encoders write (openexr.DeviceEncoder, png.DevicePngEncoder) for seeded planes, as one sha256 per file,
with the launch and raw counters of every encode call.  Two trees that print the same lines write the same files with the same launches: run
it once in each (it uses only DeviceEncoder(...).encode and DevicePngEncoder(..., segment_rows=...).encode and the counters).

    python tools/encoder_bits.py [--out FILE]

Planes are built on the host (numpy, fixed seeds).  The small batch: 37 x 21 RGB smooth, 1 x 1 gray, 20 x 13 RGB noise, 64 x 257 RGB smooth with
mild noise; for PNG also 3 x 4096 RGB, the widest row the pack kernel holds.  EXR: ZIP, ZIPS and NONE, each as float and as half.  PNG: the
default segments and one row per segment.  Then one realistic batch per encoder: 15 passes of 270 x 480 (12 RGB, 3 gray)."""
import argparse
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepdenoiser_amd import _lib, openexr, png  # noqa: E402


def smooth(rng, H, W, n, noise):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.05 + 0.6 * x / max(W, 2) + 0.2 * (c + 1) * y / max(H, 2) for c in range(n)], axis=-1).astype(np.float32)
    img = (img + noise * rng.standard_normal(img.shape).astype(np.float32)).astype(np.float32)
    return img if n == 3 else img[..., 0]


def small_batch(rng, widest):
    planes = [smooth(rng, 37, 21, 3, 1e-6), np.full((1, 1), 0.18, dtype=np.float32), rng.random((20, 13, 3), dtype=np.float32), smooth(rng, 64, 257, 3, 0.01)]
    if widest:
        planes.append(smooth(rng, 3, 4096, 3, 0.02))
    return planes


def realistic_batch(rng):
    return [smooth(rng, 270, 480, 3 if k < 12 else 1, 0.004 * (1 + k % 3)) for k in range(15)]


def shape_of(plane):
    return "x".join(str(s) for s in plane.shape)


def run(label, encoder, planes, requests, raw):
    """one encode call -> its lines: a digest per file, then the counters"""
    written = encoder.encode(requests)
    assert written == [r[0] for r in requests]
    lines = ["%-22s %-10s %s" % (label, shape_of(p), hashlib.sha256(open(path, "rb").read()).hexdigest()) for p, path in zip(planes, written)]
    lines.append("%-22s pack_launches %d deflate_launches %d %s %d downloaded_bytes %d" % (label, encoder.pack_launches, encoder.deflate_launches, raw,
                                                                                          getattr(encoder, raw), encoder.downloaded_bytes))
    encoder.release()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also append the printed lines to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print("library %s" % _lib.load().dd_version().decode(), file=sys.stderr)      # (names the tree: not one of the lines to compare)
    lines = []
    with tempfile.TemporaryDirectory() as root:
        def requests(planes, suffix, last):
            return [(os.path.join(root, "f%02d.%s" % (k, suffix)), torch.from_numpy(np.ascontiguousarray(p)).cuda(), last) for k, p in enumerate(planes)]
        for name, compression in (("zip", openexr.ZIP_COMPRESSION), ("zips", openexr.ZIPS_COMPRESSION), ("none", openexr.NO_COMPRESSION)):
            for kind in ("float", "half"):
                planes = small_batch(np.random.default_rng(1), False)
                lines += run("exr %s %s" % (name, kind), openexr.DeviceEncoder("cuda", compression=compression), planes, requests(planes, "exr", kind), "raw_chunks")
        for segment_rows in (None, 1):
            planes = small_batch(np.random.default_rng(2), True)
            lines += run("png segment_rows=%s" % segment_rows, png.DevicePngEncoder("cuda", segment_rows=segment_rows), planes, requests(planes, "png", 1.0),
                         "raw_segments")
        planes = realistic_batch(np.random.default_rng(3))
        lines += run("exr zip float 15 passes", openexr.DeviceEncoder("cuda", threads=16), planes, requests(planes, "exr", "float"), "raw_chunks")
        lines += run("png 15 passes", png.DevicePngEncoder("cuda", threads=16), planes, requests(planes, "png", 1.0), "raw_segments")
    for line in lines:
        print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
