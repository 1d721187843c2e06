"""`python -m deepdenoiser_amd.compare A B [--exposure E]` -- the quality figures of image A against image B (two .exr / .npy images of equal
size): the table `python -m deepdenoiser_amd.predict --target` prints, for one pair, from one dd_frame_quality call on the device."""
import argparse

import numpy as np
import torch

from . import openexr


def parser():
    p = argparse.ArgumentParser(description="Quality of an image against a reference image (MI355X-native).")
    p.add_argument("image", help="the image to score (.exr or .npy, [H,W], [H,W,1] or [H,W,3])")
    p.add_argument("reference", help="the image it is scored against, of the same size")
    p.add_argument("--exposure", type=float, default=1.0, help="factor in front of the 8-bit sRGB quantisation of psnr_8bit and ssim")
    p.add_argument("--device", default="cuda")
    return p


def load_image(path):
    """.npy as saved by predict ([H,W,C], C = 1 or 3, or [H,W]) or .exr (openexr.read_image: [H,W,3]) -> float32 [H,W,C]"""
    if path.lower().endswith(".npy"):
        image = np.asarray(np.load(path), dtype=np.float32)
        if image.ndim == 2:
            image = image[..., None]
    else:
        image = openexr.read_image(path)
    if image.ndim != 3 or image.shape[2] not in (1, 3):
        raise SystemExit("%s: an [H,W], [H,W,1] or [H,W,3] image is expected, not %s" % (path, image.shape))
    return np.ascontiguousarray(image)


def main(args):
    from . import quality
    a, b = load_image(args.image), load_image(args.reference)
    if a.shape[:2] != b.shape[:2]:
        raise SystemExit("%s is %dx%d, %s is %dx%d" % (args.image, a.shape[1], a.shape[0], args.reference, b.shape[1], b.shape[0]))
    if a.shape[2] != b.shape[2]:      # a 1-channel image against a gray .exr (read as three equal channels)
        a, b = a[..., :1], b[..., :1]
    result = quality.FrameQuality(args.device, exposure=args.exposure).measure({args.image: torch.from_numpy(np.ascontiguousarray(a))},
                                                                               {args.image: torch.from_numpy(np.ascontiguousarray(b))})
    for line in quality.table_lines(result):
        print(line)
    return result


if __name__ == "__main__":
    main(parser().parse_args())
