"""`python -m deepdenoiser_amd.nan_highlighter exr_filename [--output png]` -- the reference's `python NaNHighlighter.py exr_filename
[--output png]` (TensorFlow/NaNHighlighter.py:10-26 argument set): a PNG of the .exr in which channel c of a pixel is 255 where that channel
is NaN / Inf and 0 elsewhere (:40-42), written to --output or to the input's name with .png.

One file on the host; no GPU is needed (a whole frame in device memory is scanned by nonfinite.Scanner).  The reference converts BGR -> RGB
after reading (:35) and RGB -> BGR before writing (:44); between the two stands a channel-wise operation, so the round trip cancels and the
PNG's R, G, B are the .exr's R, G, B -- which is what openexr.read_image and summaries.encode_png give without either conversion."""
import argparse
import os

import numpy as np

from . import openexr
from .summaries import encode_png


def parser():
    p = argparse.ArgumentParser(description="Highlight NaN/Inf in exr files.")
    p.add_argument("exr_filename", help="The exr in which the NaN/Inf pixels need to be found.")
    p.add_argument("--output", type=str, help="The png where the pixels are highlighted.")
    return p


def highlight(image):
    """float [H,W,3] -> uint8 [H,W,3]: 255 where the value is not finite."""
    return (255.0 * np.logical_not(np.isfinite(image)).astype(np.float32)).astype(np.uint8)


def main(args):
    png_filename = args.output if isinstance(args.output, str) else os.path.splitext(args.exr_filename)[0] + ".png"
    with open(png_filename, "wb") as f:
        f.write(encode_png(highlight(openexr.read_image(args.exr_filename)), level=9))
    return png_filename


if __name__ == "__main__":
    main(parser().parse_known_args()[0])
