"""`python -m deepdenoiser_amd.predict architecture.json --input <frame directory>` -- the reference's `python Prediction.py architecture.json
--input dir` (TensorFlow/Prediction.py:23-53 argument set, :188-520 main): the directory's per-pass .exr files -> halo tiles -> forward on the
MI355X path (fp16 MFMA by default) -> crop / stitch / recombination -> <Pass>.npy and Combined.npy next to the inputs."""
import argparse
import json
import multiprocessing
import os

import numpy as np
import torch

from . import openexr, png, tf_checkpoint
from .architecture import Architecture
from .nonfinite import Scanner, mask_to_rgb
from .prediction import Predictor
from .summaries import encode_png


def parser():
    p = argparse.ArgumentParser(description="Prediction for the DeepDenoiser (MI355X-native hot path).")
    p.add_argument("json_filename", help="The json specifying all the relevant details.")
    p.add_argument("--input", type=str, help="Make a prediction for the files in this directory.")
    p.add_argument("--tile_size", default=128, help="Width and heights of the tiles into which the image is split before denoising.")
    p.add_argument("--tile_overlap_size", default=14, help="Border size of the tiles that is overlapping to avoid artifacts.")
    p.add_argument("--threads", default=multiprocessing.cpu_count() + 1, help="Number of threads to use.")
    p.add_argument("--data_format", type=str, default="channels_first", choices=["channels_first", "channels_last"],
                   help="Accepted for compatibility: the MI355X path is NHWC-native, both values give the same results.")
    p.add_argument("--dtype", default="f16", choices=["bf16", "f16", "f32"], help="storage type of activations (f32: the 1e-4 parity path)")
    p.add_argument("--tiles_per_batch", type=int, default=256)
    p.add_argument("--exr", action="store_true", help="also write <Pass>.exr")
    p.add_argument("--nonfinite", default="keep", choices=["keep", "error", "repair"],
                   help="NaN / Inf samples in the input passes: keep them (a whole tile of the output turns NaN), stop with an error that names "
                        "the passes, or repair each from the finite values around it before denoising")
    p.add_argument("--nonfinite_png", action="store_true", help="write <Pass>_nonfinite.png next to the inputs for every pass with NaN / Inf samples")
    p.add_argument("--tile_blend", default="crop", choices=["crop", "feather"],
                   help="how overlapping tiles become the frame: crop keeps one tile's prediction per pixel (the reference's stitch), feather blends "
                        "every tile that covers a pixel with weights that ramp across the overlap, which removes the step along tile borders")
    p.add_argument("--blend_width", type=int, default=None,
                   help="--tile_blend feather: pixels over which a tile's weight ramps at a side that faces another tile (default: twice the overlap; "
                        "0: plain average; at most half a tile)")
    p.add_argument("--exr_decode", default="host", choices=["host", "device"],
                   help="Where the input EXR files are decoded: on the host, or inflated on the host and rebuilt on the device by one launch.")
    openexr.add_inflate_argument(p, "--exr_decode device")
    openexr.add_encode_arguments(p)
    png.add_png_arguments(p)
    p.add_argument("--target", type=str, default=None,
                   help="directory with the ground-truth render of the frame (one .exr per pass): score every denoised pass and Combined against it on "
                        "the device, print one line per pass and write quality.json")
    p.add_argument("--exposure", type=float, default=1.0,
                   help="factor in front of the 8-bit sRGB quantisation: of the pictures --png writes, and of psnr_8bit and ssim of --target (which are "
                        "computed on exactly those pictures)")
    p.add_argument("--quality_json", type=str, default=None, help="--target: where to write the figures (default: quality.json next to the inputs)")
    p.add_argument("--ssim_png", action="store_true", help="--target: write <Pass>_ssim.png, the SSIM map (gray; magenta: a window with a NaN / Inf pixel)")
    return p


def report_quality(args, arch, out):
    """--target: the predictions `out` (still on the device) against the target frame: one dd_frame_quality call, one copy of the records."""
    from . import quality      # (imported here: a run without --target does not load it)
    targets = quality.targets_of_frame(args.target, arch, device=arch.device)
    result = quality.FrameQuality(arch.device, exposure=args.exposure).measure(out, targets, ssim_maps=args.ssim_png)
    maps = {}
    if args.ssim_png:
        result, maps = result
    short = {(k.split("/", 1)[1] if k.startswith("prediction/") else k): v for k, v in result.items()}
    for line in quality.table_lines(short):
        print(line)
    for key, ssim_map in maps.items():
        path = os.path.join(args.input, (key.split("/", 1)[1] if key.startswith("prediction/") else key) + "_ssim.png")
        with open(path, "wb") as f:
            f.write(encode_png(quality.ssim_picture(ssim_map)))
        print(path)
    path = args.quality_json or os.path.join(args.input, "quality.json")
    document = {"tile_size": int(args.tile_size), "tile_overlap_size": int(args.tile_overlap_size), "dtype": args.dtype, "nonfinite": args.nonfinite,
                "tile_blend": args.tile_blend, "exposure": float(args.exposure), "quality": result}
    with open(path, "w") as f:
        json.dump(document, f, indent=1)
    print(path)


def report_nonfinite(source, directory, write_png):
    """One line per affected pass (name, values, pixels); with write_png also <Pass>_nonfinite.png: 8-bit RGB, channel c is 255 where the
    mask bit c is set (a 1-channel pass replicated), from the device mask planes.  `source`: a Predictor or a nonfinite.Scanner."""
    scanner = source._scanner if isinstance(source, Predictor) else source
    masks = scanner.masks()
    for (name, counts), channels in zip(scanner.report().items(), scanner.channels):
        if not counts["values"]:
            continue
        print("%s: %d non-finite values in %d pixels" % (name, counts["values"], counts["pixels"]))
        if write_png:
            path = os.path.join(directory, name.rsplit("/", 1)[-1] + "_nonfinite.png")
            with open(path, "wb") as f:
                f.write(encode_png(mask_to_rgb(masks[name], channels).cpu().numpy()))
            print(path)


def main(args):
    aj = json.load(open(args.json_filename))
    assert os.path.isdir(args.input)
    arch = Architecture(aj, source_data_format="channels_last", data_format=args.data_format, device="cuda", dtype=args.dtype)
    feats = openexr.load_frame(args.input, arch, device=arch.device if args.exr_decode == "device" else None, inflate=args.exr_inflate)      # Prediction.py:223-252
    first = next(iter(feats.values()))
    height, width = first.shape[0], first.shape[1]
    mode = args.nonfinite
    predictor = Predictor(arch, tile_size=int(args.tile_size), tile_overlap_size=int(args.tile_overlap_size), tiles_per_batch=args.tiles_per_batch,
                          nonfinite=mode, tile_blend=args.tile_blend, blend_width=args.blend_width)
    predictor.prepare(height, width)                                               # raises for frames smaller than 16 pixels (Prediction.py:259-261)
    directory = os.path.dirname(os.path.abspath(args.json_filename))
    model_dir = aj["model_directory"] if os.path.isabs(aj["model_directory"]) else os.path.join(directory, aj["model_directory"])
    latest = tf_checkpoint.latest_checkpoint(model_dir) if os.path.isdir(model_dir) else None
    if latest is None:
        raise SystemExit("no checkpoint in %s (train first: python -m deepdenoiser_amd.train ...)" % model_dir)
    tf_checkpoint.load_variables(arch, latest, load_optimizer=False)               # Prediction.py:497-505 restores the Estimator's latest checkpoint
    frame = {k: v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v)) for k, v in feats.items()}
    try:
        out = predictor.predict_frame(frame)
    except ValueError:
        if mode != "error" or predictor._scanner is None:
            raise
        report_nonfinite(predictor, args.input, args.nonfinite_png)
        raise SystemExit("non-finite values in the input passes (--nonfinite repair denoises the frame anyway)")
    if mode == "repair":
        report_nonfinite(predictor, args.input, args.nonfinite_png)
    elif args.nonfinite_png:      # "keep": the prediction is today's; the frame is scanned for the pictures alone
        scanner = Scanner(arch.device, [(k, tuple(v.shape)) for k, v in frame.items()])
        scanner.scan({k: v.to(arch.device) for k, v in frame.items()})
        report_nonfinite(scanner, args.input, True)
    for path in openexr.save_predictions(args.input, out, as_exr=args.exr, encode=args.exr_encode, pixel_type=args.exr_type, png=args.png,
                                         png_encode=args.png_encode, exposure=args.exposure):        # Prediction.py:483-510
        print(path)
    if args.target:
        report_quality(args, arch, out)


if __name__ == "__main__":
    main(parser().parse_args())
