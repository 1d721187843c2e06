"""`python -m deepdenoiser_amd.predict architecture.json --input <frame directory>` -- the reference's `python Prediction.py architecture.json
--input dir` (TensorFlow/Prediction.py:23-53 argument set, :188-520 main): the directory's per-pass .exr files -> halo tiles -> forward on the
MI355X path (fp16 MFMA by default) -> crop / stitch / recombination -> <Pass>.npy and Combined.npy next to the inputs.
`--input_sequence <parent directory>` denoises every frame directory below it in one process with one Predictor; `--temporal` stabilises the
predicted passes of each frame against the previous one before the recombination (temporal.py, DESIGN 3.31: the reference has no such step);
`--target_sequence <parent directory>` scores every written frame against the target frame of its name and the sequence against its targets'
change from frame to frame (sequence_quality.py)."""
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
    p.add_argument("--input_sequence", type=str, default=None,
                   help="Denoise a frame sequence in one process: every sub-directory of this directory that holds .exr files is a frame, ordered by the "
                        "integers in its name, then by name.  Every per-frame option applies to each frame; the outputs go into each frame directory.")
    p.add_argument("--temporal", action="store_true",
                   help="--input_sequence: stabilise every predicted pass against the stabilised previous frame, fetched along the frame's Motion Vector "
                        "pass, before Combined is formed and the files are written; one line per frame and temporal.json at the end")
    p.add_argument("--temporal_alpha", type=float, default=None, help="--temporal: weight of the clamped history in a blended pixel, 0 .. 1 (default 0.8: a "
                                                                      "choice, not a measured optimum)")
    p.add_argument("--temporal_gamma", type=float, default=None, help="--temporal: the history is clamped to mean +- gamma standard deviations of the current "
                                                                      "frame's 3 x 3 neighbourhood (default 1.0: a choice, not a measured optimum)")
    p.add_argument("--motion_scale", type=float, nargs=2, default=None, metavar=("SX", "SY"),
                   help="--temporal, --target_sequence: previous position = (x + SX * motion X, y + SY * motion Y) (default -1 1: an unverified reading "
                        "of Cycles' Vector pass)")
    p.add_argument("--temporal_guide", action="append", default=None, metavar="Pass:tolerance",
                   help="--temporal: do not blend a pixel whose <Pass> differs from the previous frame's at the pixel it came from by more than the "
                        "tolerance (repeatable, at most 4), e.g. Normal:0.25")
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
    p.add_argument("--target_sequence", type=str, default=None,
                   help="--input_sequence: the directory with the ground-truth renders of the sequence, one sub-directory per frame named as the input "
                        "frame's.  Every frame is scored as --target scores it (the table and quality.json in the frame directory; --exposure and "
                        "--ssim_png apply), and from the second frame on against its previous frame along the frame's Motion Vector pass: how much "
                        "the error changes from frame to frame (on what is written: the stabilised passes with --temporal).  One line per pass and "
                        "sequence_quality.json at the end")
    p.add_argument("--sequence_quality_json", type=str, default=None,
                   help="--target_sequence: where to write the figures of the sequence (default: sequence_quality.json in the --input_sequence directory)")
    return p


def short_name(key):
    """'prediction/<Pass>' -> '<Pass>': the name of a pass in the printed tables and in the files next to the inputs."""
    return key.split("/", 1)[1] if key.startswith("prediction/") else key


def run_parameters(args):
    """The options that decide what was scored, as quality.json and sequence_quality.json record them."""
    return {"tile_size": int(args.tile_size), "tile_overlap_size": int(args.tile_overlap_size), "dtype": args.dtype, "nonfinite": args.nonfinite,
            "tile_blend": args.tile_blend, "exposure": float(args.exposure)}


def report_quality(args, arch, out, directory=None, targets=None, json_path=None, scorer=None):
    """--target: the predictions `out` (still on the device) against the target frame: one dd_frame_quality call, one copy of the records.
    directory: where the pictures and quality.json go (default: --input); targets: the loaded target frame (default: --target's); json_path: of the
    json (default: --quality_json, else quality.json in the directory); scorer: a FrameQuality to reuse.  -> the figures."""
    from . import quality      # (imported here: a run without --target does not load it)
    directory = args.input if directory is None else directory
    if targets is None:
        targets = quality.targets_of_frame(args.target, arch, device=arch.device)
    scorer = scorer or quality.FrameQuality(arch.device, exposure=args.exposure)
    result = scorer.measure(out, targets, ssim_maps=args.ssim_png)
    maps = {}
    if args.ssim_png:
        result, maps = result
    for line in quality.table_lines({short_name(k): v for k, v in result.items()}):
        print(line)
    for key, ssim_map in maps.items():
        path = os.path.join(directory, short_name(key) + "_ssim.png")
        with open(path, "wb") as f:
            f.write(encode_png(quality.ssim_picture(ssim_map)))
        print(path)
    path = json_path or args.quality_json or os.path.join(directory, "quality.json")
    with open(path, "w") as f:
        json.dump(dict(run_parameters(args), quality=result), f, indent=1)
    print(path)
    return result


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


TEMPORAL_OPTIONS = ("temporal_alpha", "temporal_gamma", "motion_scale", "temporal_guide")


def check_option_rules(args):
    """The rules across options that the parser does not know (tests parse ["a.json"] alone): -> the text of the usage error, or None."""
    sequence = getattr(args, "input_sequence", None)
    if (args.input is None) == (sequence is None):
        return "exactly one of --input / --input_sequence must be given"
    target_sequence = getattr(args, "target_sequence", None)
    if target_sequence is not None and sequence is None:
        return "--target_sequence needs --input_sequence"
    temporal_options = [o for o in TEMPORAL_OPTIONS if getattr(args, o, None) is not None]
    if (getattr(args, "temporal", False) or temporal_options) and sequence is None:
        return "--temporal and its options need --input_sequence"
    if target_sequence is not None and not getattr(args, "temporal", False):      # (the scorer follows the motion vectors too)
        temporal_options = [o for o in temporal_options if o != "motion_scale"]
    if temporal_options and not getattr(args, "temporal", False):
        return "%s need%s --temporal" % (", ".join("--" + o for o in temporal_options), "s" if len(temporal_options) == 1 else "")
    if args.target and sequence is not None:
        return "--target needs --input (scoring sequences is out of scope)"
    return None


class Run:
    """What the frames of one process share: the architecture, the Predictor (plan, program and graph per frame size) and the loaded weights."""

    def __init__(self, args):
        self.args = args
        self.aj = json.load(open(args.json_filename))
        self.arch = Architecture(self.aj, source_data_format="channels_last", data_format=args.data_format, device="cuda", dtype=args.dtype)
        self.predictor = Predictor(self.arch, tile_size=int(args.tile_size), tile_overlap_size=int(args.tile_overlap_size),
                                   tiles_per_batch=args.tiles_per_batch, nonfinite=args.nonfinite, tile_blend=args.tile_blend, blend_width=args.blend_width)
        self.loaded = False

    def load_weights(self):
        if self.loaded:
            return
        directory = os.path.dirname(os.path.abspath(self.args.json_filename))
        model_dir = self.aj["model_directory"] if os.path.isabs(self.aj["model_directory"]) else os.path.join(directory, self.aj["model_directory"])
        latest = tf_checkpoint.latest_checkpoint(model_dir) if os.path.isdir(model_dir) else None
        if latest is None:
            raise SystemExit("no checkpoint in %s (train first: python -m deepdenoiser_amd.train ...)" % model_dir)
        tf_checkpoint.load_variables(self.arch, latest, load_optimizer=False)      # Prediction.py:497-505 restores the Estimator's latest checkpoint
        self.loaded = True


def load_passes(directory, names, args, device):
    """--temporal, --target_sequence: the [H,W,3] device tensors of the passes `names` of a frame directory, by the '_<Pass>_' file rule, decoded
    where --exr_decode says.  A frame without one of them is an ExrError that names the directory."""
    frame = openexr.OpenEXRDirectory(directory)
    paths = [frame.file_of(name) for name in names]
    if args.exr_decode == "device":
        decoded = openexr.DeviceDecoder(device, inflate=args.exr_inflate).decode([(path, 3) for path in paths])
        return {name: image for name, (image, _) in zip(names, decoded)}
    return {name: torch.from_numpy(np.ascontiguousarray(openexr.read_image(path))).to(device) for name, path in zip(names, paths)}


def stabilise(run, stabilizer, passes, out):
    """--temporal: the predicted passes of `out` through the stabiliser, then Combined and the four combined features from the STABILISED
    members (prediction.recombine), so that what is written stays consistent with its parts.  passes: the frame's Motion Vector and guide
    passes (load_passes).  -> the dictionary to write, in out's order."""
    from .naming import Naming
    from .prediction import RECOMBINE_MEMBERS, recombine
    arch = run.arch
    guide_names = [g for g, _ in stabilizer.guides]
    members = [Naming.feature_prediction_name(f.name) for f in arch.feature_predictions if f.is_target and f.load_data]
    stable = stabilizer.stabilize({k: out[k] for k in members}, passes["Motion Vector"], {g: passes[g] for g in guide_names})
    result = dict(stable)
    if all(Naming.feature_prediction_name(m) in stable for m in RECOMBINE_MEMBERS):
        first = stable[members[0]]
        result.update(recombine(run.predictor.lib, {m: stable[Naming.feature_prediction_name(m)] for m in RECOMBINE_MEMBERS},
                                first.shape[0] * first.shape[1], torch.cuda.current_stream().cuda_stream))
    return {k: result[k] for k in out}


class SequenceScore:
    """--target_sequence: what the frames of the run share (the two scorers) and what they leave (the figures per frame)."""

    def __init__(self, args, device):
        from . import quality, sequence_quality
        self.parent = args.target_sequence
        self.frame_quality = quality.FrameQuality(device, exposure=args.exposure)
        self.sequence_quality = sequence_quality.SequenceQuality(device, exposure=args.exposure, motion_scale=args.motion_scale)
        self.frames = []

    @staticmethod
    def check_directories(parent, directories):
        """Every frame directory needs a sub-directory of its name under `parent` with .exr files: -> the first one that is missing, or None."""
        for d in directories:
            t = os.path.join(parent, os.path.basename(d))
            if not (os.path.isdir(t) and any(n.endswith(".exr") for n in os.listdir(t))):
                return t
        return None

    def score(self, run, directory, out, motion):
        """The frame as --target scores it (into the frame directory), then against the previous frame along `motion`."""
        from . import quality
        args, arch = run.args, run.arch
        targets = quality.targets_of_frame(os.path.join(self.parent, os.path.basename(directory)), arch, device=arch.device)
        result = report_quality(args, arch, out, directory=directory, targets=targets, json_path=os.path.join(directory, "quality.json"), scorer=self.frame_quality)
        temporal_quality = self.sequence_quality.measure(out, targets, motion)
        self.frames.append({"directory": os.path.basename(directory), "quality": result, "temporal_quality": temporal_quality})

    def document(self, args, stabilizer):
        measured = self.sequence_quality.summary()
        summary = {}
        for name in (self.frames[0]["quality"] if self.frames else {}):
            means = {}
            for key in self.frames[0]["quality"][name]:
                values = [f["quality"][name][key] for f in self.frames if f["quality"].get(name, {}).get(key) is not None]
                means[key] = sum(values) / len(values) if values else None
            summary[name] = {"temporal_quality": measured.get(name), "quality": means}
        parameters = run_parameters(args)      # (this document begins with the exposure and the motion scale)
        return {"exposure": parameters.pop("exposure"), "motion_scale": list(self.sequence_quality.motion_scale), **parameters,
                "temporal": stabilizer.parameters() if stabilizer is not None else None, "frames": self.frames, "summary": summary}


def denoise_frame(run, directory, stabilizer=None, score=None):
    """One frame directory: its .exr files -> the prediction -> <Pass>.npy (and what the options add) next to the inputs.  score: the
    SequenceScore of a --target_sequence run.  -> the stabiliser's report of the frame, or None."""
    args, arch, predictor = run.args, run.arch, run.predictor
    feats = openexr.load_frame(directory, arch, device=arch.device if args.exr_decode == "device" else None, inflate=args.exr_inflate)      # Prediction.py:223-252
    first = next(iter(feats.values()))
    height, width = first.shape[0], first.shape[1]
    mode = args.nonfinite
    predictor.prepare(height, width)                                               # raises for frames smaller than 16 pixels (Prediction.py:259-261)
    run.load_weights()
    frame = {k: v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v)) for k, v in feats.items()}
    try:
        out = predictor.predict_frame(frame)
    except ValueError:
        if mode != "error" or predictor._scanner is None:
            raise
        report_nonfinite(predictor, directory, args.nonfinite_png)
        raise SystemExit("non-finite values in the input passes (--nonfinite repair denoises the frame anyway)")
    if mode == "repair":
        report_nonfinite(predictor, directory, args.nonfinite_png)
    elif args.nonfinite_png:      # "keep": the prediction is today's; the frame is scanned for the pictures alone
        scanner = Scanner(arch.device, [(k, tuple(v.shape)) for k, v in frame.items()])
        scanner.scan({k: v.to(arch.device) for k, v in frame.items()})
        report_nonfinite(scanner, directory, True)
    report, passes = None, None
    if stabilizer is not None or score is not None:      # the Motion Vector pass of the INPUT frame, once for both
        passes = load_passes(directory, ["Motion Vector"] + ([g for g, _ in stabilizer.guides] if stabilizer is not None else []), args, arch.device)
    if stabilizer is not None:
        out = stabilise(run, stabilizer, passes, out)
        report = stabilizer.report()
    for path in openexr.save_predictions(directory, out, as_exr=args.exr, encode=args.exr_encode, pixel_type=args.exr_type, png=args.png,
                                         png_encode=args.png_encode, exposure=args.exposure):        # Prediction.py:483-510
        print(path)
    if args.target:
        report_quality(args, arch, out)
    if score is not None:
        score.score(run, directory, out, passes["Motion Vector"])
    return report


def temporal_line(directory, report):
    """One line per frame of a --temporal run: the pixels blended of the first pass's categories and the flicker over all passes."""
    first = next(iter(report.values()))
    pixels = sum(first[k] for k in ("pixels_offscreen", "pixels_guide", "pixels_nonfinite", "pixels_blended"))
    before = [r["flicker_before"] for r in report.values() if r["flicker_before"] is not None]
    after = [r["flicker_after"] for r in report.values() if r["flicker_after"] is not None]
    if not before:
        return "%s: passed through (the first frame of the history)" % directory
    return ("%s: %d of %d pixels blended, %d offscreen, %d rejected by a guide, %d non-finite (%s); mean |frame - history| %.6g -> %.6g over %d passes"
            % (directory, first["pixels_blended"], pixels, first["pixels_offscreen"], first["pixels_guide"], first["pixels_nonfinite"],
               next(iter(report)), sum(before) / len(before), sum(after) / len(after), len(before)))


def main(args):
    message = check_option_rules(args)
    if message:
        raise SystemExit(message)
    if args.input is not None:
        assert os.path.isdir(args.input)
        denoise_frame(Run(args), args.input)
        return
    from . import temporal
    assert os.path.isdir(args.input_sequence)
    directories = temporal.frame_directories(args.input_sequence)
    if not directories:
        raise SystemExit("no sub-directory of %s holds .exr files" % args.input_sequence)
    target_sequence = getattr(args, "target_sequence", None)
    if target_sequence is not None:
        from .sequence_quality import table_lines
        missing = SequenceScore.check_directories(target_sequence, directories)
        if missing:
            raise SystemExit("--target_sequence: no target frame directory %s with .exr files" % missing)
    stabilizer = None
    if args.temporal:
        try:
            guides = [temporal.parse_guide(g) for g in (args.temporal_guide or [])]
            stabilizer = temporal.TemporalStabilizer("cuda", alpha=0.8 if args.temporal_alpha is None else args.temporal_alpha,
                                                     gamma=1.0 if args.temporal_gamma is None else args.temporal_gamma,
                                                     motion_scale=args.motion_scale, guides=guides)
        except ValueError as e:
            raise SystemExit("--temporal: %s" % e)
    run = Run(args)
    score = SequenceScore(args, "cuda") if target_sequence is not None else None
    reports = [(d, denoise_frame(run, d, stabilizer, score)) for d in directories]
    if stabilizer is not None:
        for d, report in reports:
            print(temporal_line(d, report))
        path = os.path.join(args.input_sequence, "temporal.json")
        with open(path, "w") as f:
            json.dump(dict(stabilizer.parameters(), frames=[{"directory": os.path.basename(d), "passes": report} for d, report in reports]), f, indent=1)
        print(path)
    if score is not None:
        document = score.document(args, stabilizer)
        measured = {short_name(k): v["temporal_quality"] for k, v in document["summary"].items() if v["temporal_quality"] is not None}
        for line in table_lines(measured):
            print(line)
        path = args.sequence_quality_json or os.path.join(args.input_sequence, "sequence_quality.json")
        with open(path, "w") as f:
            json.dump(document, f, indent=1)
        print(path)


if __name__ == "__main__":
    main(parser().parse_args())
