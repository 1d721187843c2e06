"""Frames: a directory with one .exr per render pass, the feature dictionary the Predictor takes from it, the files written for its
predictions, and the command-line options that say where the files are decoded and encoded."""
import os

import numpy as np

from .codec import ExrError, _image_planes, read_image, write_exr, write_image
from .decode import DeviceDecoder
from .encode import FLOAT, DeviceEncoder, _pixel_type


# ---------------------------------------------------------------------------------------------------- command line
def _add_rule(p, rule):
    """A rule across options of parser `p`: rule(parsed) -> the text of a usage error, or None.  The rules are checked after every parse, in
    the order they were added; the parser's parse_known_args (parse_args goes through it) is wrapped once, with the first of them."""
    if not hasattr(p, "_cross_option_rules"):
        rules = p._cross_option_rules = []
        inner = p.parse_known_args

        def parse_known_args(args=None, namespace=None):
            parsed, rest = inner(args, namespace)
            for check in rules:
                message = check(parsed)
                if message:
                    p.error(message)
            return parsed, rest
        p.parse_known_args = parse_known_args
    p._cross_option_rules.append(rule)


def add_encode_arguments(p):
    """--exr_encode and --exr_type on a parser that has --exr: both only say how <Pass>.exr is written, so `device` (or `half`) without --exr
    is a usage error of the parser."""
    p.add_argument("--exr_encode", default="host", choices=["host", "device"],
                   help="with --exr, where <Pass>.exr is encoded: by the host writer, or on the device by one pack and one deflate launch for all "
                        "passes (the host writes headers, offset tables and the bytes it downloads).")
    p.add_argument("--exr_type", default="float", choices=["float", "half"], help="with --exr, the pixel type of the written channels")
    _add_rule(p, lambda parsed: "--exr_encode device needs --exr" if parsed.exr_encode == "device" and not parsed.exr else None)
    _add_rule(p, lambda parsed: "--exr_type %s needs --exr" % parsed.exr_type if parsed.exr_type != "float" and not parsed.exr else None)


def add_inflate_argument(p, what):
    """--exr_inflate on a parser that has --exr_decode: the device inflates only into the staged buffer of the device decoder, so `device`
    without --exr_decode device is a usage error of the parser."""
    p.add_argument("--exr_inflate", default="host", choices=["host", "device"],
                   help="%s: with --exr_decode device, where the zlib streams of ZIP / ZIPS chunks are inflated: on the host threads, or on the "
                        "device by one launch per batch (the host only reads the files)." % what)
    _add_rule(p, lambda parsed: "--exr_inflate device needs --exr_decode device" if parsed.exr_inflate == "device" and parsed.exr_decode != "device" else None)


# ---------------------------------------------------------------------------------------------------- a directory of render passes
class OpenEXRDirectory:
    """One rendered frame: a directory with one .exr per render pass, matched by '_<Pass>_' in the file name (the underscores keep
    'Normal' and 'Screen Space Normal' apart, OpenEXRDirectory.py:29-53); 1-channel passes keep channel 0 (:66-68).  A missing or
    ambiguous pass and non-finite samples raise ExrError (the reference logs and marks the directory invalid)."""

    def __init__(self, directory):
        self.directory = directory
        self.render_pass_to_image = {}

    def exr_files(self):
        return sorted(os.path.join(self.directory, n) for n in os.listdir(self.directory) if n.endswith(".exr"))

    def file_of(self, render_pass):
        hits = [p for p in self.exr_files() if "_" + render_pass + "_" in os.path.basename(p)]
        if not hits:
            raise ExrError("%s does not contain an exr file for %s" % (self.directory, render_pass))
        if len(hits) > 1:
            raise ExrError("more than one file in %s could be used for the %s pass" % (self.directory, render_pass))
        return hits[0]

    def load_images(self, render_passes, single_channel=()):
        for render_pass in render_passes:
            path = self.file_of(render_pass)
            image = read_image(path)
            if render_pass in single_channel:
                image = image[:, :, 0]
            if not np.isfinite(image).all():
                raise ExrError("there is at least one value in %s which is not finite" % path)
            self.render_pass_to_image[render_pass] = image
        return self.render_pass_to_image

    def size_of_loaded_images(self):
        for image in self.render_pass_to_image.values():
            return image.shape[0], image.shape[1]
        return 0, 0


# ---------------------------------------------------------------------------------------------------- a frame for the Predictor
def load_frame(directory, architecture, device=None, inflate="host"):
    """The feature dictionary Prediction.main builds from a directory of .exr files (Prediction.py:223-252): one [H,W,C] float32 array
    per required feature under 'source_image/0/<Pass>'.  Passes that are not loaded (`load_data` false) are constant 1.0 (colour) or
    0.5 (direct / indirect).  A pass's file is the one whose name contains '_<Pass>_'; the reference's looser rule -- the first
    listed file whose path contains the pass name -- is the fallback, made deterministic by taking the shortest such name.
    With a `device` every pass is a tensor on it: the files are decoded there by one DeviceDecoder.decode call (the same values);
    inflate="device" lets that decoder inflate on the device too."""
    if inflate not in ("host", "device"):
        raise ValueError("inflate=%r (host or device)" % (inflate,))
    if inflate == "device" and device is None:
        raise ValueError("inflate='device' needs a device to decode on")
    from ..naming import Naming
    frame = OpenEXRDirectory(directory)
    files = frame.exr_files()
    features, size = {}, None
    required = list(architecture.auxiliary_features) + list(architecture.feature_predictions)
    loaded = [f for f in required if f.load_data]

    def file_of(f):
        try:
            return frame.file_of(f.name)
        except ExrError:
            loose = sorted((p for p in files if f.name in os.path.basename(p)), key=lambda p: (len(os.path.basename(p)), p))
            if not loose:
                raise ExrError("image for '%s' could not be loaded or does not exist in %s" % (f.name, directory))
            return loose[0]

    def on_host():
        for f in loaded:
            path = file_of(f)
            yield f, path, read_image(path)[..., :f.number_of_channels]

    def on_device():
        paths = [file_of(f) for f in loaded]
        decoded = DeviceDecoder(device, inflate=inflate).decode([(path, f.number_of_channels) for f, path in zip(loaded, paths)])
        for f, path, (image, _) in zip(loaded, paths, decoded):
            yield f, path, image
    for f, path, image in (on_host() if device is None else on_device()):
        if size is None:
            size = tuple(image.shape[:2])
        elif size != tuple(image.shape[:2]):
            raise ExrError("%s is %dx%d, the other passes are %dx%d" % (path, image.shape[1], image.shape[0], size[1], size[0]))
        features[Naming.source_feature_name(f.name, index=0)] = image
    if size is None:
        raise ExrError("no pass of the architecture is loaded from files")
    for f in required:
        if not f.load_data:
            value = 1.0 if f.feature_prediction_type == "COLOR" else 0.5        # Prediction.py:244-249
            shape = size + (f.number_of_channels,)
            if device is None:
                features[Naming.source_feature_name(f.name, index=0)] = np.full(shape, value, dtype=np.float32)
            else:
                import torch
                features[Naming.source_feature_name(f.name, index=0)] = torch.full(shape, value, dtype=torch.float32, device=device)
    return features


def save_predictions(directory, predictions, as_exr=False, encode="host", pixel_type="float", png=False, png_encode="host", exposure=1.0):
    """Prediction.py:483-510 stores every denoised pass and the combined image as <directory>/<Pass>.npy for the Blender side;
    as_exr additionally writes <Pass>.exr.  `predictions`: the dictionary Predictor.predict_frame returns.  encode="device": the .exr
    files of all passes are encoded by one DeviceEncoder.encode call from the tensors where they are (the same planes); pixel_type "half"
    writes HALF channels (the values rounded to nearest even, as numpy's astype(float16)), on either path.  png additionally writes
    <Pass>.png, the 8-bit sRGB picture of the pass times `exposure` (png.py): png_encode="host" by numpy and zlib, "device" by one
    DevicePngEncoder.encode call from the tensors where they are (the same pixels).  With png=False nothing changes."""
    if png_encode not in ("host", "device"):
        raise ValueError("png_encode=%r (host or device)" % (png_encode,))
    if not png and png_encode == "device":
        raise ValueError("png_encode=%r says how the .png files are written: it needs png" % (png_encode,))
    if encode not in ("host", "device"):
        raise ValueError("encode=%r (host or device)" % (encode,))
    kind = _pixel_type(pixel_type)
    if not as_exr and (encode == "device" or kind != FLOAT):
        raise ValueError("encode=%r and pixel_type=%r say how the .exr files are written: they need as_exr" % (encode, pixel_type))
    written, requests, pictures = [], [], []
    for key, value in predictions.items():
        name = key.split("/", 1)[1] if key.startswith("prediction/") else key
        arr = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
        path = os.path.join(directory, name + ".npy")
        np.save(path, arr)
        written.append(path)
        if as_exr:
            exr = os.path.join(directory, name + ".exr")
            if encode == "device":
                if not hasattr(value, "detach"):
                    raise ValueError("encode='device' takes the predictions as device tensors; %s is none" % key)
                requests.append((exr, value if value.shape[-1] == 3 else value[..., 0], kind))
            elif kind == FLOAT:
                write_image(exr, arr if arr.shape[-1] == 3 else arr[..., 0])
            else:
                with np.errstate(over="ignore"):                # (a value past 65504 becomes an infinity: HALF's own rule)
                    image = np.asarray(arr if arr.shape[-1] == 3 else arr[..., 0], dtype=np.float32).astype(np.float16)
                write_exr(exr, _image_planes(image))
            written.append(exr)
        if png:
            pictures.append((name, value if png_encode == "device" else arr))
    if requests:
        import torch
        encoder = DeviceEncoder(requests[0][1].device, threads=16)
        try:
            encoder.encode([(path, image.to(torch.float32), kind) for path, image, kind in requests])
        finally:
            encoder.release()
    if pictures:
        from ..png import save_pngs
        written += save_pngs(directory, pictures, encode=png_encode, exposure=exposure)
    return written
