"""How good is a denoised frame?  Full-frame quality figures against the ground-truth render, computed where the frames are
(csrc/dd_quality.hip, include/dd_hip.h: dd_frame_quality).

    quality = FrameQuality(device)                                  # threshold table, records and scratch, cached per (pairs, H, W)
    figures = quality.measure(predictor.predict_frame(frame), targets_of_frame(directory, architecture))
    figures["prediction/Diffuse Color"]["psnr_8bit"], figures["Combined"]["ssim"], ...

Scene-referred figures (mse, mae, rel_mse, smape, max_abs) are taken on the linear radiances; display-referred ones (psnr_8bit, ssim) on the
8-bit sRGB bytes of `exposure * value` -- the bytes of the image summaries (metrics.preview_thresholds).  A pixel with a NaN / Inf channel in
either image is left out of every figure and shows up as pixels - valid_pixels; an SSIM window with such a pixel is left out of ssim."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import frame_launch
from . import metrics as M
from . import openexr
from .naming import Naming

EPSILON = 1e-2                  # LossDifference.py:15: the epsilon of the SMAPE form (and of rel_mse)
TILE = L.QUALITY_TILE           # a workgroup of dd_frame_quality owns TILE x TILE pixels and the windows that start there
WINDOW = 11


class FrameQuality:
    def __init__(self, device, exposure=1.0, epsilon=EPSILON):
        self.lib = L.load()
        self.exposure, self.epsilon = float(exposure), float(epsilon)
        self._thresholds = torch.from_numpy(M.preview_thresholds()).to(torch.device(device))
        self.device = self._thresholds.device      # (with its index: what the tensors of a pair are compared with)
        self._buffers = {}

    def _buffers_of(self, n, H, W):
        key = (n, H, W)
        if key not in self._buffers:
            self._buffers[key] = frame_launch.record_buffers(self.lib.dd_frame_quality_scratch_bytes, L.QualityRecord, n, H, W, self.device)
        return self._buffers[key]

    def launch(self, pairs, ssim_maps=False):
        """pairs: a sequence of (prediction, target) [H,W,C] tensors of one frame size.  One dd_frame_quality call on the current stream, no
        synchronisation: -> (the device records as a uint8 tensor, the list of device SSIM maps or None)."""
        pairs = list(pairs)
        if not 1 <= len(pairs) <= L.QUALITY_MAX_PAIRS:
            raise ValueError("1 .. %d pairs are expected, not %d" % (L.QUALITY_MAX_PAIRS, len(pairs)))
        H, W = int(pairs[0][0].shape[0]), int(pairs[0][0].shape[1])
        table = (L.QualityPair * len(pairs))()
        for i, (p, t) in enumerate(pairs):
            for what, v in (("prediction", p), ("target", t)):
                frame_launch.check_frame("pair %d: the %s" % (i, what), v, H, W, self.device, least=0)      # (the channels: below, on both sides)
            if p.shape[2] != t.shape[2] or p.shape[2] not in (1, 3):
                raise ValueError("pair %d: 1 or 3 channels on both sides are expected, not %d and %d" % (i, p.shape[2], t.shape[2]))
            table[i] = L.QualityPair(p.data_ptr(), t.data_ptr(), p.stride(1), t.stride(1), p.shape[2])
        records, scratch = self._buffers_of(len(pairs), H, W)
        maps, map_ptrs = None, None
        if ssim_maps and H >= WINDOW and W >= WINDOW:
            maps = [torch.empty((H - WINDOW + 1, W - WINDOW + 1), dtype=torch.float32, device=self.device) for _ in pairs]
            map_ptrs = (C.c_void_p * len(pairs))(*[m.data_ptr() for m in maps])
        L.check(self.lib.dd_frame_quality(table, len(pairs), H, W, self._thresholds.data_ptr(), self.exposure, self.epsilon, map_ptrs,
                                          records.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return records, maps

    def measure(self, predictions, targets, ssim_maps=False):
        """predictions, targets: {name: [H,W,C] tensor}; every prediction is scored against the target of its name (a ValueError names the ones
        without).  One launch pair, ONE device-to-host copy (the records: the only synchronisation).  -> {name: figures}, and with
        ssim_maps=True also {name: device [(H-10),(W-10)] map, NaN at invalid windows} (empty for frames without a window)."""
        names = list(predictions)
        missing = [n for n in names if n not in targets]
        if missing:
            raise ValueError("no target for %s" % ", ".join(missing))
        pairs = [(self._resident(predictions[n]), self._resident(targets[n])) for n in names]
        records, maps = self.launch(pairs, ssim_maps)
        recs = frame_launch.read_records(records, L.QualityRecord, len(names))
        out = {n: figures(recs[i], *pairs[i][0].shape) for i, n in enumerate(names)}
        if ssim_maps:
            return out, ({} if maps is None else dict(zip(names, maps)))
        return out

    def _resident(self, v):
        v = torch.as_tensor(v)
        if v.dtype != torch.float32 or v.device != self.device:
            v = v.to(device=self.device, dtype=torch.float32)
        return v if v.dim() == 3 and v.stride(2) == 1 and v.stride(1) >= v.shape[2] and v.stride(0) == v.shape[1] * v.stride(1) else v.contiguous()


def figures(rec, H, W, channels):
    """A dd_quality_record -> the dictionary of measure(): sums over (valid pixels * channels) in float64 on the host."""
    n, nw = int(rec.pixels_valid), int(rec.windows_valid)
    terms = float(n * channels)
    out = {"pixels": H * W, "valid_pixels": n, "windows": max(H - WINDOW + 1, 0) * max(W - WINDOW + 1, 0), "valid_windows": nw}
    for key, value in (("mse", rec.se), ("mae", rec.ae), ("rel_mse", rec.rse), ("smape", rec.smape)):
        out[key] = float(value) / terms if n else None
    out["max_abs"] = float(rec.max_abs) if n else None
    if not n:
        out["psnr_8bit"] = None
    elif rec.ldr_sq_err == 0:
        out["psnr_8bit"] = math.inf
    else:
        out["psnr_8bit"] = 10.0 * math.log10(255.0 ** 2 * terms / float(rec.ldr_sq_err))
    out["ssim"] = float(rec.ssim_sum) / nw if nw else None
    return out


# ---------------------------------------------------------------------------------------------------------------- the target frame
def target_passes(architecture):
    """The passes predict_frame returns a prediction for: the predicted features that are targets and are loaded from files."""
    return [f for f in architecture.feature_predictions if f.is_target and f.load_data]


def target_names(architecture):
    """The keys of targets_of_frame (= the keys of Predictor.predict_frame): 'prediction/<Pass>' per pass, then -- when every member of the
    recombination is among them -- the four combined features and 'Combined'."""
    from .prediction import _COMBINED, RECOMBINE_MEMBERS
    passes = [f.name for f in target_passes(architecture)]
    names = [Naming.feature_prediction_name(n) for n in passes]
    if all(m in passes for m in RECOMBINE_MEMBERS):
        names += [Naming.feature_prediction_name(c) for c in _COMBINED] + ["Combined"]
    return names


def _file_of(frame, files, name, directory):
    """openexr.load_frame's rule: the file whose name contains '_<Pass>_', else the shortest name that contains the pass name."""
    try:
        return frame.file_of(name)
    except openexr.ExrError:
        loose = sorted((p for p in files if name in os.path.basename(p)), key=lambda p: (len(os.path.basename(p)), p))
        if not loose:
            raise openexr.ExrError("image for '%s' could not be loaded or does not exist in %s" % (name, directory))
        return loose[0]


def targets_of_frame(directory, architecture, device="cuda", recombine=True):
    """The target-side twin of openexr.load_frame: {'prediction/<Pass>': float32 [H,W,C]} for every pass of target_passes(), read from the
    directory's .exr files, on `device`; with every member present also the four combined features and 'Combined', formed on the device by
    dd_recombine exactly as Predictor forms them from its predictions.  recombine=False stops after the files (no device work at all when
    device is "cpu")."""
    frame = openexr.OpenEXRDirectory(directory)
    files = frame.exr_files()
    out, whole, size = {}, {}, None
    for f in target_passes(architecture):
        path = _file_of(frame, files, f.name, directory)
        image = openexr.read_image(path)
        if size is None:
            size = image.shape[:2]
        elif size != image.shape[:2]:
            raise openexr.ExrError("%s is %dx%d, the other passes are %dx%d" % (path, image.shape[1], image.shape[0], size[1], size[0]))
        whole[f.name] = torch.from_numpy(np.ascontiguousarray(image)).to(device)
        out[Naming.feature_prediction_name(f.name)] = whole[f.name][..., :f.number_of_channels]
    if size is None:
        raise openexr.ExrError("no predicted pass of the architecture is loaded from files")
    from .prediction import RECOMBINE_MEMBERS, recombine as _recombine
    if recombine and all(m in whole for m in RECOMBINE_MEMBERS):
        out.update(_recombine(L.load(), {m: whole[m] for m in RECOMBINE_MEMBERS}, size[0] * size[1], torch.cuda.current_stream().cuda_stream))
    return out


# ---------------------------------------------------------------------------------------------------------------- reports
COLUMNS = ("mse", "rel_mse", "smape", "psnr_8bit", "ssim")


def table_lines(result):
    """One line per scored image: mse, rel_mse, smape, psnr_8bit, ssim, invalid pixels."""
    def cell(v):
        return "%12s" % "-" if v is None else "%12.6g" % v
    width = max([len(n) for n in result] + [4])
    lines = ["%-*s %s %10s" % (width, "pass", " ".join("%12s" % c for c in COLUMNS), "invalid")]
    for name, r in result.items():
        lines.append("%-*s %s %10d" % (width, name, " ".join(cell(r[c]) for c in COLUMNS), r["pixels"] - r["valid_pixels"]))
    return lines


def ssim_picture(ssim_map):
    """device [h,w] fp32 SSIM map -> uint8 [h,w,3] host array: gray 255 * clamp(ssim, 0, 1), magenta where the window is invalid (NaN)."""
    nan = torch.isnan(ssim_map)
    gray = (torch.nan_to_num(ssim_map, nan=0.0).clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
    rgb = torch.stack([gray, gray, gray], dim=-1)
    rgb[nan] = torch.tensor([255, 0, 255], dtype=torch.uint8, device=rgb.device)
    return rgb.cpu().numpy()
