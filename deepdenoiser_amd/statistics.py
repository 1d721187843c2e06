"""Data-set statistics of a frame set, reduced on the device: <mode>_statistics.json without TensorFlow and without a tile set on disk.

    python -m deepdenoiser_amd.statistics tfrecords.json [--mode M ...] [--output DIR] [--frame_memory_gb X] [--threads N] [--exr_decode {host,device}] [--exr_inflate {host,device}]

The reference makes the file with `python TFRecordsCreator.py tfrecords.json --statistics` (TFRecordsStatistics.py, FeatureStatistics.py): two
sweeps over the tiles it wrote to disk, in TensorFlow 1.x eager mode.  Here the rendered EXR frames are the data set (frame_bank.py): the
scenes are loaded into device memory in chunks that fit, ONE dd_tile_statistics launch per chunk (csrc/dd_frame_statistics.hip) reduces every
window of the reference's tile grid (TFRecordsCreator.py:125-133) and every pass to a row of doubles, and the rows are joined on the host in
float64 by the reference's rules (TFRecordsStatistics.py:236-316 per tile, :143-221 over the tiles), its quirks included:

    minimum, maximum      over every sample of every window -- also for the ' Masked' entries (:255-256)
    mean                  the mean over windows of the per-window mean over all samples (:275, :150)
    coverage              the mean over windows of  pixels with sum_c |x_c| != 0  /  T * T  (:277-281; Alpha: x - 1 in place of x)
    variance              the mean over windows of the per-window mean of (x - mean)^2, `mean` being the global one above (:315, :201)
    ' Masked' entries     for direct / indirect passes that are no volume passes (:68-70), m = the non-black mask of the target colour pass
                          RenderPasses.direct_or_indirect_to_color_render_pass names (:246-248).  Per window with mask_sum = sum m > 0:
                          mean sum(x m) / mask_sum -- a sum over three channels divided by PIXELS (:258); coverage count / mask_sum with
                          the count over all pixels (:261-265); variance sum((x - mean)^2 m) / mask_sum (:309).  Windows with
                          mask_sum == 0 contribute nothing; an empty list gives 0 (:148-149, :199-200)
    statistics_log1p      the same on l = sign(x) log1p(|x|), with the raw coverage (:216-218)

Source entries aggregate every samples-per-pixel count of the list and every source index (:115-116); a mode with
group_by_samples_per_pixel gets one file per count (:30-34, :227-228).  One deliberate deviation: TFRecordsStatistics.py:132 and :185 pass
`source_feature` where `target_feature` is meant, so the reference's unmasked target_image/<Pass> entries describe the last source pass; here
they are computed from the target pass.

The variance about a mean that is known only after the last window comes from the kernel's SHIFTED sums (pivot K = the window's first
sample):  sum (x - mean)^2 = sum (x - K)^2 - 2 (mean - K) sum (x - K) + n (mean - K)^2,  so every plane is read once.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

from . import _lib as L
from .naming import Naming
from .render_passes import RenderPasses

F = {name: k for k, name in enumerate(L.STAT_FIELD_NAMES)}      # field name -> column of a row
WINDOW_DTYPE = np.dtype([("plane", "<i4"), ("mask_plane", "<i4"), ("y0", "<i4"), ("x0", "<i4")])
assert WINDOW_DTYPE.itemsize == C.sizeof(L.StatWindow)
TARGET = -1      # `spp_index` of a target window


def has_masked_entry(render_pass):
    return RenderPasses.is_direct_or_indirect_render_pass(render_pass) and not RenderPasses.is_volume_render_pass(render_pass)


def window_table(sizes, tile, n_spps, sources):
    """The windows of scenes of `sizes` [(height, width)]: for every scene and every grid tile (h // T by w // T, remainders dropped,
    TFRecordsCreator.py:125-133) one window per source rendering -- for each samples-per-pixel count, each source index -- masked by the
    scene's target plane, then one for the target plane.  Planes as FrameBank.for_passes lays them out.
    -> (windows [n] WINDOW_DTYPE, spp_index [n] int: the position of the window's count in the list, TARGET for a target window)"""
    per_scene = n_spps * sources + 1
    windows, spp_index = [], []
    for s, (h, w) in enumerate(sizes):
        target = s * per_scene + per_scene - 1
        for i in range(h // tile):
            for j in range(w // tile):
                for k in range(n_spps):
                    for index in range(sources):
                        windows.append((s * per_scene + k * sources + index, target, i * tile, j * tile))
                        spp_index.append(k)
                windows.append((target, target, i * tile, j * tile))
                spp_index.append(TARGET)
    return np.array(windows, dtype=WINDOW_DTYPE).reshape(-1), np.asarray(spp_index, dtype=np.int64).reshape(-1)


def chunk_scenes(scenes, bytes_per_pixel, memory_limit_bytes):
    """Consecutive scenes in groups whose planes fit `memory_limit_bytes` (None: one group); a scene that does not fit alone stands alone (the
    bank then refuses it by name of the limit)."""
    if memory_limit_bytes is None:
        return [list(scenes)] if scenes else []
    chunks, size = [], 0
    for scene in scenes:
        need = scene.height * scene.width * bytes_per_pixel
        if not chunks or size + need > memory_limit_bytes:
            chunks.append([])
            size = 0
        chunks[-1].append(scene)
        size += need
    return chunks


def _mean(values):
    return float(np.mean(values)) if len(values) else 0.0      # TFRecordsStatistics.py:148-149: an empty list gives 0


def _moments(rows, suffix, samples, channels, masked):
    """(mean, variance) of one entry from its windows' rows; suffix '' or '_log1p'."""
    K = rows[:, F["pivot" + suffix]]
    if not masked:
        s1, s2 = rows[:, F["sum" + suffix]], rows[:, F["sum_sq" + suffix]]
        mean = _mean(K + s1 / samples)
        d = mean - K
        return mean, _mean((s2 - 2.0 * d * s1 + samples * d * d) / samples)
    keep = rows[:, F["mask_sum"]] > 0
    K, ms = K[keep], rows[keep, F["mask_sum"]]
    s1, s2 = rows[keep, F["masked_sum" + suffix]], rows[keep, F["masked_sum_sq" + suffix]]
    mean = _mean(s1 / ms + channels * K)                         # sum over the channels of x m, divided by the mask's PIXELS
    d = mean - K
    return mean, _mean((s2 - 2.0 * d * s1 + channels * ms * d * d) / ms)


def join_entry(rows, tile, channels, masked):
    """One entry of the file from the rows [n, STAT_FIELDS] of its windows (rows marked absent are dropped)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, L.STAT_FIELDS)
    rows = rows[rows[:, F["present"]] != 0]
    pixels = tile * tile
    samples = pixels * channels
    if masked:
        keep = rows[:, F["mask_sum"]] > 0
        coverage = _mean(rows[keep, F["count"]] / rows[keep, F["mask_sum"]])
    else:
        coverage = _mean(rows[:, F["count"]] / pixels)
    out = {"number_of_channels": channels}
    for key, suffix in (("statistics", ""), ("statistics_log1p", "_log1p")):
        mean, variance = _moments(rows, suffix, samples, channels, masked)
        out[key] = {"minimum": float(rows[:, F["min" + suffix]].min()) if len(rows) else float("inf"),
                    "maximum": float(rows[:, F["max" + suffix]].max()) if len(rows) else float("-inf"),
                    "mean": mean, "variance": variance, "coverage": coverage}
    return out


class FrameStatistics:
    """The statistics of `frame_set` (frame_bank.FrameSet).  `passes`: the slots of a launch, the union of the source and target passes;
    `compute` fills `rows` [n_windows, n_passes, STAT_FIELDS] and `spp_index` [n_windows]; `results` joins them."""

    def __init__(self, frame_set, group_by_samples_per_pixel=False):
        self.frame_set, self.group = frame_set, bool(group_by_samples_per_pixel)
        self.tile, self.sources, self.spps = frame_set.tile, frame_set.number_of_sources_per_example, list(frame_set.source_spps)
        self.source_passes, self.target_passes = list(frame_set.source_passes), list(frame_set.target_passes)
        self.passes = self.source_passes + [p for p in self.target_passes if p not in self.source_passes]
        if not 1 <= len(self.passes) <= L.STAT_MAX_PASSES:
            raise ValueError("%d passes: 1 .. %d fit one launch" % (len(self.passes), L.STAT_MAX_PASSES))
        self.mask_of = {}
        for name in self.passes:
            if has_masked_entry(name):
                color = RenderPasses.direct_or_indirect_to_color_render_pass(name)
                if color not in self.target_passes:      # (the reference: a KeyError in target_features, TFRecordsStatistics.py:247)
                    raise ValueError("'%s' is masked by the target pass '%s', which the target features do not list" % (name, color))
                self.mask_of[name] = color
        self.source_channels = {p: RenderPasses.number_of_channels(p) for p in self.source_passes}
        self.target_channels = {p: RenderPasses.number_of_channels(p) for p in self.target_passes}
        self.bytes_per_pixel = 4 * (len(self.spps) * self.sources * sum(self.source_channels.values()) + sum(self.target_channels.values()))
        self.rows = np.zeros((0, len(self.passes), L.STAT_FIELDS))
        self.spp_index = np.zeros((0,), dtype=np.int64)
        self.skipped = list(frame_set.skipped)

    # ================================================================== the device side
    def launch(self, bank):
        """ONE dd_tile_statistics launch over every window of `bank` (FrameBank.for_passes of this set's passes and counts)
        -> (rows [n, n_passes, STAT_FIELDS] as a device tensor, spp_index [n])."""
        import torch
        windows, spp_index = window_table([(s.height, s.width) for s in bank.scenes], self.tile, len(self.spps), self.sources)
        desc = L.StatDesc()
        desc.n_passes, desc.n_planes, desc.plane_hw = len(self.passes), bank.n_planes, bank.plane_hw.data_ptr()
        for en, name in zip(desc.pass_, self.passes):
            en.planes, en.C, en.is_alpha = bank.pointers[name].data_ptr(), RenderPasses.number_of_channels(name), int(name == RenderPasses.ALPHA)
            en.mask_planes = bank.pointers[self.mask_of[name]].data_ptr() if name in self.mask_of else None
        table = torch.from_numpy(windows.view(np.uint8).copy()).to(bank.device)
        rows = torch.empty((len(windows), len(self.passes), L.STAT_FIELDS), dtype=torch.float64, device=bank.device)
        L.check(L.load().dd_tile_statistics(C.byref(desc), table.data_ptr(), len(windows), self.tile, rows.data_ptr(),
                                            torch.cuda.current_stream(bank.device).cuda_stream))
        return rows, spp_index

    def compute(self, device="cuda", memory_limit_bytes=None, threads=4, log=print, decode="host", inflate="host"):
        """Scenes in chunks that fit the limit (default: 80 % of the free device memory): load, launch, copy the table back, free."""
        import torch
        from .frame_bank import FrameBank
        device = torch.device(device)
        if memory_limit_bytes is None:
            memory_limit_bytes = int(0.8 * torch.cuda.mem_get_info(device)[0])
        rows, index = [], []
        for scenes in chunk_scenes(self.frame_set.scenes, self.bytes_per_pixel, memory_limit_bytes):
            bank = FrameBank.for_passes(self.frame_set, self.source_channels, self.target_channels, self.spps, scenes=scenes, device=device,
                                        memory_limit_bytes=memory_limit_bytes, threads=threads, log=log, decode=decode, inflate=inflate)
            self.skipped += bank.skipped
            if bank.scenes:
                with torch.cuda.device(device):
                    r, k = self.launch(bank)
                    rows.append(r.cpu().numpy())         # (the copy waits for the launch: the planes may go afterwards)
                index.append(k)
            del bank
        if not rows:
            raise ValueError("no usable scene is left (%d skipped)" % len(self.skipped))
        self.add_rows(rows, index)
        return self

    def add_rows(self, rows, spp_index):
        """Append the tables of further chunks (lists of [n, n_passes, STAT_FIELDS] and [n])."""
        self.rows = np.concatenate([self.rows] + [np.asarray(r, dtype=np.float64) for r in rows], axis=0)
        self.spp_index = np.concatenate([self.spp_index] + [np.asarray(k, dtype=np.int64) for k in spp_index], axis=0)

    # ================================================================== the join
    def statistics(self, spps=None):
        """{feature name: entry} over the source windows of the counts `spps` (all of the list when None) and the target windows."""
        wanted = [k for k, spp in enumerate(self.spps) if spps is None or spp in spps]
        source, target = np.isin(self.spp_index, wanted), self.spp_index == TARGET
        out = {}
        for windows, passes, feature_name in ((source, self.source_passes, Naming.source_feature_name), (target, self.target_passes, Naming.target_feature_name)):
            for name in passes:
                rows, ch = self.rows[windows, self.passes.index(name)], RenderPasses.number_of_channels(name)
                out[feature_name(name)] = join_entry(rows, self.tile, ch, False)
                if name in self.mask_of:
                    out[feature_name(name, masked=True)] = join_entry(rows, self.tile, ch, True)
        return out

    def results(self):
        """[(samples per pixel or None, statistics)]: one per count when grouped, else one (TFRecordsStatistics.py:28-34)."""
        if self.group:
            return [(spp, self.statistics([spp])) for spp in self.spps]
        return [(None, self.statistics())]

    def write(self, directory, mode):
        """<directory>/<mode>_statistics.json, or <mode>_statistics_<spp>.json per count when grouped (TFRecordsStatistics.py:226-233).
        -> [(path, samples per pixel or None, statistics)]"""
        os.makedirs(directory, exist_ok=True)
        out = []
        for spp, stats in self.results():
            path = os.path.join(directory, mode + ("_statistics.json" if spp is None else "_statistics_%d.json" % spp))
            with open(path, "w", encoding="utf-8") as f:
                f.write(json.dumps(stats, sort_keys=True, indent=2))
            out.append((path, spp, stats))
        return out


def table_lines(stats):
    """One line per entry: name, mean, variance, log1p mean, log1p variance, coverage."""
    width = max([len(n) for n in stats] + [4])
    lines = ["%-*s %14s %14s %14s %14s %10s" % (width, "name", "mean", "variance", "log1p mean", "log1p variance", "coverage")]
    for name in sorted(stats):
        s, l = stats[name]["statistics"], stats[name]["statistics_log1p"]
        lines.append("%-*s %14.6g %14.6g %14.6g %14.6g %10.4f" % (width, name, s["mean"], s["variance"], l["mean"], l["variance"], s["coverage"]))
    return lines


def parser():
    p = argparse.ArgumentParser(description="Statistics of a frame set (<mode>_statistics.json), reduced on the device.")
    p.add_argument("json_filename", help="The TFRecords-JSON that names the scenes (the schema of TFRecordsExample.json).")
    p.add_argument("--mode", action="append", default=None, help="A mode of the JSON; may be given more than once (default: every mode).")
    p.add_argument("--output", default=None, help="Directory of the statistics files (default: the JSON's base_tfrecords_directory).")
    p.add_argument("--frame_memory_gb", type=float, default=None,
                   help="The most device memory the frames of one chunk may take (default: 80 %% of what is free).")
    p.add_argument("--threads", type=int, default=4, help="EXR decoder threads.")
    p.add_argument("--device", default="cuda", help="The device the frames are reduced on.")
    p.add_argument("--exr_decode", default="host", choices=["host", "device"],
                   help="Where the EXR files are decoded: on the host, or inflated on the host and rebuilt on the device by one launch per scene.")
    from . import openexr
    openexr.add_inflate_argument(p, "--exr_decode device")
    return p


def main(args, log=print):
    from .frame_bank import FrameSet
    with open(args.json_filename, encoding="utf-8") as f:
        j = json.load(f)
    here = os.path.dirname(os.path.abspath(args.json_filename))
    directory = args.output
    if directory is None:
        base = j["base_tfrecords_directory"]
        directory = base if os.path.isabs(base) else os.path.join(here, base)
    limit = None if args.frame_memory_gb is None else int(args.frame_memory_gb * 2 ** 30)
    written = []
    for mode in (args.mode or list(j["modes"])):
        frame_set = FrameSet.from_json(args.json_filename, mode, log=log)
        stats = FrameStatistics(frame_set, j["modes"][mode].get("group_by_samples_per_pixel", False))
        stats.compute(args.device, limit, max(1, min(args.threads, 8)), log, decode=args.exr_decode, inflate=args.exr_inflate)
        for path, spp, entries in stats.write(directory, mode):
            log("statistics: %s%s -- %d scene(s), %d window(s), %d skipped -> %s"
                % (mode, "" if spp is None else " at %d samples per pixel" % spp, len(frame_set.scenes) - (len(stats.skipped) - len(frame_set.skipped)),
                   len(stats.rows), len(stats.skipped), path))
            for line in table_lines(entries):
                log(line)
            written.append(path)
    return written


if __name__ == "__main__":
    main(parser().parse_args(sys.argv[1:]))
