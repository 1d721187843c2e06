"""Training from rendered frames that stay in device memory: no .tfrecords in between.

The reference trains from tile records that TFRecordsCreator.py cuts out of the rendered EXRs (TFRecordsCreator.py:97-160; it needs
TensorFlow 1.x and OpenCV).  Here the EXRs themselves are the data set:

    FrameSet     the TFRecords-JSON (TFRecordsExample.json) and the scene directories it names: which renderings exist, which are usable
                 (OpenEXRDirectories.py:18-29, OpenEXRDirectory.py:20, TFRecordsCreator.py:62-88); host only, reads EXR headers only
    FrameBank    the passes an architecture loads, of one samples-per-pixel count, decoded once and kept as fp32 planes on the device
                 (FrameBank.for_passes: a given set of passes, of one or several counts, without an architecture -- statistics.py)
    TileSampler  a mini-batch = B windows of resident planes: `draw` picks them (random crops, the reference's fixed grid of
                 TFRecordsCreator.py:125-133, or crops drawn where the noise is: frame_importance.py), `sample` uploads the B records and
                 makes ONE dd_sample_tiles launch that crops and augments every pass into the program's input and target buffers
                 (csrc/dd_tile_sampler.hip)

A PLANE is one rendering of one scene.  Plane indices are shared by all passes: scene s of a bank with S sources per example owns planes
s * (S + 1) + 0 .. S-1 (its source renderings, in path order) and s * (S + 1) + S (its target rendering).  A record is four int32
(source plane, target plane, y0, x0).
"""
import concurrent.futures
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib as L
from . import openexr
from .data_augmentation import DataAugmentation
from .input_assembly import write_constant_flags
from .render_passes import RenderPassesUsage

# dd_tile_record as a numpy record (64 bytes)
RECORD_DTYPE = np.dtype([("source_plane", "<i4"), ("target_plane", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("flip", "<i4"), ("rotate", "<i4"),
                         ("permute", "<i4"), ("normal_rotation", "<f4", (9,))])
assert RECORD_DTYPE.itemsize == C.sizeof(L.TileRecord)


class Scene:
    """One usable entry of exr_directories: `sources[spp]` = the first number_of_sources_per_example rendering directories of that spp in
    path order, `target` = the first rendering of the target spp (TFRecordsCreator.py:152), all of `height` x `width` pixels."""

    def __init__(self, directory, sources, target, target_spp, height, width):
        self.directory, self.sources, self.target, self.target_spp, self.height, self.width = directory, sources, target, target_spp, height, width


class FrameSet:
    def __init__(self, scenes, tile, number_of_sources_per_example, source_spps, source_passes, target_passes, skipped):
        self.scenes, self.tile, self.number_of_sources_per_example = scenes, tile, number_of_sources_per_example
        self.source_spps, self.source_passes, self.target_passes, self.skipped = source_spps, source_passes, target_passes, skipped

    @staticmethod
    def renderings(scene_directory):
        """{spp: [rendering directories, sorted by path]}: every subdirectory is one rendering, its spp the third field from the end of its
        '_'-separated path (OpenEXRDirectories.py:18-29, OpenEXRDirectory.py:20)."""
        out = {}
        for name in os.listdir(scene_directory):
            path = os.path.join(scene_directory, name)
            if os.path.isdir(path):
                try:
                    spp = int(path.split("_")[-3])
                except (ValueError, IndexError):
                    raise openexr.ExrError("%s: the directory name does not carry the samples per pixel (<...>_<spp>_<a>_<b>)" % path)
                out.setdefault(spp, []).append(path)
        for paths in out.values():
            paths.sort()
        return out

    @staticmethod
    def from_json(path, mode, log=print):
        """The scenes of `mode` ('training', 'validation', ...) in the TFRecords-JSON at `path`.  A scene that cannot be used is skipped with
        one line through `log` (the reference logs it and marks it invalid); a set without a usable scene raises."""
        with open(path, encoding="utf-8") as f:
            j = json.load(f)
        if mode not in j["modes"]:
            raise KeyError("%s has no mode '%s'" % (path, mode))
        here = os.path.dirname(os.path.abspath(path))
        base = j["base_exr_directory"] if os.path.isabs(j["base_exr_directory"]) else os.path.join(here, j["base_exr_directory"])
        tile = int(j["modes"][mode]["tiles_height_width"])
        S = int(j["source"]["number_of_sources_per_example"])
        spps = [int(s) for s in j["source"]["samples_per_pixel"]]
        source_passes = RenderPassesUsage(**j["source"]["features"]).render_passes()
        target_passes = RenderPassesUsage(**j["target"]["features"]).render_passes()
        scenes, skipped = [], []
        for name in j["modes"][mode]["exr_directories"]:
            directory = os.path.join(base, name)
            try:
                scenes.append(FrameSet._scene(directory, tile, S, spps, j["target"]["samples_per_pixel"], source_passes, target_passes))
            except openexr.ExrError as e:
                skipped.append((directory, str(e)))
                log("frames: %s skipped: %s" % (directory, e))
        if not scenes:
            raise ValueError("%s: no usable scene for mode '%s' (%d skipped)" % (path, mode, len(skipped)))
        return FrameSet(scenes, tile, S, spps, source_passes, target_passes, skipped)

    @staticmethod
    def _scene(directory, tile, S, spps, target_spp, source_passes, target_passes):
        if not os.path.isdir(directory):
            raise openexr.ExrError("base directory does not exist")
        found = FrameSet.renderings(directory)
        sources = {}
        for spp in spps:
            if spp not in found:
                raise openexr.ExrError("no subdirectory for %d samples per pixel" % spp)
            if len(found[spp]) < S:
                raise openexr.ExrError("%d subdirectories for %d samples per pixel are required, there is/are only %d" % (S, spp, len(found[spp])))
            sources[spp] = found[spp][:S]
        if target_spp == "best":
            target_spp = max(found) if found else 0
        target_spp = int(target_spp)
        if target_spp not in found:
            raise openexr.ExrError("no subdirectory for %d samples per pixel" % target_spp)
        target = found[target_spp][0]
        size = None
        for rendering, passes in [(r, source_passes) for spp in spps for r in sources[spp]] + [(target, target_passes)]:
            frame = openexr.OpenEXRDirectory(rendering)
            for render_pass in passes:
                file = frame.file_of(render_pass)              # ExrError: missing or ambiguous pass
                hw = openexr.image_size(file)
                if size is None:
                    size = hw
                elif hw != size:
                    raise openexr.ExrError("%s is %dx%d, other images of the scene are %dx%d" % (file, hw[1], hw[0], size[1], size[0]))
        if size is None:
            raise openexr.ExrError("no render pass is required: nothing to load")
        if size[0] < tile or size[1] < tile:
            raise openexr.ExrError("the images are %dx%d: smaller than one tile of %d pixels" % (size[1], size[0], tile))
        return Scene(directory, sources, target, target_spp, size[0], size[1])


class FrameBank:
    """The frames of `frame_set` an architecture trains on, as fp32 device planes [h, w, channels]: the passes it loads (f.load_data) of the
    source renderings of ONE samples-per-pixel count (the reference trains on one, Training.py:735) and of the target rendering.

    planes[name][p]: the tensor of pass `name` in plane p, or None (a pass that is only a source has no tensor in a target plane);
    pointers[name]: the same as a device int64 array (0 where None); plane_hw: device int32 [n_planes, 2]; hw: the same on the host.
    A scene with a non-finite sample is skipped with one line through `log` (OpenEXRDirectory.py:72-76).
    decode: 'host' -- every file goes through openexr.read_image on `threads` threads and is uploaded; 'device' -- the host only inflates and
    one dd_exr_reconstruct launch per scene rebuilds the planes on the device (openexr.DeviceDecoder): the same planes, bit for bit.
    inflate: with decode 'device', 'device' -- the host only reads the files and a dd_exr_inflate launch per scene inflates them."""

    def __init__(self, arch, frame_set, spp=None, device=None, memory_limit_bytes=None, threads=4, log=print, decode="host", inflate="host"):
        self.frame_set, self.tile, self.S = frame_set, frame_set.tile, frame_set.number_of_sources_per_example
        self.spp = int(frame_set.source_spps[0] if spp is None else spp)
        self.device = torch.device(arch.device if device is None else device)
        if self.spp not in frame_set.source_spps:
            raise ValueError("%d samples per pixel: the frame set lists %s" % (self.spp, frame_set.source_spps))
        self.spps = [self.spp]
        self._channels(arch)
        for what, need, have in (("source", self.source_channels, frame_set.source_passes), ("target", self.target_channels, frame_set.target_passes)):
            for name in need:
                if name not in have:
                    raise ValueError("the architecture loads the %s pass '%s', which the frame set's %s features do not list" % (what, name, what))
        self._load(frame_set.scenes, memory_limit_bytes, threads, log, decode, inflate)
        if not self.scenes:
            raise ValueError("no usable scene is left (%d skipped)" % (len(frame_set.skipped) + len(self.skipped)))
        self._tables()

    @classmethod
    def for_passes(cls, frame_set, source_channels, target_channels, spp, scenes=None, device="cuda", memory_limit_bytes=None, threads=4, log=print,
                   decode="host", inflate="host"):
        """A bank of the passes `source_channels` / `target_channels` ({pass name: channels}) without an Architecture: what the data-set
        statistics read (deepdenoiser_amd/statistics.py).  `spp`: one samples-per-pixel count or a list of them -- with a list a scene owns
        len(spp) * S source planes, those of the first count first, and `S` is that product, so source_plane / target_plane hold.  `scenes`:
        the scenes of `frame_set` to load (all of them when None).  A bank whose scenes were all skipped has no plane and is not refused."""
        self = cls.__new__(cls)
        self.frame_set, self.tile, self.device = frame_set, frame_set.tile, torch.device(device)
        self.spps = [int(s) for s in (spp if isinstance(spp, (list, tuple)) else [spp])]
        for s in self.spps:
            if s not in frame_set.source_spps:
                raise ValueError("%d samples per pixel: the frame set lists %s" % (s, frame_set.source_spps))
        self.spp, self.S = self.spps[0], frame_set.number_of_sources_per_example * len(self.spps)
        self.source_channels, self.target_channels = dict(source_channels), dict(target_channels)
        self._load(frame_set.scenes if scenes is None else scenes, memory_limit_bytes, threads, log, decode, inflate)
        self._tables()
        return self

    def _load(self, scenes, memory_limit_bytes, threads, log, decode="host", inflate="host"):
        if decode not in ("host", "device"):
            raise ValueError("decode: 'host' or 'device', not %r" % (decode,))
        if inflate not in ("host", "device"):
            raise ValueError("inflate: 'host' or 'device', not %r" % (inflate,))
        if inflate == "device" and decode != "device":
            raise ValueError("inflate='device' needs decode='device': the device inflates into the staged buffer of the device decoder")
        self.decode, self.inflate = decode, inflate
        # (a decoder refuses a device that is no GPU with ValueError, before anything is read)
        decoder = openexr.DeviceDecoder(self.device, threads=max(1, min(int(threads), 16)), inflate=inflate) if decode == "device" else None
        # ---- the bytes, before anything is allocated
        per_pixel = 4 * (self.S * sum(self.source_channels.values()) + sum(self.target_channels.values()))
        self.total_bytes = sum(s.height * s.width * per_pixel for s in scenes)
        if memory_limit_bytes is None:
            memory_limit_bytes = int(0.8 * torch.cuda.mem_get_info(self.device)[0]) if self.device.type == "cuda" else None
        if memory_limit_bytes is not None and self.total_bytes > memory_limit_bytes:
            raise MemoryError("the frames take %d bytes of device memory (%d scenes, %d source renderings each, %d spp), the limit is %d bytes"
                              % (self.total_bytes, len(scenes), self.S, self.spp, memory_limit_bytes))
        # ---- decode and upload, scene by scene
        self.threads = max(1, min(int(threads), 32))
        self.scenes, self.hw, self.skipped = [], [], []
        self.planes = {name: [] for name in set(self.source_channels) | set(self.target_channels)}
        self.decoder = decoder                                # (None on the host path; its counters say what the load cost, tools/exr_decode_timing.py)
        with concurrent.futures.ThreadPoolExecutor(max_workers=self.threads) as pool:
            for scene in scenes:
                try:
                    loaded = self._load_scene(scene, pool) if decoder is None else self._load_scene_device(scene, decoder)
                except openexr.ExrError as e:
                    self.skipped.append((scene.directory, str(e)))
                    log("frames: %s skipped: %s" % (scene.directory, e))
                    continue
                self.scenes.append(scene)
                for plane in loaded:
                    self.hw.append((scene.height, scene.width))
                    for name in self.planes:
                        self.planes[name].append(plane.get(name))
        if decoder is not None:
            decoder.release()

    def _channels(self, arch):
        features = arch.feature_predictions + arch.auxiliary_features
        self.source_channels = {f.name: f.number_of_channels for f in features if f.load_data}
        self.target_channels = {f.name: f.number_of_channels for f in arch.feature_predictions if f.load_data and f.is_target}

    def _tables(self):
        self.n_planes = len(self.hw)
        self.plane_hw = torch.tensor(self.hw, dtype=torch.int32).to(self.device)
        self.pointers = {name: torch.tensor([0 if t is None else t.data_ptr() for t in tensors], dtype=torch.int64).to(self.device)
                         for name, tensors in self.planes.items()}

    @classmethod
    def synthetic(cls, arch, tile, sizes, sources=1, device=None, seed=0):
        """A bank of uniform random planes, one scene per (height, width) of `sizes`, made on the device: for measurements
        (tools/tile_sampler_timing.py), no file is read."""
        self = cls.__new__(cls)
        self.frame_set, self.tile, self.S, self.spp, self.skipped = None, int(tile), int(sources), 0, []
        self.device = torch.device(arch.device if device is None else device)
        self._channels(arch)
        gen = torch.Generator(device=self.device).manual_seed(seed)
        self.scenes = [Scene("synthetic_%d" % k, {}, None, 0, h, w) for k, (h, w) in enumerate(sizes)]
        self.hw = [(s.height, s.width) for s in self.scenes for _ in range(self.S + 1)]
        self.planes = {name: [] for name in set(self.source_channels) | set(self.target_channels)}
        for p, (h, w) in enumerate(self.hw):
            channels = self.target_channels if p % (self.S + 1) == self.S else self.source_channels
            for name in self.planes:
                self.planes[name].append(torch.rand((h, w, channels[name]), generator=gen, device=self.device) if name in channels else None)
        self.total_bytes = sum(t.numel() * 4 for tensors in self.planes.values() for t in tensors if t is not None)
        self._tables()
        return self

    def _load_scene(self, scene, pool):
        """[{pass name: device tensor}] for the scene's S source planes and its target plane."""
        def load(rendering, name, channels):
            frame = openexr.OpenEXRDirectory(rendering)
            path = frame.file_of(name)
            image = openexr.read_image(path)[..., :channels]
            if image.shape[:2] != (scene.height, scene.width):
                raise openexr.ExrError("%s is %dx%d, the scene is %dx%d" % (path, image.shape[1], image.shape[0], scene.width, scene.height))
            if not np.isfinite(image).all():
                raise openexr.ExrError("there is at least one value in %s which is not finite" % path)
            return np.ascontiguousarray(image, dtype=np.float32)
        renderings = [r for spp in self.spps for r in scene.sources[spp]]
        jobs = [(p, name, pool.submit(load, r, name, ch)) for p, r in enumerate(renderings) for name, ch in self.source_channels.items()]
        same = scene.target in renderings                     # ("best" may be the source spp itself: the rendering is decoded once)
        if not same:
            jobs += [(self.S, name, pool.submit(load, scene.target, name, ch)) for name, ch in self.target_channels.items()]
        planes = [{} for _ in range(self.S + 1)]
        error = None
        for p, name, job in jobs:
            try:
                planes[p][name] = torch.from_numpy(job.result()).to(self.device)
            except openexr.ExrError as e:                      # (every job is waited for: none outlives the scene)
                error = error or e
        if error is not None:
            raise error
        if same:
            first = planes[renderings.index(scene.target)]
            planes[self.S] = {name: first[name] for name in self.target_channels}
        return planes

    def _load_scene_device(self, scene, decoder):
        """_load_scene with the files rebuilt on the device: one decode call for the scene, and the error of the first file that has one, in
        the order _load_scene submits its jobs."""
        renderings = [r for spp in self.spps for r in scene.sources[spp]]
        jobs = [(p, r, name, ch) for p, r in enumerate(renderings) for name, ch in self.source_channels.items()]
        same = scene.target in renderings
        if not same:
            jobs += [(self.S, scene.target, name, ch) for name, ch in self.target_channels.items()]
        found = []
        for p, rendering, name, ch in jobs:
            try:
                found.append(openexr.OpenEXRDirectory(rendering).file_of(name))
            except openexr.ExrError as e:
                found.append(e)
        wanted = [k for k, path in enumerate(found) if not isinstance(path, openexr.ExrError)]
        decoded = dict(zip(wanted, decoder.decode([(found[k], jobs[k][3]) for k in wanted], errors="return")))
        planes = [{} for _ in range(self.S + 1)]
        for k, (p, rendering, name, ch) in enumerate(jobs):
            result = decoded.get(k, found[k])
            if isinstance(result, openexr.ExrError):
                raise result
            image, nonfinite = result
            if tuple(image.shape[:2]) != (scene.height, scene.width):
                raise openexr.ExrError("%s is %dx%d, the scene is %dx%d" % (found[k], image.shape[1], image.shape[0], scene.width, scene.height))
            if nonfinite:
                raise openexr.ExrError("there is at least one value in %s which is not finite" % found[k])
            planes[p][name] = image
        if same:
            first = planes[renderings.index(scene.target)]
            planes[self.S] = {name: first[name] for name in self.target_channels}
        return planes

    def source_plane(self, scene_index, source_index):
        return scene_index * (self.S + 1) + source_index

    def target_plane(self, scene_index):
        return scene_index * (self.S + 1) + self.S


class TileRecords:
    """Which windows make a mini-batch of B examples: the host side of the sampler (no device, no program)."""

    def __init__(self, bank, B):
        self.bank, self.B, self.T = bank, int(B), bank.tile
        self._order, self._cursor = None, 0
        self.importance = None

    def set_importance(self, importance):
        """Attach the frame_importance.ImportanceMap of this bank: `draw` then knows the crops 'importance'."""
        if importance.tile != self.T or importance.sizes != [(s.height, s.width) for s in self.bank.scenes]:
            raise ValueError("the importance map was made for other frames: tiles of %d, scenes %s" % (importance.tile, importance.sizes))
        self.importance = importance

    def grid_records(self, index_tuples):
        """The reference's tile set (TFRecordsCreator.py:125-133 times Training.py:544-549) as records [n, 4] int32 (source plane, target
        plane, y0, x0): for every scene, `for i in range(h // T): for j in range(w // T)`, for every source index tuple."""
        bank, T = self.bank, self.T
        out = [(bank.source_plane(s, tup[0]), bank.target_plane(s), i * T, j * T)
               for s, scene in enumerate(bank.scenes) for i in range(scene.height // T) for j in range(scene.width // T) for tup in index_tuples]
        return np.asarray(out, dtype=np.int32).reshape(-1, 4)

    def epoch_examples(self, index_tuples):
        """Examples of an epoch, in every crop mode: the size of the grid set."""
        return sum((s.height // self.T) * (s.width // self.T) for s in self.bank.scenes) * len(index_tuples)

    def reset(self):
        self._order, self._cursor = None, 0

    def draw(self, rng, crops, index_tuples, rank=0, world=1):
        """The records [B, 4] of this rank's next mini-batch, or None when the epoch holds no further whole round of `world` mini-batches
        (the next call then starts an epoch).  `rng`: the random.Random all ranks share -- every rank draws the same world * B examples and
        takes examples rank * B .. (rank + 1) * B - 1 of them.  crops 'random': scene uniform, origin uniform in [0, h-T] x [0, w-T], source
        index from a uniformly chosen index tuple; 'grid': the grid set, shuffled once per epoch and handed out in that order; 'importance':
        as 'random', every example by ImportanceMap.draw of the attached map (set_importance)."""
        if crops not in ("random", "grid", "importance"):
            raise ValueError("crops: 'random', 'grid' or 'importance', not %r" % (crops,))
        if crops == "importance" and self.importance is None:
            raise ValueError("crops 'importance': no importance map is attached (TileRecords.set_importance)")
        bank, T, need = self.bank, self.T, self.B * world
        if self._order is None:
            self._cursor = 0
            if crops == "grid":
                self._order = self.grid_records(index_tuples)
                perm = list(range(len(self._order)))
                rng.shuffle(perm)
                self._order = self._order[perm]
            else:
                self._order = self.epoch_examples(index_tuples)
        total = len(self._order) if crops == "grid" else self._order
        if self._cursor + need > total:
            self.reset()
            return None
        if crops == "grid":
            drawn = self._order[self._cursor:self._cursor + need]
        elif crops == "importance":
            drawn = np.empty((need, 4), dtype=np.int32)
            for k in range(need):
                s, y0, x0, tup = self.importance.draw(rng, index_tuples)
                drawn[k] = (bank.source_plane(s, tup[0]), bank.target_plane(s), y0, x0)
        else:
            drawn = np.empty((need, 4), dtype=np.int32)
            for k in range(need):
                s = rng.randrange(len(bank.scenes))
                tup = index_tuples[rng.randrange(len(index_tuples))]
                scene = bank.scenes[s]
                drawn[k] = (bank.source_plane(s, tup[0]), bank.target_plane(s), rng.randint(0, scene.height - T), rng.randint(0, scene.width - T))
        self._cursor += need
        return np.ascontiguousarray(drawn[rank * self.B:(rank + 1) * self.B])

    def validate(self, records):
        """ValueError for a record the kernel would have to clamp: a plane index out of range, a source (target) plane that holds no source
        (target) pass, planes of different sizes, an origin outside [0, h-T] x [0, w-T]."""
        bank, T = self.bank, self.T
        records = np.asarray(records)
        if records.shape != (self.B, 4):
            raise ValueError("records: expected [%d, 4] (source plane, target plane, y0, x0), got %s" % (self.B, records.shape))
        for b, (sp, tp, y0, x0) in enumerate(records.tolist()):
            for what, p in (("source", sp), ("target", tp)):
                if not 0 <= p < bank.n_planes:
                    raise ValueError("record %d: %s plane index %d out of range (0 .. %d)" % (b, what, p, bank.n_planes - 1))
            if sp % (bank.S + 1) == bank.S or tp % (bank.S + 1) != bank.S:
                raise ValueError("record %d: plane %d is no source plane or plane %d is no target plane" % (b, sp, tp))
            if bank.hw[sp] != bank.hw[tp]:
                raise ValueError("record %d: the source plane is %s, the target plane %s" % (b, bank.hw[sp], bank.hw[tp]))
            h, w = bank.hw[sp]
            if not (0 <= y0 <= h - T and 0 <= x0 <= w - T):
                raise ValueError("record %d: origin (%d, %d) outside [0, %d] x [0, %d]" % (b, y0, x0, h - T, w - T))

    def pack(self, records, draws=None):
        """The dd_tile_record table of a mini-batch as a numpy record array (draws None: identity draws)."""
        table = np.zeros(self.B, dtype=RECORD_DTYPE)
        records = np.asarray(records, dtype=np.int32)
        for k, key in enumerate(("source_plane", "target_plane", "y0", "x0")):
            table[key] = records[:, k]
        if draws is not None:
            for key in ("flip", "rotate", "permute"):
                table[key] = np.asarray(draws[key], dtype=np.int32)
            table["normal_rotation"] = np.asarray(draws["normal_rotation"], dtype=np.float32).reshape(self.B, 9)
        return table


class TileSampler(TileRecords):
    """Fills `program.input.raw[*]` and `program.targets[0]` with windows of `bank`'s planes.  usage: DataAugmentationUsage."""
    RING = 4

    def __init__(self, program, bank, usage):
        TileRecords.__init__(self, bank, program.B)
        if program.H != bank.tile or program.W != bank.tile:
            raise ValueError("the program was built for %dx%d tiles, the frames are cut into %d" % (program.H, program.W, bank.tile))
        self.program, self.bank, self.usage, self.lib = program, bank, usage, L.load()
        B, T = self.B, self.T
        inp = program.input
        if inp.frame_input is not None:
            inp.disable_frame_input()
        passes = []
        for f in inp.features:
            raw, ch = inp.raw[f.name], f.number_of_channels
            if f.load_data:
                passes.append((f.name, bank.pointers[f.name], raw.data_ptr(), ch, ch, 0))
            else:                                              # generated passes (Training.py:531-538): constant, written once
                raw.fill_(1.0 if f.feature_prediction_type == "COLOR" else 0.5)
        for i, f in enumerate(program.head):
            block, ch = program.targets[0][i * B:(i + 1) * B], f.number_of_channels
            if not f.load_data:
                block[..., :ch].fill_(1.0 if f.feature_prediction_type == "COLOR" else 0.5)
            elif f.name not in bank.target_channels:
                raise ValueError("'%s' is predicted but is not a target: there is nothing to train it on" % f.name)
            else:
                passes.append((f.name, bank.pointers[f.name], block.data_ptr(), ch, int(block.shape[-1]), 1))
        for name, buf in inp.flags_raw.items():
            write_constant_flags(program.arch, name, buf)
        if not 1 <= len(passes) <= L.TILE_MAX_PASSES:
            raise ValueError("%d passes to fill: 1 .. %d fit one launch" % (len(passes), L.TILE_MAX_PASSES))
        if usage.use_flip_left_right and any(name == "Normal" for name, *_ in passes):
            raise Exception("Flipping for normals is not supported.")      # DataAugmentation.py:22-23
        self.desc = L.TileSamplerDesc()
        self.desc.n_passes, self.desc.n_planes, self.desc.plane_hw = len(passes), bank.n_planes, bank.plane_hw.data_ptr()
        for en, (name, pointers, dst, ch, ld, from_target) in zip(self.desc.pass_, passes):
            en.planes, en.dst, en.C, en.kind, en.ld_dst, en.from_target = pointers.data_ptr(), dst, ch, DataAugmentation._kind(name, ch), ld, from_target
        self._records_dev = torch.zeros(B * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=bank.device)
        self._ring = []

    # ================================================================== the launch
    def sample(self, records, draws=None):
        """Fill the program's input and target buffers with the windows of `records`, augmented with `draws` (DataAugmentation.draw) under the
        sampler's usage switches; draws None: no augmentation (validation).  One stream-ordered table upload (a ring of pinned buffers, no
        host synchronisation) and one launch on the current stream."""
        self.validate(records)
        table = self.pack(records, draws)
        if not self._ring:
            self._ring = [[torch.empty(self._records_dev.numel(), dtype=torch.uint8, pin_memory=True), None] for _ in range(self.RING)]
        slot = self._ring.pop(0)
        self._ring.append(slot)
        if slot[1] is not None:
            slot[1].synchronize()                              # (RING uploads ago: long executed)
        slot[0].numpy()[:] = table.view(np.uint8)
        self._records_dev.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        u = self.usage
        on = draws is not None
        L.check(self.lib.dd_sample_tiles(C.byref(self.desc), self._records_dev.data_ptr(), self.B, self.T, int(on and u.use_flip_left_right),
                                         int(on and u.use_rotate_90), int(on and u.use_rgb_permutation), int(on and u.use_normal_rotation),
                                         torch.cuda.current_stream().cuda_stream))
