"""Full-frame inference: halo tiling -> batched forward on the HIP path -> on-device crop/stitch -> recombination.

Mirrors the reference's Prediction.main (TensorFlow/Prediction.py:188-520) for the part that is on the hot path:
the integer tile plan and crop windows (bit-exact, tiling.py), row-major tile order (:325-326, :380-382), stitch
(:384-441) and recombination (:443-481).  Differences by design: tiles are batched
(the reference's batch-1 Estimator.predict and its temporary TFRecord round trip, :316-338, are not part of the
contract), crop/stitch/recombine run on the device, and tile_blend="feather" blends the overlapping tile predictions instead of cropping them
(dd_stitch_blend; the default "crop" is the reference's stitch).  EXR decode (cv2) is out of scope: frames are given as
tensors keyed by the reference's feature names.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from .input_assembly import write_constant_flags
from .naming import Naming
from .tiling import blend_cover, blend_weights, tile_plan

_COMBINED = ("Diffuse", "Glossy", "Subsurface", "Transmission")
_SINGLES = ("Volume Direct", "Volume Indirect", "Environment", "Emission")
RECOMBINE_MEMBERS = tuple(c + s for c in _COMBINED for s in (" Color", " Direct", " Indirect")) + _SINGLES      # every pass 'Combined' is formed from


class BlendTables:
    """What dd_stitch_blend needs of a tile plan: per axis the origins, the normalised weights of tiling.blend_weights and the first / last
    covering tile of every image coordinate, on the device, and the two dd_blend_axis structs that point at them."""

    def __init__(self, plan, device, width=None):
        self.plan, self._keep = plan, []
        self.rows, self.cols = self._axis(plan.rows, device, width), self._axis(plan.cols, device, width)

    def _axis(self, axis, device, width):
        first, last = blend_cover(axis)
        host = (C.c_int * axis.count)(*axis.origins)
        dev = [torch.tensor(axis.origins, dtype=torch.int32, device=device), torch.from_numpy(blend_weights(axis, width)).to(device).contiguous(),
               torch.tensor(first, dtype=torch.int32, device=device), torch.tensor(last, dtype=torch.int32, device=device)]
        self._keep += [host] + dev
        return L.BlendAxis(axis.count, host, *(t.data_ptr() for t in dev))

    def blend(self, lib, tiles_ptr, ldt, tiles_per_image, frames, C_, first_tile, n_tiles, stream):
        """frames [n_img, H, W, ldf] += the tiles [first_tile, first_tile + n_tiles) of the plan, read from [n_img * tiles_per_image, T, T, ldt]."""
        if tuple(frames.shape[1:3]) != (self.plan.height, self.plan.width):      # (the cover tables are as long as the plan's frame is large)
            raise ValueError("frames of %dx%d for the tables of a %dx%d plan" % (frames.shape[1], frames.shape[2], self.plan.height, self.plan.width))
        L.check(lib.dd_stitch_blend(tiles_ptr, self.plan.tile, ldt, tiles_per_image, frames.data_ptr(), frames.shape[0], frames.shape[1],
                                    frames.shape[2], frames.shape[3], C_, C.byref(self.rows), C.byref(self.cols), first_tile, n_tiles, stream))


class Predictor:
    def __init__(self, architecture, tile_size=128, tile_overlap_size=14, tiles_per_batch=16, use_graph=True, nonfinite="keep", nonfinite_radius=2,
                 tile_blend="crop", blend_width=None):
        """tile_blend: how the overlapping tile predictions become the frame.  "crop": one tile's prediction per pixel, the others dropped
        (Prediction.py:384-441, bit for bit).  "feather": every pixel is the weighted mean of all tiles that cover it, the weights ramping
        linearly over blend_width pixels at every tile side that faces another tile (tiling.blend_weights; None: twice the plan's
        overlap), by dd_stitch_blend next to the forward -- no step along the tile borders; the output does not depend on tiles_per_batch.
        nonfinite: what to do about NaN / Inf samples in the source passes of a frame (nonfinite.py).  "keep": nothing -- no scan, no launch,
        no allocation; one such sample makes a whole tile of every predicted pass NaN.  "error": scan the frame and raise ValueError naming the
        affected passes before any forward launch.  "repair": scan, then replace every such value by the mean of the finite values of its channel
        in the (2 nonfinite_radius + 1)^2 window, on the device and without a host synchronisation; nonfinite_report() gives the counts."""
        if nonfinite not in ("keep", "error", "repair"):
            raise ValueError('nonfinite must be "keep", "error" or "repair", not %r' % (nonfinite,))
        if not 1 <= int(nonfinite_radius) <= 4:
            raise ValueError("nonfinite_radius must be 1 .. 4, not %r" % (nonfinite_radius,))
        if tile_blend not in ("crop", "feather"):
            raise ValueError('tile_blend must be "crop" or "feather", not %r' % (tile_blend,))
        if blend_width is not None and not 0 <= int(blend_width) <= int(tile_size) // 2:
            raise ValueError("blend_width must be 0 .. tile_size // 2 = %d, not %r" % (int(tile_size) // 2, blend_width))
        self.tile_blend, self.blend_width = tile_blend, None if blend_width is None else int(blend_width)
        self.nonfinite, self.nonfinite_radius = nonfinite, int(nonfinite_radius)
        self._scanners, self._scanner = {}, None
        self.arch, self.tile_size, self.tile_overlap_size, self.tiles_per_batch = architecture, tile_size, tile_overlap_size, tiles_per_batch
        self.lib = L.load()
        self.use_graph = use_graph
        self._plans, self._graphs, self._blends = {}, {}, {}
        self.profile = None          # a list: predict_frame appends (start, before forward, after forward, end) timing events per tile batch / frame

    def prepare(self, H, W):
        """Build (and cache) the tile program for an HxW frame; the network parameters exist after this call, so weights are loaded
        with `architecture.params.load_list(...)` between prepare() and predict_frame()."""
        self._frame_plan(H, W)

    def _frame_plan(self, H, W):
        """Tile plan, gather indices and stitch tables of a frame size (cached: every frame of a sequence shares them)."""
        key = (H, W)
        if key in self._plans:
            return self._plans[key]
        dev = self.arch.device
        plan = tile_plan(H, W, self.tile_size, self.tile_overlap_size)
        T = plan.tile
        n_batches = -(-plan.count // max(1, self.tiles_per_batch))
        Bt = -(-plan.count // n_batches)          # balanced batches: 209 tiles at <= 64 per batch -> 4 x 53, not 3 x 64 + 17
        prog = self.arch.program(Bt, T, T)
        NF = prog.NF
        # ONE_HOT_ENCODING: the reference's prediction input_fn adds the constant one-hot planes of every flag name to the source
        # dictionary (Prediction.py:97-98 -> FeatureFlags.add_to_source_dictionary); they are written once here.  A caller may still
        # pass 'feature_flag/<name>' frames, which predict_frame() tiles like any other input.
        for name, buf in prog.flags_raw.items():
            write_constant_flags(self.arch, name, buf)
        origins = plan.windows()                                                              # row-major (Prediction.py:380-382)
        grid = [(hi, wi) for hi in range(plan.rows.count) for wi in range(plan.cols.count)]
        chunks = []
        for start in range(0, plan.count, Bt):
            ids = list(range(start, min(start + Bt, plan.count)))
            pad = ids + [ids[-1]] * (Bt - len(ids))                                           # ragged last batch: repeat a tile, never stitched
            oyx = torch.tensor([[origins[t][0], origins[t][1]] for t in pad], dtype=torch.int32, device=dev)     # dd_extract_tiles table
            table = (L.StitchEntry * (len(ids) * NF))()
            n = 0
            for f in range(NF):
                for slot, ti in enumerate(ids):
                    hi, wi = grid[ti]
                    (cy0, cy1), (cx0, cx1) = plan.rows.crops[hi], plan.cols.crops[wi]
                    table[n] = L.StitchEntry(f * Bt + slot, cy0, cy1, cx0, cx1, f, plan.rows.offsets[hi], plan.cols.offsets[wi])
                    n += 1
            tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
            chunks.append((oyx, tdev, n))
        if self.tile_blend == "feather":      # (raises for a blend_width beyond half of the tile a small frame shrank the plan to)
            self._blends[key] = BlendTables(plan, dev, self.blend_width)
        self._plans[key] = (plan, prog, chunks)
        return self._plans[key]

    def predict_frame(self, features):
        """features: {'source_image/0/<Pass>': [H,W,C] float32 tensor} -> {'prediction/<Pass>': [H,W,C]} (+ 'Combined' if all passes exist)."""
        arch, lib = self.arch, self.lib
        dev = arch.device
        names = arch.required_source_names()
        frame = {k: torch.as_tensor(features[k], dtype=torch.float32).to(dev).contiguous() for k in names}
        H, W = frame[names[0]].shape[0], frame[names[0]].shape[1]
        plan, prog, chunks = self._frame_plan(H, W)
        T, NF = plan.tile, prog.NF
        frames = torch.empty((NF, H, W, 3), dtype=torch.float32, device=dev)      # (the crops of the tile plan cover every pixel exactly once: tests/test_tiling_golden.py)
        # the MFMA operand images are re-packed only when the weights may have changed since this program last packed them (a frame sequence
        # runs on fixed weights: 30 us per 1080p frame); DD_PACK_EVERY_FRAME=1: always
        key = arch.params.state_key()
        if self.__dict__.setdefault("_packed", {}).get(id(prog)) != key or os.environ.get("DD_PACK_EVERY_FRAME", "0") == "1":
            prog.pack_weights()
            self._packed[id(prog)] = key
        stream = prog.g.stream_ptr()
        feats = prog.head + arch.auxiliary_features
        for f in feats:
            fr = frame[Naming.source_feature_name(f.name, index=0)]
            if fr.dim() != 3 or fr.shape[2] < f.number_of_channels or tuple(fr.shape[:2]) != (H, W):
                raise ValueError("%s: expected a [%d,%d,>=%d] frame, got %s" % (f.name, H, W, f.number_of_channels, tuple(fr.shape)))
        if self.nonfinite != "keep":
            self._scan_frame(features, frame, feats)
        flag_frames = {}
        for name, buf in prog.flags_raw.items():
            key = Naming.feature_flags_name(name)
            if key not in features:      # the constant one-hot plane (Prediction.py:108): rewritten per frame, a previous caller's planes must not linger
                write_constant_flags(arch, name, buf)
            if key in features:
                fr = torch.as_tensor(features[key], dtype=torch.float32).to(dev).contiguous()
                if tuple(fr.shape) != (H, W, prog.flags_raw[name].shape[3]):
                    raise ValueError("%s: expected a [%d,%d,%d] frame, got %s" % (key, H, W, prog.flags_raw[name].shape[3], tuple(fr.shape)))
                flag_frames[name] = fr
        # Render passes whose frames have exactly the pass's channels are read in place by the input assembly (no tile copies); anything else
        # (wider frames, DD_FRAME_INPUT=0, the unfused input path) goes through dd_extract_tiles as before.
        direct = (prog.fused_input and os.environ.get("DD_FRAME_INPUT", "1") != "0"
                  and all(frame[Naming.source_feature_name(f.name, index=0)].shape[2] == f.number_of_channels for f in feats))
        if direct:
            if prog.frame_input != (H, W):      # (programs are cached per (tiles per batch, tile): another frame size may share this one)
                prog.enable_frame_input(H, W)
            prog.set_frame_sources({f.name: frame[Naming.source_feature_name(f.name, index=0)] for f in feats})
        elif prog.frame_input is not None:      # (programs are cached per architecture: an earlier frame may have been read in place)
            prog.disable_frame_input()
        ev = None
        if self.profile is not None:      # (bench.py: where a frame's time goes on the device, and how long the device waits for the host between frames)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        blend, first_tile = self._blends.get((H, W)), 0
        for oyx, tdev, n in chunks:
            if direct:
                prog.frame_origins.copy_(oyx, non_blocking=True)
            for name, fr in flag_frames.items():
                raw = prog.flags_raw[name]
                L.check(lib.dd_extract_tiles(fr.data_ptr(), H, W, fr.shape[2], fr.shape[2], raw.data_ptr(), T, raw.shape[3],
                                             oyx.data_ptr(), oyx.shape[0], stream))
            for f in (() if direct else feats):                         # halo tiles straight into the program's input buffers
                fr = frame[Naming.source_feature_name(f.name, index=0)]
                raw = prog.raw[f.name]
                L.check(lib.dd_extract_tiles(fr.data_ptr(), H, W, fr.shape[2], f.number_of_channels, raw.data_ptr(), T, raw.shape[3],
                                             oyx.data_ptr(), oyx.shape[0], stream))
            if ev is not None and oyx is chunks[0][0]:
                ev[1].record()
            self._forward(prog)
            if ev is not None and oyx is chunks[-1][0]:
                ev[2].record()
            tiles = prog.predictions[0]                                  # [NF*Bt, T, T, 3], feature-major
            if blend is None:
                L.check(lib.dd_stitch(tiles.ptr, T, 3, frames.data_ptr(), H, W, 3, 3, tdev.data_ptr(), n, stream))
            else:                                                        # (n // NF: the batch's real tiles; a ragged batch's repeated tile is not one)
                blend.blend(lib, tiles.ptr, 3, oyx.shape[0], frames, 3, first_tile, n // NF, stream)
                first_tile += n // NF
        out = {}
        for f in arch.feature_predictions:
            if f.is_target and f.load_data:
                out[Naming.feature_prediction_name(f.name)] = frames[prog.head_index[f.name]][..., :f.number_of_channels]
        self._recombine(prog, frames, out, H * W, stream)
        if ev is not None:
            ev[3].record()
            self.profile.append(ev)
        return out

    def _scan_frame(self, features, frame, feats):
        """nonfinite = "error" / "repair": the required source passes of the frame through nonfinite.Scanner, on the program's stream and in
        front of the first tile batch, so the in-place input assembly and dd_extract_tiles both see repaired passes.  The caller's tensors are
        never modified: a pass that IS the caller's tensor (already a contiguous fp32 device tensor) is cloned before it is repaired."""
        from .nonfinite import Scanner
        keys = list(dict.fromkeys(Naming.source_feature_name(f.name, index=0) for f in feats))
        channels = {Naming.source_feature_name(f.name, index=0): f.number_of_channels for f in feats}
        if self.nonfinite == "repair":
            for k in keys:
                if torch.is_tensor(features[k]) and features[k].data_ptr() == frame[k].data_ptr():
                    frame[k] = frame[k].clone()
        sig = tuple((k, tuple(frame[k].shape), channels[k]) for k in keys)
        if sig not in self._scanners:
            self._scanners[sig] = Scanner(self.arch.device, sig)
        self._scanner = self._scanners[sig]
        self._scanner.scan(frame)
        if self.nonfinite == "repair":
            self._scanner.repair(frame, radius=self.nonfinite_radius)
            return
        bad = {k: v for k, v in self._scanner.report().items() if v["values"]}
        if bad:
            raise ValueError("non-finite values in the frame: " + "; ".join("%s: %d values in %d pixels" % (k, v["values"], v["pixels"])
                                                                             for k, v in bad.items()))

    def nonfinite_report(self):
        """{'source_image/0/<Pass>': {"values": int, "pixels": int}} of the last frame scanned (nonfinite = "error" / "repair"); synchronises."""
        if self._scanner is None:
            raise RuntimeError('nonfinite_report() needs a frame predicted with nonfinite="error" or "repair"')
        return self._scanner.report()

    def nonfinite_masks(self):
        """{'source_image/0/<Pass>': uint8 [H,W] device plane, bit c set where channel c was non-finite} of the last frame scanned."""
        if self._scanner is None:
            raise RuntimeError('nonfinite_masks() needs a frame predicted with nonfinite="error" or "repair"')
        return self._scanner.masks()

    def _forward(self, prog):
        """The tile program's forward launches, replayed from a hipGraph after one eager pass (the ~80 launches of a batch of tiles
        cost more on the host than on the device once the kernels are fast)."""
        if not self.use_graph:
            prog.forward(pack=False)
            return
        key = (id(prog), prog.frame_input)             # (a graph replays the input-assembly launch it was captured with)
        gr = self._graphs.get(key)
        if gr is None:
            prog.forward(pack=False)                 # eager once: binds every launch, warms the caches
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                prog.forward(pack=False)
            self._graphs[key] = gr
        gr.replay()

    def _recombine(self, prog, frames, out, npix, stream):
        idx = prog.head_index
        if not all(n in idx and prog.head[idx[n]].load_data for n in RECOMBINE_MEMBERS):
            return
        out.update(recombine(self.lib, {n: frames[idx[n]] for n in RECOMBINE_MEMBERS}, npix, stream))


def recombine(lib, passes, npix, stream):
    """The recombination of Prediction.py:443-481 by dd_recombine: passes = {pass name: contiguous fp32 [H,W,3] device tensor} with every name
    of RECOMBINE_MEMBERS -> {'prediction/<combined feature>': [H,W,3]} for the four combined features, then 'Combined'.  Predictor._recombine
    forms them from the predicted frames, quality.targets_of_frame from the target frames: one launch either way."""
    first = passes[RECOMBINE_MEMBERS[0]]
    comb = torch.zeros((len(_COMBINED) + 1,) + tuple(first.shape), dtype=torch.float32, device=first.device)
    out = {}
    d = L.RecombineDesc()
    d.n_triples = len(_COMBINED)
    for k, c in enumerate(_COMBINED):
        d.color[k], d.direct[k], d.indirect[k] = (passes[c + s].data_ptr() for s in (" Color", " Direct", " Indirect"))
        d.combined[k] = comb[k].data_ptr()
        out[Naming.feature_prediction_name(c)] = comb[k]
    d.n_singles = len(_SINGLES)
    for j, s in enumerate(_SINGLES):
        d.single[j] = passes[s].data_ptr()
    d.image = comb[len(_COMBINED)].data_ptr()
    L.check(lib.dd_recombine(C.byref(d), npix, stream))
    out["Combined"] = comb[len(_COMBINED)]
    return out
