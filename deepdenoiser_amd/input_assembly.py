"""The network input of a Program: raw pass buffers -> standardize + variance -> SourceEncoder's channel layout (SourceEncoder.py:29-79).

tuple_layout() is the ONE statement of that layout; the dd_assemble_input table, the DD_FUSE_INPUT=0 dd_gather_input table and the
embedding-row gradient are all driven by it.  Filling a table is host only (fill_assemble_table / fill_gather_table return the ctypes array);
the upload to the device is apart from it."""
import collections
import ctypes as C
import math
import os

import torch

from . import _lib as L
from .naming import Naming

PASS, VECTOR, PLANE = 0, 1, 2      # dd_assemble_entry.kind: a render pass, the tuple's embedding row, the tuple's one-hot plane

# feature / head: the pass and its index in head order (None: an auxiliary feature); both None for the feature-flag entry
Entry = collections.namedtuple("Entry", "kind feature head nch dst_ch")


def tuple_layout(arch):
    """([the entries of tuple t, in channel order], first channel of the embedding row or None): members, auxiliary features, then the
    one-hot plane or the embedding row (SourceEncoder.prepare_neural_network_input, FeatureFlags.py:50-69).  Head order is member-major."""
    tuples = arch.feature_prediction_tuples
    T, V = len(tuples), len(arch.feature_flag_names)
    flags = {"NONE": None, "ONE_HOT_ENCODING": (PLANE, V), "EMBEDDING": (VECTOR, V // 2)}[arch.feature_flag_mode]
    layout, emb_ch0 = [], None
    for t, tup in enumerate(tuples):
        entries, ch = [], 0
        for f, head_i in [(f, j * T + t) for j, f in enumerate(tup.feature_predictions)] + [(f, None) for f in arch.auxiliary_features]:
            nch = 3 + f.feature_variance.channels(f.number_of_channels)
            entries.append(Entry(PASS, f, head_i, nch, ch))
            ch += nch
        if flags is not None:
            entries.append(Entry(flags[0], None, None, flags[1], ch))
            if flags[0] == VECTOR:
                emb_ch0 = ch
            ch += flags[1]
        assert ch == arch.input_channels(), (ch, arch.input_channels())
        layout.append(entries)
    return layout, emb_ch0


def write_constant_flags(arch, name, buf):
    """The constant one-hot plane of tuple `name` the reference's input_fn adds to the source dictionary (Training.py:757-758,
    Prediction.py:97-98 -> FeatureFlags.add_to_source_dictionary)."""
    buf.zero_()
    buf[..., arch.feature_flag_names.index(name)] = 1.0


def feature_params(f, identity=False):
    """FeatureStandardization + FeatureVariance settings of a pass as the kernels take them (Architecture.py:39-73)."""
    fp = L.FeatureParams()
    st, fv = f.feature_standardization, f.feature_variance
    if identity:
        fp.use_log1p, fp.mean, fp.inv_std, fp.use_variance = 0, 0.0, 1.0, 0
    else:
        fp.use_log1p, fp.mean = int(st.use_log1p), st.mean
        fp.inv_std = 1.0 / math.sqrt(st.variance) if st.variance != 1.0 else 1.0
        fp.use_variance = int(fv.use_variance)
    fp.variance_before = int(fv.compute_before_standardization)
    fp.mode_neighbor = int(fv.variance_mode == "neighbor")
    fp.relative, fp.compress, fp.epsilon = int(fv.relative_variance), int(fv.compress_to_one_channel), 1e-4
    return fp


class HostInputStager:
    """Feeds a Program from pinned host memory without exposing the PCIe copy on the launch stream.

    `depth` sets of device staging tensors; `stage(features, labels)` enqueues the host -> device copies of one mini-batch on a COPY stream (after
    the launch stream has finished reading that slot's previous contents), `consume()` makes the launch stream wait for the oldest staged batch
    and moves it into the program's static input buffers with device-to-device copies (the captured hipGraph reads fixed addresses).  Call
    stage() for batch k + 1 before the step of batch k: the upload then runs beside the step.  cfg-2 at 128 tile passes: 307 MB per step over
    PCIe (~6 ms at 50 GB/s) against a 9.2 ms step."""

    def __init__(self, program, depth=2):
        self.prog = program
        self.device = program.arch.device
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.depth = depth
        self.slots = [None] * depth          # per slot: (device features, device labels)
        self.ready = [None] * depth          # event: upload of the slot complete
        self.free = [None] * depth           # event: the launch stream has consumed the slot
        self.head = self.tail = self.count = 0

    def _like(self, slot, feats, labels):
        if self.slots[slot] is None:
            self.slots[slot] = ({k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in feats.items()},
                                {k: torch.empty(v.shape, dtype=v.dtype, device=self.device) for k, v in (labels or {}).items()})
        return self.slots[slot]

    def stage(self, features, labels=None):
        assert self.count < self.depth, "every staging slot holds an unconsumed batch"
        slot = self.head
        df, dl = self._like(slot, features, labels)
        with torch.cuda.stream(self.copy_stream):
            if self.free[slot] is not None:
                self.copy_stream.wait_event(self.free[slot])
            for k, v in features.items():
                df[k].copy_(v, non_blocking=True)
            for k, v in (labels or {}).items():
                dl[k].copy_(v, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.ready[slot] = (ev, features, labels)      # (the pinned sources stay referenced until the copy has run)
        self.head = (self.head + 1) % self.depth
        self.count += 1

    def consume(self):
        assert self.count > 0, "nothing staged"
        slot = self.tail
        ev = self.ready[slot][0]
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        df, dl = self.slots[slot]
        self.prog.set_inputs(df, dl if dl else None)
        done = torch.cuda.Event()
        done.record(main)
        self.free[slot] = done
        self.tail = (self.tail + 1) % self.depth
        self.count -= 1


class InputAssembly:
    """Buffers and launches of a program's network input `X` [T*B, H, W, input_channels]; constructed by Program.__init__ at the head of the
    forward list.  `head`: the program's head features, member-major."""

    def __init__(self, arch, g, B, H, W, head, training):
        self.arch, self.g, self.lib, self.B, self.H, self.W, self.head = arch, g, g.lib, B, H, W, head
        dev = arch.device
        tuples = arch.feature_prediction_tuples
        T, NF = len(tuples), len(head)
        self.features = head + arch.auxiliary_features      # (a pass's index here = its plane of the DD_FUSE_INPUT=0 staging buffer)
        self.layout, self.emb_ch0 = tuple_layout(arch)
        self.n_entries = len(self.layout[0])

        # ---------------------------------------------------------------- inputs: standardize + variance
        self.raw = {f.name: torch.zeros((B, H, W, f.number_of_channels), dtype=torch.float32, device=dev) for f in self.features}
        VL = self.VL = max(e.nch for entries in self.layout for e in entries if e.kind == PASS)      # 3 + the widest variance of any pass
        # One launch assembles the network input from the raw passes (dd_assemble_input); only the head features' standardised sources
        # are also kept in fp32 (`sources`: what the kernel-prediction head filters and what generated passes echo).  DD_FUSE_INPUT=0: the
        # round-1 lowering, one dd_prepare_feature per pass into fp32 staging planes + dd_gather_input.
        self.fused_input = os.environ.get("DD_FUSE_INPUT", "1") != "0"
        self.sources = torch.zeros(((NF if self.fused_input else len(self.features)) * B, H, W, VL), dtype=torch.float32, device=dev)
        if not self.fused_input:
            for i, f in enumerate(self.features):
                self._prepare_op(f, i, VL, self.sources)
        self.raw3 = None
        if arch.use_kernel_prediction and not arch.use_standardized_source_for_kernel_prediction:
            self.raw3 = torch.zeros((NF * B, H, W, 3), dtype=torch.float32, device=dev)   # preserved sources (Architecture.py:105-112)
            for i, f in enumerate(head):
                self._prepare_op(f, i, 3, self.raw3, identity=True)

        # ---------------------------------------------------------------- network input (SourceEncoder)
        V = len(arch.feature_flag_names)
        self.emb = None
        if arch.feature_flag_mode == "EMBEDDING":
            self.emb = g.params.get("embedding/feature_flags_embedding_matrix", (V, V // 2), V, V // 2)
        self.flags_raw = {}
        if arch.feature_flag_mode == "ONE_HOT_ENCODING":
            self.flags_raw = {t.name: torch.zeros((B, H, W, V), dtype=torch.float32, device=dev) for t in tuples}
        X = self.X = g.tensor(T * B, H, W, arch.input_channels(), requires_grad=(training and self.emb is not None))
        self._atable_dev = torch.zeros(T * self.n_entries * C.sizeof(L.AssembleEntry), dtype=torch.uint8, device=dev)
        self._atable_ring = []           # pinned staging buffers of the assemble table upload
        self._atable_sources = None      # what the device table points at: "tiles" (self.raw) or "frames" (set_frame_sources)
        self._frame_ptrs = None
        # frame input (inference, Predictor): the render passes are read in place from whole frames, image b = the window at frame_origins[b]
        self.frame_input = None          # (frame_h, frame_w) once enable_frame_input() was called
        self.frame_origins = None        # [B, 2] int32 (y, x): written by the caller before every forward
        if self.fused_input:
            g.fwd(lambda stream: self._assemble(stream), "input_assembly")      # (a function of its own: the graph hangs attributes on it)
        else:
            g.fwd(g._defer(self._make_gather, "input_assembly"))
        if X.requires_grad:   # embedding-row gradients = column sums of dX over each tuple's images (FeatureFlags.py:57-67)
            g.on_backward(self._embedding_backward)

    def _prepare_op(self, f, index, ldd, dst, identity=False):
        g, lib, B, H, W = self.g, self.lib, self.B, self.H, self.W
        fp = feature_params(f, identity)
        raw = self.raw[f.name]
        ptr = dst.data_ptr() + index * B * H * W * ldd * 4
        cs = f.number_of_channels

        def run(stream, fp=fp):
            L.check(lib.dd_prepare_feature(raw.data_ptr(), cs, ptr, ldd, C.byref(fp), B, H, W, stream))
        g.fwd(run, "input_assembly")

    # ================================================================== the two tables (host only)
    def _plane_ptr(self, index):
        return self.sources.data_ptr() + index * self.B * self.H * self.W * self.VL * 4

    def _flag_ptr(self, t):
        """What the feature-flag entry of tuple t reads: its one-hot plane, or its row of the embedding matrix (fp32 master values)."""
        name = self.arch.feature_prediction_tuples[t].name
        if self.emb is None:
            return self.flags_raw[name].data_ptr()
        return self.g.params.value_ptr(self.emb) + self.arch.feature_flag_names.index(name) * self.emb.shape[1] * 4

    def fill_assemble_table(self, frames=None):
        """The dd_assemble_entry table [T, n_entries].  frames None: the passes are read from the tile buffers `raw`; else from the frame
        dictionary of set_frame_sources()."""
        tab = (L.AssembleEntry * (len(self.layout) * self.n_entries))()
        for t, entries in enumerate(self.layout):
            for e, (kind, f, head_i, nch, dst_ch) in enumerate(entries):
                en = tab[t * self.n_entries + e]
                en.kind, en.nch, en.dst_ch = kind, nch, dst_ch
                if kind != PASS:
                    en.src = self._flag_ptr(t)
                    continue
                en.src, en.cs, en.fp = (self.raw if frames is None else frames)[f.name].data_ptr(), f.number_of_channels, feature_params(f)
                if head_i is not None:
                    en.std_out, en.ld_std = self._plane_ptr(head_i), self.VL
        return tab

    def fill_gather_table(self):
        """The dd_gather_entry table [T, n_entries] of DD_FUSE_INPUT=0: the passes come from their staging planes of `sources`."""
        HW = self.H * self.W
        tab = (L.GatherEntry * (len(self.layout) * self.n_entries))()
        for t, entries in enumerate(self.layout):
            for e, (kind, f, head_i, nch, dst_ch) in enumerate(entries):
                if kind == PASS:
                    entry = L.GatherEntry(self._plane_ptr(self.features.index(f)), self.VL, HW, nch, dst_ch)
                elif kind == PLANE:
                    entry = L.GatherEntry(self._flag_ptr(t), nch, HW, nch, dst_ch)
                else:
                    entry = L.GatherEntry(self._flag_ptr(t), 0, 0, nch, dst_ch)
                tab[t * self.n_entries + e] = entry
        return tab

    # ================================================================== upload + launches
    def _upload_assemble_table(self, frames=None):
        # stream-ordered upload without a host synchronisation (a pageable copy_ waits for the stream: one stall per inference frame): a small
        # ring of pinned staging buffers, each reused only after the copy that read it has executed
        tab = self.fill_assemble_table(frames)
        ring = self._atable_ring
        if not ring:
            for _ in range(4):
                ring.append([torch.empty(self._atable_dev.numel(), dtype=torch.uint8, pin_memory=True), None])
        slot = ring.pop(0)
        ring.append(slot)
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].copy_(torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8))
        self._atable_dev.copy_(slot[0], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()

    def _assemble(self, stream):
        X, T = self.X, len(self.layout)
        if self.frame_input is not None:
            assert self._atable_sources == "frames", "enable_frame_input() without set_frame_sources()"
            L.check(self.lib.dd_assemble_input_frames(self._atable_dev.data_ptr(), T, self.n_entries, X.ptr, X.ld, X.Cp, self.B, self.H, self.W,
                                                      self.g.code, self.frame_origins.data_ptr(), self.frame_input[0], self.frame_input[1],
                                                      stream))
            return
        if self._atable_sources != "tiles":
            self._upload_assemble_table()
            self._atable_sources = "tiles"
        L.check(self.lib.dd_assemble_input(self._atable_dev.data_ptr(), T, self.n_entries, X.ptr, X.ld, X.Cp, self.B, self.H, self.W,
                                           self.g.code, stream))

    def _make_gather(self):
        X, T, n_entries, lib, code, B, H, W = self.X, len(self.layout), self.n_entries, self.lib, self.g.code, self.B, self.H, self.W
        table_dev = torch.frombuffer(bytearray(bytes(self.fill_gather_table())), dtype=torch.uint8).to(self.arch.device)

        def gather(stream, table_dev=table_dev):
            L.check(lib.dd_gather_input(table_dev.data_ptr(), T, n_entries, X.ptr, X.ld, X.Cp, B, H, W, code, stream))
        return gather

    def embedding_one_launch(self):
        """Whether dd_colsum_segments can take every tuple's column sums of dX at once: whole 16-byte vectors from the embedding's first channel."""
        ld, D, T = self.X.ld, self.emb.shape[1], len(self.layout)      # (dX has the layout of X)
        esz = 4 if self.g.dtype == "f32" else 2
        per16 = 16 // esz
        return (T <= 64 and D <= 8 * per16 and (self.emb_ch0 * esz) % 16 == 0 and ld % per16 == 0
                and self.emb_ch0 + -(-D // per16) * per16 <= ld)

    def _embedding_backward(self):
        X, g, lib, arch, emb, emb_ch0 = self.X, self.g, self.lib, self.arch, self.emb, self.emb_ch0
        if not X.grad_written:
            return
        gx = X.grad()
        D, T, rows = emb.shape[1], len(self.layout), self.B * self.H * self.W
        esz = 4 if g.dtype == "f32" else 2
        row_of = [arch.feature_flag_names.index(tup.name) for tup in arch.feature_prediction_tuples]
        rows_of = (C.c_int * T)(*row_of)
        one_launch = self.embedding_one_launch()

        def run(stream):
            if one_launch:      # every tuple's column sums in one launch (17 launches of 8 live lanes were 0.4 ms of the example step)
                L.check(lib.dd_colsum_segments(gx.ptr + emb_ch0 * esz, gx.ld, D, rows, T, g.params.grad_ptr(emb), D, rows_of, g.code, stream))
                return
            for t, row in enumerate(row_of):
                L.check(lib.dd_colsum(gx.ptr + (t * rows * gx.ld + emb_ch0) * esz, gx.ld, D, rows, g.params.grad_ptr(emb) + row * D * 4,
                                      g.code, stream))
        g.bwd(run, "bias_grad", grad_params=[emb])

    # ================================================================== running
    def set_inputs(self, features, non_blocking=False):
        """Copy the feature dictionary (device tensors, or pinned host tensors with non_blocking=True) into the static input buffers."""
        if self.frame_input is not None:      # a Predictor read whole frames in place through this (cached, shared) program: back to the tile buffers
            self.disable_frame_input()
        for f in self.features:
            self.raw[f.name].copy_(features[Naming.source_feature_name(f.name, index=0)], non_blocking=non_blocking)
        for name, buf in self.flags_raw.items():
            key = Naming.feature_flags_name(name)
            if key in features:
                buf.copy_(features[key], non_blocking=non_blocking)
            else:
                write_constant_flags(self.arch, name, buf)

    def enable_frame_input(self, frame_h, frame_w):
        """Inference on whole frames: the input assembly reads image b of every render pass as the H x W window at `frame_origins[b]` of the
        frame given by set_frame_sources() (dd_assemble_input_frames) instead of a copied tile in `raw`.  Call before the first forward (a
        captured hipGraph keeps the launch it was captured with); the caller writes frame_origins before every forward."""
        if not self.fused_input:
            raise RuntimeError("frame input needs the fused input assembly (DD_FUSE_INPUT=0 is set)")
        if self.frame_origins is None:
            self.frame_origins = torch.zeros((self.B, 2), dtype=torch.int32, device=self.arch.device)
        self.frame_input = (int(frame_h), int(frame_w))

    def set_frame_sources(self, frames):
        """frames: {feature name: contiguous fp32 device tensor [frame_h, frame_w, number_of_channels]} for every head / auxiliary feature.
        Only the device table of the assembly launch is rewritten (stream-ordered): captured graphs stay valid from frame to frame."""
        fh, fw = self.frame_input
        for f in self.features:
            t = frames[f.name]
            if tuple(t.shape) != (fh, fw, f.number_of_channels) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("%s: expected a contiguous float32 [%d,%d,%d] frame, got %s" % (f.name, fh, fw, f.number_of_channels, tuple(t.shape)))
        ptrs = tuple(frames[f.name].data_ptr() for f in self.features)
        if self._atable_sources == "frames" and ptrs == self._frame_ptrs:
            return          # the same device buffers as the last frame (a caller that refills its frame tensors): the table stands
        self._upload_assemble_table(frames)
        self._atable_sources, self._frame_ptrs = "frames", ptrs

    def disable_frame_input(self):
        """Back to tile input (`raw`): the device table is rewritten NOW, so a hipGraph captured in tile mode may be replayed again."""
        self.frame_input = None
        if self._atable_sources != "tiles":
            self._upload_assemble_table()
            self._atable_sources = "tiles"
