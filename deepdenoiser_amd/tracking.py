"""The launches behind Program.metrics(), Program.histograms() and Program.previews(): tracked metrics, histograms and image summaries.

Each class is built from a training Program on first use (Program.tracking_metrics / tracking_histograms / tracking_previews), so a program
that never asks pays nothing: no launch, no buffer, nothing in g.fwd_ops, in a captured graph or in profile_ops.  What is tracked and how the
device tables become values is metrics.py; the descriptors come from loss_desc.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import loss_desc as LD
from . import metrics as M


def _training(program, what):
    if not program.training:
        raise RuntimeError("%s() needs a training program (built with a Training.json): there are no targets otherwise" % what)


class Metrics:
    """Descriptors, scratch and the result table of the metric launches (dd_loss_metrics per scale of the plan, dd_loss_msssim_values).
    table: [scales x DD_METRIC_SOURCES x B x 4 | ms_ssim sources x B] per-image sums; rows: the floats of one scale's block."""

    def __init__(self, program):
        _training(program, "metrics")
        self.program = prog = program
        arch, tj, lib, B, dev = prog.arch, prog.training_json, prog.lib, prog.B, prog.arch.device
        self.plan = plan = M.metric_plan(arch, tj, histograms=prog.write_histograms)
        self.scales = scales = sorted({e.scale_index for e in plan if e.quantity != "ms_ssim"})
        assert all(k < len(prog.targets) for k in scales), "scaled targets exist whenever use_multiscale_metrics is set"
        use_image, use_comb = M.combined_levels(tj)
        triples = M.combined_triples(arch) if use_comb else []
        self.slot_of = LD.slot_table(prog.head, triples)
        masked_feat = any(e.quantity == "masked_mean" and e.source[0] == "feature" for e in plan)
        masked_comb = any(e.quantity == "masked_mean" and e.source[0] == "combined" for e in plan)
        self.rows = rows = L.METRIC_SOURCES * B * 4
        ms_sources = [e.source for e in plan if e.quantity == "ms_ssim"]
        self.table = table = torch.zeros(len(scales) * rows + len(ms_sources) * B, dtype=torch.float32, device=dev)
        self.launches, self.keep = [], []
        for j, s in enumerate(scales):
            h, w = prog.dims[s]
            d = LD.sources_desc(prog, s, triples, use_image)
            LD.fill_mask_features(d, prog.head, prog.head_index, triples, masked_feat, masked_comb)
            scratch = LD.device_scratch(lib.dd_loss_metrics_scratch_bytes(B, h, w), torch.float32, dev)
            out = table[j * rows:(j + 1) * rows]
            self.keep.append((d, scratch))

            def run(stream, d=d, h=h, w=w, scratch=scratch, out=out):
                L.check(lib.dd_loss_metrics(C.byref(d), B, h, w, scratch.data_ptr(), out.data_ptr(), stream))
            self.launches.append(run)
        if ms_sources:      # BaseFeatureTraining.ms_ssim, Training.py:178-204: always predicted[0] / target[0]
            h, w = prog.dims[0]
            LD.check_ms_ssim(prog.head, (h, w), 1.0 if any(src[0] == "feature" for src in ms_sources) else 0.0)
            m, n_sources = LD.ms_ssim_desc(LD.sources_desc(prog, 0, triples, use_image),      # (a positive weight selects the source)
                                           [1.0 if ("feature", f.name) in ms_sources else 0.0 for f in prog.head],
                                           [1.0 if ("combined", c) in ms_sources else 0.0 for c, _ in triples],
                                           1.0 if ("image", M.IMAGE_NAME) in ms_sources else 0.0)
            # dd_loss_msssim_values lists features in index order, then combined, then the image: the plan's order of ms_ssim entries
            ms_sources = ([("feature", f.name) for f in prog.head if ("feature", f.name) in ms_sources]
                          + [("combined", c) for c, _ in triples if ("combined", c) in ms_sources]
                          + [src for src in ms_sources if src[0] == "image"])
            assert n_sources == len(ms_sources)
            # (scratch of its own: the loss term's scratch feeds the backward)
            scratch = LD.device_scratch(lib.dd_loss_msssim_scratch_bytes(B, h, w, n_sources), torch.float32, dev)
            out = table[len(scales) * rows:]
            self.keep.append((m, scratch))

            def run_ms(stream, m=m, h=h, w=w, scratch=scratch, out=out):
                L.check(lib.dd_loss_msssim_values(C.byref(m), B, h, w, scratch.data_ptr(), out.data_ptr(), stream))
            self.launches.append(run_ms)
        self.ms_sources = ms_sources

    def run(self):
        """Program.metric_table()"""
        self.program.g.run(self.launches)
        return self.table

    def image_sums(self, table):
        """A device table of run() with its B rows per source summed: the float64 vector [scales x DD_METRIC_SOURCES x 4 | ms_ssim sources]
        that the ranks of a data-parallel run all-reduce and values(..., count=world * B) evaluates."""
        B, n = self.program.B, len(self.scales) * self.rows
        return torch.cat([table[:n].double().reshape(-1, B, 4).sum(dim=1).reshape(-1), table[n:].double().reshape(-1, B).sum(dim=1)])

    def values(self, table, real=None, count=None):
        """Program.metric_values()"""
        if not self.plan:
            return []
        host = table.detach().cpu().numpy() if torch.is_tensor(table) else table      # ONE device-to-host copy for all metrics
        n = len(self.scales)
        images = host.size // (n * L.METRIC_SOURCES * 4 + len(self.ms_sources))      # B, or 1 for rows that are sums over images
        rows = L.METRIC_SOURCES * images * 4
        assert host.size == n * rows + len(self.ms_sources) * images, "not a metric table of this program"
        tables = {s: host[j * rows:(j + 1) * rows].reshape(L.METRIC_SOURCES, images, 4) for j, s in enumerate(self.scales)}
        ms = host[n * rows:].reshape(len(self.ms_sources), -1) if self.ms_sources else None
        ms_values = {src: ms[j] for j, src in enumerate(self.ms_sources)}
        return M.metric_values(self.plan, self.slot_of, tables, self.program.dims, real, ms_values, count)


class Histograms:
    """Descriptors, selections, scratch and the device records of the histogram launches (dd_loss_histograms, one per scale of the plan).
    records are grouped by scale; order[r] is the plan entry of record r."""

    def __init__(self, program):
        _training(program, "histograms")
        self.program = prog = program
        arch, tj, lib, B, dev = prog.arch, prog.training_json, prog.lib, prog.B, prog.arch.device
        self.plan = plan = M.histogram_plan(arch, tj)
        scales = sorted({e.scale_index for e in plan})
        assert all(k < len(prog.targets) for k in scales), "scaled targets exist whenever use_multiscale_metrics is set"
        use_image, use_comb = M.combined_levels(tj)
        triples = M.combined_triples(arch) if use_comb else []
        slot_of = LD.slot_table(prog.head, triples)
        self.limits = M.histogram_limits()
        self.nb = nb = len(self.limits)
        rec_bytes = L.histogram_record_bytes(nb)
        limits = torch.from_numpy(self.limits).to(dev)
        self.records = torch.zeros(max(len(plan), 1) * rec_bytes, dtype=torch.uint8, device=dev)
        self.order, self.launches, self.keep = [], [], [limits]
        for s in scales:
            h, w = prog.dims[s]
            entries = [i for i, e in enumerate(plan) if e.scale_index == s]
            d = LD.sources_desc(prog, s, triples, use_image)
            LD.fill_mask_features(d, prog.head, prog.head_index, triples, True, True, missing_ok=True)
            sel = (C.c_int * (2 * len(entries)))()
            for r, i in enumerate(entries):
                sel[2 * r], sel[2 * r + 1] = slot_of[plan[i].source], M.HISTOGRAM_KINDS.index(plan[i].kind)
            scratch = LD.device_scratch(lib.dd_loss_histograms_scratch_bytes(B, h, w, len(entries)), torch.float64, dev)
            out = self.records[len(self.order) * rec_bytes:(len(self.order) + len(entries)) * rec_bytes]
            self.order += entries
            self.keep.append((d, sel, scratch))

            def run(stream, d=d, h=h, w=w, sel=sel, n=len(entries), scratch=scratch, out=out):
                L.check(lib.dd_loss_histograms(C.byref(d), B, h, w, sel, n, limits.data_ptr(), nb, out.data_ptr(), scratch.data_ptr(), stream))
            self.launches.append(run)

    def run(self):
        """Program.histogram_table()"""
        self.program.g.run(self.launches)
        return self.records

    def host_table(self, records=None):
        """Program.histogram_host_table()"""
        records = self.run() if records is None else records
        host = records.detach().cpu().numpy() if torch.is_tensor(records) else records
        n = len(self.plan)
        table = M.decode_histogram_records(host[:n * L.histogram_record_bytes(self.nb)], n, self.nb)
        back = [0] * n
        for r, i in enumerate(self.order):
            back[i] = r
        return {k: v[back] for k, v in table.items()}

    def values(self, out=print):
        """Program.histograms()"""
        if not self.plan:
            return []
        return M.histogram_values(self.plan, self.host_table(), self.limits, out=out)


class Previews:
    """Descriptor, source table and threshold table of the preview launch (dd_loss_previews, scale 0); `out`: the device bytes per shape."""

    def __init__(self, program):
        _training(program, "previews")
        self.program = prog = program
        arch, tj = prog.arch, prog.training_json
        triples = M.combined_triples(arch)
        self.desc = LD.sources_desc(prog, 0, triples, M.image_members(arch) is not None)
        self.source, self.source_ld = (C.c_void_p * L.MAX_FEATURES)(), (C.c_int * L.MAX_FEATURES)()
        for i, f in enumerate(prog.head):      # the raw noisy passes as set_inputs() leaves them
            self.source[i], self.source_ld[i] = prog.raw[f.name].data_ptr(), f.number_of_channels
        self.slot_of = LD.slot_table(prog.head, triples)
        self.thresholds = torch.from_numpy(M.preview_thresholds()).to(arch.device)
        self.out = {}
        self.plans = {w: M.preview_plan(arch, tj, w) for w in ("combined", "all")}

    def plan(self, which="combined"):
        """Program.preview_plan()"""
        if which not in self.plans:
            raise ValueError("previews: which = %r ('combined' or 'all')" % (which,))
        return self.plans[which]

    def run(self, images=(0, 1, 2), which="combined", panels=("source", "prediction", "target"), exposure=1.0, error_gain=1.0):
        """Program.preview_table()"""
        prog = self.program
        plan, mask = self.plan(which), M.preview_panel_mask(panels)
        images = [int(b) for b in images]
        if not plan:
            raise ValueError("previews: the architecture has no source to show")
        P = bin(mask).count("1")
        shape = (len(plan), len(images) * prog.H, P * prog.W, 3)
        if shape not in self.out:
            self.out[shape] = torch.zeros(shape, dtype=torch.uint8, device=prog.arch.device)
        out = self.out[shape]
        img = (C.c_int * max(len(images), 1))(*images)
        slots = (C.c_int * len(plan))(*[self.slot_of[e.source] for e in plan])

        def run(stream):
            L.check(prog.lib.dd_loss_previews(C.byref(self.desc), self.source, self.source_ld, prog.B, prog.H, prog.W, img, len(images), slots,
                                              len(plan), mask, self.thresholds.data_ptr(), float(exposure), float(error_gain), out.data_ptr(),
                                              stream))
        prog.g.run([run])
        return out

    def images(self, table, images, which="combined"):
        """Program.preview_images()"""
        H = self.program.H
        host = table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
        plan, n = self.plan(which), len(images)
        assert host.shape[0] == len(plan) and host.shape[1] == n * H, "not a preview table of this plan"
        return [(tag, host[j, k * H:(k + 1) * H]) for j, e in enumerate(plan) for k, tag in enumerate(M.preview_tags(e.name, n))]

    def previews(self, images=(0, 1, 2), which="combined", panels=("source", "prediction", "target"), exposure=1.0, error_gain=1.0):
        """Program.previews()"""
        images = list(images)
        return self.images(self.run(images, which, panels, exposure, error_gain), images, which)
