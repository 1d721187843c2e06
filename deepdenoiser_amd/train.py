"""`python -m deepdenoiser_amd.train training.json` -- the reference's `python Training.py training.json` (TensorFlow/Training.py:33-61 argument
set, :944-1289 main) on the MI355X path: TFRecord tiles -> device augmentation -> Trainer.step -> TensorFlow-format checkpoints in the
architecture's model_directory.  One process per GPU under torch.distributed.run shards every mini-batch over the ranks.

Input pipeline (Training.py:826-843): the file list is shuffled per epoch, records are decoded by `--threads` background threads, examples pass a
shuffle buffer of 20 x batch_size, mini-batches are stacked into pinned host memory `prefetch` (5) deep and uploaded on a copy stream while the
previous step runs.  Every random choice comes from an RNG seeded by (seed, epoch) that all ranks share, so the ranks see the SAME sequence of
mini-batches and each takes every world-th one; an epoch is cut to a multiple of `world` mini-batches, so every rank runs the same number of
steps (and collectives).  `--validate` is a validation-only run; otherwise every `--validation_interval` epochs are followed by a validation
pass over base/validation/<spp>/ for every validation*.json (Training.py:1230-1284).

Summaries (metrics.py, summaries.py): every `--summary_steps` steps (100 = the Estimator's save_summary_steps, Training.py:1214) rank 0 writes
`loss`, `learning_rate`, `batch_size` (Training.py:676-677) and the tracked scalars of Training.json's statistics sections (Training.py:688-698)
for the current mini-batch into a TensorBoard event file in the model directory; a validation pass averages the same metrics over the
validation set (eval_metric_ops, Training.py:704-719), prints them and writes them with `loss` into <model_directory>/eval_<validation json stem>/
(estimator.evaluate(name=...), Training.py:874-877).  With `--histograms` the same training event also carries the histograms the
*_histogram flags of the statistics sections ask for (tf.summary.histogram, Training.py:679-686; metrics.histogram_plan), binned on the device
from the forward that yields the tracked scalars; validation passes write none (the reference adds them in TRAIN mode only).  Without the
flag the *_histogram keys are read and, said once, not written.

Image summaries (new: the reference writes none): with `--image_steps N` rank 0 renders, every N steps, the first `--image_count` examples of
its staged mini-batch as source | prediction | target [| difference, `--image_difference`] previews of the sources `--images` names
(metrics.preview_plan), on the device from the pre-step forward (shared with the tracked scalars when both fall on one step), and writes them
as ONE event of their own that holds only the images.  Every validation pass then also writes the previews of the first examples of each
validation set's first mini-batch into that set's eval_<name> event file at the global step: that stream is not shuffled, so the same
tiles appear every epoch.  No collective: the other ranks do nothing.  Not reproduced: histograms of weights or gradients.

Frames on the device (new: the reference trains from tile records only): with `--frames tfrecords.json` (or "frames" in Training.json) the
rendered EXRs the TFRecords-JSON names are decoded once and kept as fp32 planes in device memory (frame_bank.py); base_tfrecords_directory is
not read and no .tfrecords file is needed.  A mini-batch is then B records (plane, origin, augmentation draw) and ONE dd_sample_tiles launch
that crops and augments every pass into the program's input and target buffers; TileStream, Uploader and DataAugmentation.apply are not
used.  `--frames_crops random` cuts the tiles anywhere in a frame, `grid` on the fixed grid of the tile sets; an epoch has as many examples
as the grid in either mode.  `--frames_crops importance` draws the tiles where the noisy sources differ from the target: one
dd_importance_cells launch scores the training frames when they are loaded, the draw stays on the host (frame_importance.py; the floor
`--frames_importance_floor`, the cell side `--frames_importance_cell`, the density as pictures `--frames_importance_png`).  With
`--frames_importance_refresh N` the scores follow the model: one dd_importance_update launch inside every step scores the cells the
mini-batch covers by the SMAPE between prediction and target, and every N steps the visited cells of the map move towards it by
`--frames_importance_rate` (all ranks add their integer tables, so all hold the same map).  Validation runs over the grid of the JSON's
validation mode, without augmentation."""
import argparse
import json
import multiprocessing
import os
import queue
import random
import threading
import time

import numpy as np
import torch

from . import grad_clip, loss_scale, summaries, tf_checkpoint, tfrecords
from .architecture import Architecture
from .data_augmentation import DataAugmentation, DataAugmentationUsage
from .metrics import MeanAccumulator
from .naming import Naming
from .tiling import source_index_tuples
from .training import Trainer


IMPORTANCE_FLAGS = ("frames_importance_floor", "frames_importance_cell", "frames_importance_png", "frames_importance_refresh")


class _Parser(argparse.ArgumentParser):
    """The sub-options of `--frames_crops importance` are refused without it (by name), `--frames_importance_rate` without
    `--frames_importance_refresh`; the defaults of the floor and the rate are filled in afterwards, so that a given value can be told from
    the default."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.frames_crops != "importance":
            for name in IMPORTANCE_FLAGS:
                if getattr(ns, name) is not None:
                    self.error("--%s needs --frames_crops importance" % name)
        if ns.frames_importance_refresh is None and ns.frames_importance_rate is not None:
            self.error("--frames_importance_rate needs --frames_importance_refresh")
        if ns.frames_importance_refresh is not None and ns.frames_importance_refresh < 1:
            self.error("--frames_importance_refresh: %d (at least 1 step)" % ns.frames_importance_refresh)
        if ns.frames_importance_floor is None:
            from .frame_importance import DEFAULT_FLOOR
            ns.frames_importance_floor = DEFAULT_FLOOR
        if ns.frames_importance_rate is None:
            from .frame_importance import DEFAULT_RATE
            ns.frames_importance_rate = DEFAULT_RATE
        elif not 0.0 < ns.frames_importance_rate <= 1.0:
            self.error("--frames_importance_rate: %r (above 0, at most 1)" % ns.frames_importance_rate)
        return ns


def parser():
    p = _Parser(description="Training for the DeepDenoiser (MI355X-native hot path).")
    p.add_argument("json_filename", help="The json specifying all the relevant details.")
    p.add_argument("--validate", action="store_true", help="Perform a validation step.")
    p.add_argument("--threads", type=int, default=multiprocessing.cpu_count() + 1, help="Number of threads to use (host-side decoding)")
    p.add_argument("--train_epochs", type=int, default=10000, help="Number of epochs to train.")
    p.add_argument("--validation_interval", type=int, default=1, help="Number of epochs after which a validation is made.")
    p.add_argument("--data_format", type=str, default="channels_first", choices=["channels_first", "channels_last"],
                   help="Accepted for compatibility: the MI355X path is NHWC-native, both values give the same results.")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"], help="storage type of activations (accumulation is fp32)")
    p.add_argument("--summary_steps", type=int, default=100,
                   help="Write the loss and the tracked metrics of the current mini-batch as TensorBoard scalars every this many steps (0: never).")
    p.add_argument("--histograms", action="store_true",
                   help="Also write the histograms that the *_histogram flags of Training.json ask for, every --summary_steps steps "
                        "(binned on the device; a tag with an inf / NaN value is left out for that step).")
    p.add_argument("--image_steps", type=int, default=0,
                   help="Write image summaries (source | prediction | target previews, rendered on the device) every this many steps and "
                        "with every validation pass (0: never).")
    p.add_argument("--images", default="combined", choices=["combined", "all"],
                   help="Which sources get a preview: the combined image and the combined features, or also every predicted pass.")
    p.add_argument("--image_count", type=int, default=3, help="Examples of the mini-batch per preview (tf.summary.image's max_outputs).")
    p.add_argument("--image_exposure", type=float, default=1.0, help="Factor applied to the values of a preview before the sRGB quantisation.")
    p.add_argument("--image_difference", action="store_true", help="Add a fourth panel: the absolute loss difference of prediction and target.")
    p.add_argument("--loss_scale", type=loss_scale.cli_value, default=None, metavar="{dynamic,<number>}",
                   help="Loss scale of the optimisation step: 'dynamic' keeps it on the device (halved on an inf / NaN gradient, whose step is skipped, "
                        "doubled after 2000 applied steps), a positive number fixes it.  Default: 4096 for f16, 1 for bf16 / f32.")
    p.add_argument("--clip_norm", type=grad_clip.cli_value, default=None, metavar="X",
                   help="Clip the gradients by their global norm (tf.clip_by_global_norm) on the device: they are multiplied by X / max(norm, X).  "
                        "Overrides the optional \"gradient_clip_norm\" of Training.json; absent, null or 0: off.")
    p.add_argument("--gradient_norms", action="store_true",
                   help="Every --summary_steps steps also write gradient_norm/<variable> and weight_norm/<variable> of every variable and "
                        "gradient_nonfinite_variables (the global gradient_norm and gradient_clip_coefficient are written whenever this or "
                        "clipping is on).")
    p.add_argument("--frames", default=None, metavar="PATH",
                   help="Train from rendered EXR frames kept in device memory instead of .tfrecords tiles: the TFRecords-JSON (the schema of "
                        "TFRecordsExample.json) that names the scene directories.  Overrides the optional \"frames\" of Training.json; "
                        "base_tfrecords_directory is then not read.")
    p.add_argument("--frames_spp", type=int, default=None, help="Samples per pixel of the source renderings (default: the first of source.samples_per_pixel).")
    p.add_argument("--frames_crops", default="random", choices=["random", "grid", "importance"],
                   help="Where the tiles of a mini-batch are cut: anywhere in a frame, on the fixed grid of the .tfrecords tile sets "
                        "(shuffled per epoch), or anywhere with a probability that grows with the SMAPE between the noisy sources and the "
                        "target inside the tile (scored on the device when the frames are loaded; this changes the training distribution on "
                        "purpose, no loss re-weighting is applied).  An epoch has as many examples as the grid in every mode.")
    p.add_argument("--frames_importance_floor", type=float, default=None, metavar="F",
                   help="With --frames_crops importance: the share of the draws that ignores the scores (0 .. 1), so that easy regions do not "
                        "vanish.  Default 0.25: a choice, not a measured optimum.")
    p.add_argument("--frames_importance_cell", type=int, default=None, metavar="G",
                   help="With --frames_crops importance: the side of the cells the frames are scored in (1 .. 64, a divisor of the tile; "
                        "default: the largest of 16, 8, 4, 2, 1 that divides it).")
    p.add_argument("--frames_importance_png", default=None, metavar="DIR",
                   help="With --frames_crops importance: rank 0 writes the density as <scene directory name>_importance.png per training scene into DIR.")
    p.add_argument("--frames_importance_refresh", type=int, default=None, metavar="N",
                   help="With --frames_crops importance: every N steps (at least 1) move the scores of the cells the mini-batches covered "
                        "towards the error the model made there (the SMAPE between prediction and target, scored by one launch inside every "
                        "step), so that the draws follow what the model still gets wrong.  Off by default; not saved with a checkpoint.")
    p.add_argument("--frames_importance_rate", type=float, default=None, metavar="A",
                   help="With --frames_importance_refresh: how far a visited cell moves towards the model's error at a refresh (above 0, at "
                        "most 1; 1 replaces the score).  Default 0.5: a choice, not a measured optimum.")
    p.add_argument("--exr_decode", default="host", choices=["host", "device"],
                   help="--frames: where the EXR files are decoded: on the host, or inflated on the host and rebuilt on the device by one launch per scene.")
    from . import openexr
    openexr.add_inflate_argument(p, "--frames")
    p.add_argument("--frame_memory_gb", type=float, default=None,
                   help="The most device memory the frames may take (default: 80 %% of what is free when they are loaded).")
    p.add_argument("--seed", type=int, default=0, help="seed of the file / example shuffles and of the source index tuples (shared by all ranks)")
    return p


def gradient_scalars(report, per_variable=False):
    """[(tag, value)] of a grad_clip report: gradient_norm and gradient_clip_coefficient; per_variable (--gradient_norms): also
    gradient_nonfinite_variables and gradient_norm/<variable>, weight_norm/<variable> of every variable, in creation order."""
    out = [("gradient_norm", report["grad_norm"]), ("gradient_clip_coefficient", report["coef"])]
    if per_variable:
        out.append(("gradient_nonfinite_variables", report["nonfinite_variables"]))
        out += [("gradient_norm/" + name, v["grad_norm"]) for name, v in report["variables"].items()]
        out += [("weight_norm/" + name, v["weight_norm"]) for name, v in report["variables"].items()]
    return out


def evaluation_jsons(base, mode):
    """<mode>*.json next to the tfrecords directories, statistics files excluded (Training.py:916-927)."""
    out = []
    for name in sorted(os.listdir(base)):
        stem, ext = os.path.splitext(name)
        if stem.startswith(mode) and ext == ".json" and "statistics" not in stem and os.path.isfile(os.path.join(base, name)):
            out.append(name)
    return out


class TileStream:
    """Mini-batches of one epoch for this rank: an iterator of (features, labels) dictionaries of pinned host tensors.

    directory: the <mode>[/<spp>] directory of .tfrecords.gz files; `rng`: random.Random shared by all ranks (None: file and record order,
    as validation reads them); `threads` decoder threads each own a file at a time and hand decoded examples to the batcher IN FILE ORDER
    (the shuffled order), so the sequence of examples does not depend on thread timing."""

    def __init__(self, directory, mode, arch, batch, tile, spp, index_tuples, rank=0, world=1, rng=None, threads=4, prefetch=5, pinned=True,
                 pad_last=False):
        """pad_last (validation): the examples left over after the last whole round of `world` mini-batches are evaluated too -- the round is
        filled up by repeating examples from the start of the epoch (`padded` counts them; the reference's dataset.batch() evaluates the
        remainder as a smaller batch, a static launch program cannot).  Without it they are dropped and counted in `dropped`."""
        self.arch, self.batch, self.tile, self.spp, self.tuples = arch, batch, tile, spp, index_tuples
        self.rank, self.world, self.rng, self.prefetch, self.pinned = rank, world, rng, prefetch, pinned
        self.pad_last, self.padded, self.dropped, self._const = pad_last, 0, 0, {}
        self.real_in_last = batch          # real (not repeated) examples in this rank's LAST mini-batch of the epoch (pad_last)
        self.passes = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
        self.targets = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
        self.required = sorted({i for t in index_tuples for i in t})
        self.files = tfrecords.list_files(directory, mode)
        if rng is not None:
            rng.shuffle(self.files)                                     # Training.py:826-828 (files.shuffle)
        self.threads = max(1, min(int(threads), len(self.files), 32))
        self.decoded = 0

    def _decode_file(self, path):
        out = []
        for rec in tfrecords.read_records(path):
            src, tgt = tfrecords.decode_example(tfrecords.parse_example(rec), self.passes, self.tile, [self.spp], self.required, self.targets)
            for tup in self.tuples:                                     # one training example per (source index tuple, target): Training.py:544-549
                out.append((src[self.spp][tup[0]], tgt))
        return out

    def _examples(self):
        """Decoded examples in (shuffled) file order; files are decoded `threads` at a time, at most 2 x threads files ahead."""
        slots = [queue.Queue(maxsize=1) for _ in self.files]
        ahead = threading.Semaphore(2 * self.threads)
        nxt = iter(range(len(self.files)))
        lock = threading.Lock()

        def worker():
            while True:
                # the look-ahead permit comes BEFORE the index, both under one lock: a permit holder then always owns the lowest outstanding
                # index (taken the other way round the other workers could park 2 x threads later files, take every permit, and leave the
                # worker holding the index the consumer waits for without one: ADVICE r4)
                with lock:
                    ahead.acquire()
                    i = next(nxt, None)
                if i is None:
                    ahead.release()
                    return
                try:
                    slots[i].put(self._decode_file(self.files[i]))
                except BaseException as e:                               # surfaces in the consumer
                    slots[i].put(e)
        pool = [threading.Thread(target=worker, daemon=True) for _ in range(self.threads)]
        for t in pool:
            t.start()
        for i in range(len(self.files)):
            got = slots[i].get()
            ahead.release()
            if isinstance(got, BaseException):
                raise got
            yield from got

    def _shuffled(self):
        """Training.py:836-838: a shuffle buffer of 20 x batch_size examples."""
        if self.rng is None:
            yield from self._examples()
            return
        size, buf = 20 * self.batch, []
        for ex in self._examples():
            if len(buf) < size:
                buf.append(ex)
                continue
            j = self.rng.randrange(size)
            buf[j], ex = ex, buf[j]
            yield ex
        self.rng.shuffle(buf)
        yield from buf

    def _stack(self, group):
        feats, labels = {}, {}
        B, tile = self.batch, self.tile

        def host(shape):      # (allocated pinned: empty(...).pin_memory() allocates pageable memory and copies its garbage into a second buffer)
            return torch.empty(shape, dtype=torch.float32, pin_memory=bool(self.pinned and torch.cuda.is_available()))
        for k, ch in self.passes.items():
            t = host((B, tile, tile, ch))
            np.stack([s[k] for s, _ in group], out=t.numpy())
            feats[Naming.source_feature_name(k, index=0)] = t
        for k in self.targets:
            t = host((B, tile, tile, self.passes[k]))
            np.stack([tg[k] for _, tg in group], out=t.numpy())
            labels[Naming.target_feature_name(k)] = t
        for f in self.arch.feature_predictions + self.arch.auxiliary_features:      # generated passes (Training.py:531-538)
            if not f.load_data:
                value = 1.0 if f.feature_prediction_type == "COLOR" else 0.5
                key = (f.number_of_channels, value)
                if key not in self._const:      # constant passes: one (pinned) tensor for the whole stream, not one per mini-batch
                    self._const[key] = host((B, tile, tile, f.number_of_channels)).fill_(value)
                feats[Naming.source_feature_name(f.name, index=0)] = self._const[key]
                if f.is_target:
                    labels[Naming.target_feature_name(f.name)] = self._const[key]
        return feats, labels

    def __iter__(self):
        """This rank's mini-batches; a background thread keeps `prefetch` of them stacked ahead of the consumer."""
        ready = queue.Queue(maxsize=self.prefetch)
        END = object()

        def producer():
            try:
                group, buf, head = [], [], []
                need = self.batch * self.world

                def feed(ex):
                    nonlocal group, buf
                    buf.append(ex)
                    if len(buf) == self.batch:
                        group.append(buf)
                        buf = []
                        if len(group) == self.world:                     # only whole rounds of `world` mini-batches: every rank gets one
                            ready.put(self._stack(group[self.rank]))
                            group = []
                for ex in self._shuffled():
                    self.decoded += 1
                    if self.pad_last and len(head) < need:
                        head.append(ex)
                    feed(ex)
                left = len(group) * self.batch + len(buf)
                if left and self.pad_last and head:
                    # fill the last round by cycling over ITS OWN examples (not the start of the epoch: those would be counted twice), and
                    # tell the consumer how many of this rank's last mini-batch are real: it weighs that mini-batch's mean by the count, a
                    # mini-batch of repeats only by zero (the fixed-size programme cannot evaluate a smaller remainder batch)
                    tail = [ex for b in group for ex in b] + list(buf)
                    self.real_in_last = max(0, min(self.batch, left - self.rank * self.batch))
                    for k in range(need - left):
                        feed(tail[k % len(tail)])
                    self.padded = need - left
                else:
                    self.dropped = left
                ready.put(END)
            except BaseException as e:
                ready.put(e)
        threading.Thread(target=producer, daemon=True).start()
        while True:
            item = ready.get()
            if item is END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item


class Uploader:
    """Host -> device copies of the next mini-batch on a side stream while the current step runs; the consumer's stream waits on the copy's
    event, the copy waits until the step that read the previous contents of the staging tensors has been enqueued."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)

    def stage(self, feats, labels):
        done = torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            df = {k: v.to(self.device, non_blocking=True) for k, v in feats.items()}
            dl = {k: v.to(self.device, non_blocking=True) for k, v in labels.items()}
            done.record(self.stream)
        return df, dl, done, (feats, labels)                            # (the pinned sources stay alive until the copy has run)


def preview_settings(args, B):
    """The keyword arguments of Program.preview_table for the command line's --image_* flags, or None when image summaries are off."""
    if args.image_steps <= 0:
        return None
    if not 1 <= args.image_count <= 16:
        raise ValueError("--image_count %d: 1 .. 16 examples fit one preview launch" % args.image_count)
    panels = ("source", "prediction", "target") + (("difference",) if args.image_difference else ())
    return {"images": list(range(min(args.image_count, B))), "which": args.images, "panels": panels, "exposure": args.image_exposure}


def preview_summaries(prog, table, preview):
    """[(tag, height, width, colorspace, png)] of a preview table (Program.preview_table): one copy from the device, one PNG per image."""
    return [summaries.image_summary(tag, a) for tag, a in prog.preview_images(table, preview["images"], preview["which"])]


def _evaluate_set(trainer, arch, stem, feeds, tail, B, rank, world, plan, metrics_out, previews_out, preview, printed=None):
    """One validation set.  `feeds` yields once per mini-batch of this rank, AFTER it has put that mini-batch into the program's input
    buffers; tail() -> (padded, real_in_last, decoded) once it is exhausted.  Returns (stem, mean loss, examples) or None for an empty set."""
    import torch.distributed as dist
    total = torch.zeros(2, dtype=torch.float64, device=arch.device)
    losses, tables = [], []
    for _ in feeds:
        trainer.program.zero_grads()
        trainer.program.forward()
        losses.append(trainer.program.loss_buf.double().sum())
        if plan:      # (a copy on the device: how many of the LAST mini-batch are real is known only when the stream has ended)
            tables.append(trainer.program.metric_table().clone())
        if previews_out is not None and preview is not None and len(losses) == 1:
            previews_out[stem] = preview_summaries(trainer.program, trainer.program.preview_table(**preview), preview)
    padded, real_in_last, decoded = tail()
    # every example counts once: a mini-batch's mean is weighed by its REAL examples (the last round of the epoch is filled with repeats)
    for i, l in enumerate(losses):
        w = real_in_last if (padded and i == len(losses) - 1) else B
        total[0] += l * w
        total[1] += w
    if world > 1:
        dist.all_reduce(total)
    if plan:
        acc = MeanAccumulator(len(plan))
        for i, t in enumerate(tables):
            w = real_in_last if (padded and i == len(tables) - 1) else B
            if w > 0:      # repeated examples do not count
                acc.add(trainer.program.metric_values(t, real=w), w)
        if world > 1:
            state = torch.from_numpy(acc.state()).to(arch.device)
            dist.all_reduce(state)
            acc.from_state(state.cpu().numpy())
        if acc.weight > 0:
            metrics_out[stem] = list(zip([e.name for e in plan], acc.result()))
    if float(total[1]) > 0:
        if padded and rank == 0:
            print("validation set %s: the last round was filled up with %d repeated example(s) (%d decoded)" % (printed or stem, padded, decoded))
        return stem, float(total[0] / total[1]), int(total[1])
    return None


def run_validation(trainer, arch, tj, base, B, rank, world, threads, metrics_out=None, previews_out=None, preview=None):
    """Training.py:1230-1250 / :1264-1284: every validation*.json, tiles of base/validation/<spp>/, no augmentation, mean loss.
    metrics_out: a dict that receives {validation json stem: [(metric name, mean over the set)]} -- the tracked metrics of every mini-batch
    (program.metrics over its real examples), averaged with the weights the loss gets.  previews_out (with `preview`, preview_settings): a
    dict that receives {stem: image summaries of the first examples of the set's first mini-batch} -- on the rank that passes it only."""
    results = []
    plan = trainer.program.metric_plan() if metrics_out is not None else []
    for name in evaluation_jsons(base, "validation"):
        st = json.load(open(os.path.join(base, name), encoding="utf-8"))
        spp = st["source_samples_per_pixel_list"][0]
        vdir = os.path.join(base, "validation", str(spp))
        if not os.path.isdir(vdir):
            vdir = os.path.join(base, "validation")                      # data sets written without group_by_samples_per_pixel
        tuples, _ = source_index_tuples(st["number_of_sources_per_example"], tj["number_of_source_index_tuples"], arch.number_of_sources_per_target,
                                        rng=random.Random(0))
        if st["tiles_height_width"] != trainer.program.H:
            print("validation set %s: tiles of %d pixels, the program was built for %d -- skipped" % (name, st["tiles_height_width"], trainer.program.H))
            continue
        stream = TileStream(vdir, "validation", arch, B, st["tiles_height_width"], spp, tuples, rank, world, rng=None, threads=threads, pad_last=True)

        def feeds(stream=stream):
            for feats, labels in stream:
                trainer.program.set_inputs({k: v.to(arch.device) for k, v in feats.items()}, {k: v.to(arch.device) for k, v in labels.items()})
                yield
        got = _evaluate_set(trainer, arch, os.path.splitext(name)[0], feeds(), lambda: (stream.padded, stream.real_in_last, stream.decoded), B, rank,
                            world, plan, metrics_out, previews_out, preview, printed=name)
        if got is not None:
            results.append(got)
    return results


def run_validation_frames(trainer, arch, tj, sampler, B, rank, world, metrics_out=None, previews_out=None, preview=None, stem="validation"):
    """The validation pass of a --frames run: the grid records of the validation frames (frame_bank.TileSampler.grid_records), no
    augmentation; the last round is filled up by cycling over its own examples and weighed by the real ones, as run_validation does."""
    plan = trainer.program.metric_plan() if metrics_out is not None else []
    tuples, _ = source_index_tuples(sampler.bank.S, tj["number_of_source_index_tuples"], arch.number_of_sources_per_target, rng=random.Random(0))
    records = sampler.grid_records(tuples)
    need, count = B * world, len(records)
    left = count % need
    padded, real_in_last = 0, B
    if left:
        tail = records[count - left:]
        records = np.concatenate([records, tail[np.arange(need - left) % left]])
        padded, real_in_last = need - left, max(0, min(B, left - rank * B))

    def feeds():
        for r0 in range(0, len(records), need):
            sampler.sample(records[r0 + rank * B:r0 + (rank + 1) * B])
            yield
    got = _evaluate_set(trainer, arch, stem, feeds(), lambda: (padded, real_in_last, count), B, rank, world, plan, metrics_out, previews_out, preview)
    return [got] if got is not None else []


def main(args):
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    tj = json.load(open(args.json_filename, encoding="utf-8"))
    directory = os.path.dirname(os.path.abspath(args.json_filename))
    aj = json.load(open(os.path.join(directory, tj["architecture"])))
    arch = Architecture(aj, source_data_format="channels_last", data_format=args.data_format, device="cuda:%d" % local, dtype=args.dtype,
                        loss_scale=args.loss_scale, clip_norm=grad_clip.resolve_clip_norm(args.clip_norm, tj),
                        track_gradient_norms=args.gradient_norms)
    if "training" not in tj["modes"]:
        raise Exception("No training mode found.")
    frames_json = args.frames
    if frames_json is None and tj.get("frames"):
        frames_json = tj["frames"] if os.path.isabs(tj["frames"]) else os.path.join(directory, tj["frames"])
    base = frame_set = None
    if frames_json is not None:      # frames kept on the device (frame_bank.py): no .tfrecords, base_tfrecords_directory is not read
        from .frame_bank import FrameBank, FrameSet, TileSampler
        frame_set = FrameSet.from_json(frames_json, "training", log=print if rank == 0 else (lambda *a: None))
        st = {"tiles_height_width": frame_set.tile, "number_of_sources_per_example": frame_set.number_of_sources_per_example,
              "source_samples_per_pixel_list": [frame_set.source_spps[0] if args.frames_spp is None else args.frames_spp]}
    else:
        base = tj["base_tfrecords_directory"] if os.path.isabs(tj["base_tfrecords_directory"]) else os.path.join(directory, tj["base_tfrecords_directory"])
        st = tfrecords.read_settings(base, "training")
    spp = st["source_samples_per_pixel_list"][0]
    B, tile = tj["batch_size"], st["tiles_height_width"]
    trainer = Trainer(arch, tj, B, tile, tile, world_size=world)
    model_dir = aj["model_directory"] if os.path.isabs(aj["model_directory"]) else os.path.join(directory, aj["model_directory"])
    step = 0
    latest = tf_checkpoint.latest_checkpoint(model_dir) if os.path.isdir(model_dir) else None
    if latest:
        step = tf_checkpoint.load_variables(arch, latest)["global_step"]
        print("restored %s (global_step %d)" % (latest, step))
    validate = "validation" in tj["modes"]
    usage = DataAugmentationUsage.from_training_json(tj)
    sampler = validation_sampler = scorer = None
    if frame_set is not None:
        quiet = print if rank == 0 else (lambda *a: None)
        limit = None if args.frame_memory_gb is None else int(args.frame_memory_gb * 2 ** 30)
        threads = max(1, min(args.threads, 8))      # EXR decoders: a small fixed cap, whatever the host has

        def resident(mode, frames):
            bank = FrameBank(arch, frames, spp, arch.device, limit, threads=threads, log=quiet, decode=args.exr_decode, inflate=args.exr_inflate)
            quiet("frames: %s -- %d scene(s), %d planes, %.3f GB on the device (%d spp, tiles of %d)"
                  % (mode, len(bank.scenes), bank.n_planes, bank.total_bytes / 1e9, bank.spp, bank.tile))
            return TileSampler(trainer.program, bank, usage)
        if not args.validate:
            sampler = resident("training", frame_set)
            if args.frames_crops == "importance":      # scored once, on every rank (each holds the whole bank: the same table everywhere)
                from .frame_importance import ImportanceMap
                importance = ImportanceMap(sampler.bank, cell=args.frames_importance_cell, floor=args.frames_importance_floor)
                sampler.set_importance(importance)
                quiet(importance.describe())

                def write_importance_pngs():
                    if args.frames_importance_png is None or rank != 0:
                        return
                    os.makedirs(args.frames_importance_png, exist_ok=True)
                    for s, scene in enumerate(sampler.bank.scenes):
                        name = os.path.basename(os.path.normpath(scene.directory)) + "_importance.png"
                        with open(os.path.join(args.frames_importance_png, name), "wb") as f:
                            f.write(summaries.encode_png(importance.picture(s)))
                write_importance_pngs()
                if args.frames_importance_refresh is not None:      # one more launch inside the step, before the trainer builds its segments
                    from .frame_importance import ImportanceScorer
                    scorer = ImportanceScorer(trainer.program, sampler, importance)
        with open(frames_json, encoding="utf-8") as f:
            validate = validate and "validation" in json.load(f)["modes"]
        if validate or args.validate:
            validation_set = FrameSet.from_json(frames_json, "validation", log=quiet)
            if validation_set.tile != tile:
                raise ValueError("validation tiles of %d pixels, training tiles of %d" % (validation_set.tile, tile))
            validation_sampler = resident("validation", validation_set)

    eval_writers = {}

    preview = preview_settings(args, B)

    def report_validation(tag):
        tracked, shown = {}, ({} if (preview is not None and rank == 0) else None)
        if validation_sampler is not None:
            results = run_validation_frames(trainer, arch, tj, validation_sampler, B, rank, world, metrics_out=tracked, previews_out=shown, preview=preview)
        else:
            results = run_validation(trainer, arch, tj, base, B, rank, world, args.threads, metrics_out=tracked, previews_out=shown, preview=preview)
        for name, loss, n in results:
            if rank == 0:
                print("%s: %s loss %.5f over %d batches" % (tag, name, loss, n))
                for metric, value in tracked.get(name, []):
                    print("%s: %s %s %.6g" % (tag, name, metric, value))
                if name not in eval_writers:      # estimator.evaluate(name=name): one event file per run and validation set
                    eval_writers[name] = summaries.EventFileWriter(os.path.join(model_dir, "eval_" + name))
                eval_writers[name].add_scalars(step, [("loss", loss)] + tracked.get(name, []))
                if shown and name in shown:
                    eval_writers[name].add_images(step, shown[name])

    if args.validate:                                                     # Training.py:1230: a validation-only run
        report_validation("validation")
        for w in eval_writers.values():
            w.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    writer = summaries.EventFileWriter(model_dir) if (rank == 0 and (args.summary_steps > 0 or preview is not None)) else None
    trainer.program.write_histograms = bool(args.histograms)
    hist_plan = trainer.program.histogram_plan() if (args.histograms and args.summary_steps > 0) else []
    names = [e.name for e in trainer.program.metric_plan()] if args.summary_steps > 0 else []

    def pre_step_forward():
        prog = trainer.program
        prog.zero_grads()
        prog.forward()

    def tracked_scalars(forwarded=False):
        """The tracked metrics of the staged mini-batch at the current weights: a forward of its own BEFORE trainer.step() (the step is left
        as it is, and its backward may reuse prediction buffers; forwarded: the image summaries of this step have made it already).  Under
        data parallelism the per-image sums of all ranks are added, so rank 0 logs the global batch.  The same forward yields the
        histograms (--histograms): (scalars, histograms)."""
        if not names and not hist_plan:
            return [], None
        prog = trainer.program
        if not forwarded:
            pre_step_forward()
        records = prog.histogram_table() if hist_plan else None      # (launched now, read back behind the metric launches)
        scalars = _scalars(prog) if names else []
        return scalars, (tracked_histograms(prog, records) if hist_plan else None)

    def tracked_histograms(prog, records):
        """[(tag, HistogramProto fields)] of the forward just made.  Data parallelism: one SUM all-reduce over counts / num / nonfinite / sum /
        sum_squares (float64: a count is exact up to 2^53) and one MAX all-reduce over [max, -min]; every rank takes part, rank 0 writes."""
        from . import metrics as M
        table = prog.histogram_host_table(records)
        if world > 1:
            adds, ext = (torch.from_numpy(v).to(arch.device) for v in M.histogram_reduce_pack(table))
            dist.all_reduce(adds)
            dist.all_reduce(ext, op=dist.ReduceOp.MAX)
            table = M.histogram_reduce_unpack(adds.cpu().numpy(), ext.cpu().numpy(), *table["counts"].shape)
        tracked = prog.tracking_histograms
        return M.histogram_values(tracked.plan, table, tracked.limits, out=print if rank == 0 else (lambda *a: None))

    def _scalars(prog):
        table = prog.metric_table()
        if world == 1:
            return list(zip(names, prog.metric_values(table)))
        sums = prog.tracking_metrics.image_sums(table)
        dist.all_reduce(sums)
        return list(zip(names, prog.metric_values(sums.cpu().numpy(), count=world * B)))

    def refresh_importance():
        """Every rank: the tables of all ranks' steps since the last refresh, folded into the map the next draws come from (every rank takes
        the same number of steps, so the collective lines up, and every rank ends with the same bytes).  Rank 0 reports."""
        sums, counts = scorer.collect(dist)
        folded = importance.fold(sums, counts, args.frames_importance_rate)
        if rank != 0:
            return
        visited = counts > 0
        error = float((sums[visited].astype(np.float64) / 4294967296.0 / counts[visited]).mean()) if folded else 0.0
        share = folded / max(len(counts), 1)
        print("frames: importance refresh at step %d -- %d cells folded (%.1f %% of %d), mean model error %.4f, the heaviest tenth of the "
              "windows holds %.1f %% of the weight" % (step, folded, 100.0 * share, len(counts), error, 100.0 * importance.heaviest_tenth_share()))
        write_importance_pngs()
        if writer is not None:
            writer.add_scalars(step, [("frames_importance/folded_share", share), ("frames_importance/model_error", error)])

    gen = torch.Generator().manual_seed(1234 + rank)
    uploader = Uploader(arch.device) if sampler is None else None
    main_stream = torch.cuda.current_stream()

    def tfrecords_steps(stream):
        """Puts one mini-batch after the other into the program's input buffers; yields whether it was the epoch's last."""
        it = iter(stream)
        nxt = next(it, None)
        staged = uploader.stage(*nxt) if nxt is not None else None
        while staged is not None:
            feats, labels, done, keep = staged
            main_stream.wait_event(done)
            for v in list(feats.values()) + list(labels.values()):       # allocated on the copy stream, read on the launch stream
                v.record_stream(main_stream)
            feats, labels = DataAugmentation.apply(feats, labels, DataAugmentation.draw(B, gen), usage)
            trainer.program.set_inputs(feats, labels)
            nxt = next(it, None)                                         # the next mini-batch uploads while this step runs
            staged = uploader.stage(*nxt) if nxt is not None else None
            yield staged is None

    def frames_steps(rng, tuples):
        """The same from resident frames: B records and B draws, one upload of a few KB and one launch per mini-batch (frame_bank.py)."""
        sampler.reset()
        records = sampler.draw(rng, args.frames_crops, tuples, rank, world)
        while records is not None:
            sampler.sample(records, DataAugmentation.draw(B, gen))
            records = sampler.draw(rng, args.frames_crops, tuples, rank, world)
            yield records is None

    for epoch in range(args.train_epochs):
        rng = random.Random(args.seed * 1000003 + epoch)                 # shared by the ranks: same files, same shuffle, same index tuples
        tuples, _ = source_index_tuples(st["number_of_sources_per_example"], tj["number_of_source_index_tuples"], arch.number_of_sources_per_target,
                                        rng=rng)                         # redrawn every epoch (Training.py:1258)
        if sampler is None:
            stream = TileStream(os.path.join(base, "training"), "training", arch, B, tile, spp, tuples, rank, world, rng=rng, threads=args.threads)
            steps = tfrecords_steps(stream)
        else:
            stream = None
            steps = frames_steps(rng, tuples)
        total, count, t0, steps0 = 0.0, 0, time.time(), step
        for last in steps:
            summary = args.summary_steps > 0 and (step + 1) % args.summary_steps == 0
            # image summaries: rank 0 alone, launched on the pre-step forward (made here, shared with the tracked scalars), read back behind
            # the step like the histogram records
            show = preview is not None and rank == 0 and (step + 1) % args.image_steps == 0
            shown = None
            if show:
                pre_step_forward()
                shown = trainer.program.preview_table(**preview)
            scalars, histos = tracked_scalars(forwarded=show) if summary else (None, None)
            loss = trainer.step()
            step += 1
            if scorer is not None and step % args.frames_importance_refresh == 0:
                refresh_importance()
            if shown is not None:
                writer.add_images(step, preview_summaries(trainer.program, shown, preview))
            if summary:
                mean_loss = loss.double().sum()
                if dist is not None:
                    dist.all_reduce(mean_loss)
                scaler = trainer.program.sync_adam_step()                # (the loss is about to be read back: the wait is paid for anyway)
                if scaler is not None:
                    scalars = [("loss_scale", scaler["scale"]), ("skipped_steps", scaler["skipped_total"])] + scalars
                # clipping / --gradient_norms: the tables of this step's reduction (every rank holds the same bytes; rank 0 writes)
                norms = trainer.program.gradient_report() if writer is not None else None
                if norms is not None:
                    scalars = gradient_scalars(norms, per_variable=args.gradient_norms) + scalars
                if writer is not None:
                    head = [("loss", float(mean_loss) / world), ("learning_rate", tj["learning_rate"]), ("batch_size", tj["batch_size"])]
                    if histos:      # ONE event: the scalars up to batch_size, the histograms, the tracked scalars (Training.py:676-698)
                        writer.add_summaries(step, head, histos, scalars)
                    else:
                        writer.add_scalars(step, head + scalars)
            if step % 50 == 0 or last:
                total, count = total + float(loss), count + 1
        if dist is not None:
            dist.barrier()
        if rank == 0:
            dt = max(time.time() - t0, 1e-9)
            skipped = (trainer.program.sync_adam_step() or {}).get("skipped_total", 0)
            print("epoch %d: global_step %d, loss %.5f (%d steps, %.1f tiles/s, %d examples %s)%s" % (
                epoch + 1, step, total / max(count, 1), step - steps0, (step - steps0) * B * world / dt,
                stream.decoded if stream is not None else (step - steps0) * B * world,
                "decoded" if stream is not None else "cut from resident frames", ", %d steps skipped so far (loss scale)" % skipped if skipped else ""))
            tf_checkpoint.save_variables(arch, model_dir, global_step=step)
        if dist is not None:
            dist.barrier()                                               # nobody runs ahead of the checkpoint
        if validate and (epoch + 1) % args.validation_interval == 0:
            report_validation("epoch %d" % (epoch + 1))
    for w in [writer] + list(eval_writers.values()):
        if w is not None:
            w.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(parser().parse_args())
