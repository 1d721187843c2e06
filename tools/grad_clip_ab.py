"""Time per Trainer.step() of the bench workload (cfg-2 U-Net KPCN, 128 tile-passes of 128 x 128, hipGraph, bf16 storage) without and with
gradient clipping by global norm -- the A/B behind DESIGN.md 3.22.  Both models live in ONE process and take turns, `--runs` times each:
wall time over `--steps` steps after `--warmup`, like bench.py, with bench.py's inputs.  The clipped model clips at a tenth of its first
step's norm (the launches and their cost are the same whatever the coefficient turns out to be); `--variants off,track,on` adds a model that only measures the norms (coef = 1).  `--variants off`
needs nothing this tool's commit added, so it also runs from a checkout of an older commit (with that checkout as the working directory):
how the parent commit is timed in the same call.  One JSON line per variant.

    python tools/grad_clip_ab.py --steps 60 --runs 4
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())

from bench import synthetic_inputs                                 # noqa: E402
from deepdenoiser_amd import configs                               # noqa: E402
from deepdenoiser_amd.architecture import Architecture             # noqa: E402
from deepdenoiser_amd.training import Trainer                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="off,on", help="comma-separated: off, track, on")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    variants = args.variants.split(",")
    assert variants and all(v in ("off", "track", "on") for v in variants), variants

    def trainer_for(**kw):
        arch = Architecture(configs.cfg2_unet_kpcn(), device="cuda:0", dtype=args.dtype, seed=2, **kw)
        trainer = Trainer(arch, configs.bench_training(), args.batch, args.tile, args.tile)
        trainer.program.set_inputs(*synthetic_inputs(arch, args.batch, args.tile, args.tile, "cuda:0", seed=1000))
        return trainer

    trainers = {}
    for v in variants:
        if v == "off":
            trainers[v] = trainer_for()
        elif v == "track":
            trainers[v] = trainer_for(track_gradient_norms=True)
        else:      # a first step of a tracking model gives the norm to clip against
            probe = trainer_for(track_gradient_norms=True)
            probe.step()
            norm0 = probe.program.gradient_report()["grad_norm"]
            del probe
            trainers[v] = trainer_for(clip_norm=0.1 * norm0)
    for t in trainers.values():
        for _ in range(args.warmup):
            t.step()
    ms = {v: [] for v in variants}
    for _ in range(args.runs):
        for v in variants:      # the variants take turns: a drift of the box's clocks meets all of them
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                trainers[v].step()
            torch.cuda.synchronize()
            ms[v].append(1e3 * (time.perf_counter() - t0) / args.steps)
    for v in variants:
        trainer, arch = trainers[v], trainers[v].arch
        out = {"label": args.label, "clip": v, "dtype": args.dtype, "ms_per_step": [round(x, 4) for x in ms[v]],
               "median_ms": round(sorted(ms[v])[len(ms[v]) // 2], 4), "steps": args.steps, "arena_bytes": int(arch.params.grads.numel() * 4),
               "variables": len(arch.params.params), "loss": float(trainer.program.loss_buf)}
        if v != "off":
            prog = trainer.program
            rep = prog.gradient_report()
            out.update(clip_norm=arch.clip_norm, grad_norm=rep["grad_norm"], coef=rep["coef"], chunks=prog.clipper.n_chunks)
            # the two reduction launches alone: HIP events around 50 repeats on the otherwise idle stream
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(50):
                prog.clipper.measure(1.0, prog.g.stream_ptr())
            b.record()
            torch.cuda.synchronize()
            out["reduction_us"] = round(1e3 * a.elapsed_time(b) / 50, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
