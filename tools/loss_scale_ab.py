"""Time per Trainer.step() of the bench workload (cfg-2 U-Net KPCN, 128 tile-passes of 128 x 128, hipGraph) in fp16 storage with a static or a
dynamic loss scale -- the A/B behind DESIGN.md's loss-scale section.  Wall time over `--steps` steps after `--warmup`, like bench.py, `--runs`
times; the inputs are bench.py's.  `--loss_scale static` needs nothing this tool's commit added, so it also runs from a checkout of an older
commit (run it with that checkout as the working directory).

    python tools/loss_scale_ab.py --loss_scale static  --steps 60 --runs 3
    python tools/loss_scale_ab.py --loss_scale dynamic --steps 60 --runs 3
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
    ap.add_argument("--loss_scale", default="static", choices=["static", "dynamic"])
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    kw = {"loss_scale": "dynamic"} if args.loss_scale == "dynamic" else {}
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cuda:0", dtype=args.dtype, seed=2, **kw)
    trainer = Trainer(arch, configs.bench_training(), args.batch, args.tile, args.tile)
    trainer.program.set_inputs(*synthetic_inputs(arch, args.batch, args.tile, args.tile, "cuda:0", seed=1000))
    for _ in range(args.warmup):
        trainer.step()
    ms = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            trainer.step()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {"label": args.label, "loss_scale": args.loss_scale, "dtype": args.dtype, "ms_per_step": [round(x, 4) for x in ms],
           "median_ms": round(sorted(ms)[len(ms) // 2], 4), "steps": args.steps, "arena_bytes": int(arch.params.grads.numel() * 4),
           "loss": float(trainer.program.loss_buf)}
    scaler = getattr(trainer.program, "scaler", None)
    if scaler is not None:
        out["scaler"] = scaler.state()
    else:
        out["skipped_steps"] = getattr(trainer.program, "skipped_steps", 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
