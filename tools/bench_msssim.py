"""What the MS-SSIM loss term costs per training step (bench.py is not changed; the measurement behind DESIGN 3.14).

    python tools/bench_msssim.py [--steps 30] [--warmup 8] [--rounds 3] [--out FILE.json]      # step times, variants alternated
    python tools/bench_msssim.py --profile ex_all [--no-graph]                                 # a few steps of ONE variant, for rocprofv3

Variants (bf16 storage, 128 tile passes of 128 x 128 per step, captured hipGraph, as bench.py runs cfg-2):
  cfg2_off / cfg2_features      bench.py's own configuration (cfg-2 is one SINGLE tuple: the features level is the only one that exists),
                                ms_ssim 0 (no launch is added) against a features-level weight;
  ex_off / ex_image / ex_all    the 17-tuple example network without its 1-channel Alpha pass (16 passes x 8 tiles = 128 tile passes):
                                ms_ssim 0, on the combined image only, on all three levels (16 features + 4 combined features + the image).
The variants of a group are timed alternately, `rounds` times each; the spread of the rounds is printed next to the median."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deepdenoiser_amd import configs  # noqa: E402
from deepdenoiser_amd.naming import Naming  # noqa: E402


def variants():
    no_alpha = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
    cfg2, ex = configs.cfg2_unet_kpcn, lambda: configs.architecture(flag_mode="NONE", combined=no_alpha)
    bench = dict(combined_mean=0.0, image_mean=0.0)
    return {
        "cfg2_off": (cfg2, dict(bench), 128),
        "cfg2_features": (cfg2, dict(bench, ms_ssim=(0.6, 0.0, 0.0)), 128),
        "ex_off": (ex, {}, 8),
        "ex_image": (ex, dict(ms_ssim=(0.0, 0.0, 4.0)), 8),
        "ex_all": (ex, dict(ms_ssim=(0.6, 2.0, 4.0)), 8),
    }


def make(name, tile, use_graph=True):
    from bench import synthetic_inputs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.training import Trainer
    make_aj, knobs, B = variants()[name]
    arch = Architecture(make_aj(), device="cuda", dtype="bf16", seed=2)
    trainer = Trainer(arch, configs.training(**knobs), B, tile, tile, world_size=1, use_graph=use_graph)
    feats, labels = synthetic_inputs(arch, B, tile, tile, "cuda", seed=1000)
    for f in arch.feature_predictions:      # labels that correlate with the sources (the time of the launches does not depend on the values)
        labels[Naming.target_feature_name(f.name)] = feats[Naming.source_feature_name(f.name, index=0)].clone()
    trainer.program.set_inputs(feats, labels)
    return trainer


def timed(trainer, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def algorithmic_bytes(trainer):
    """both tensors of every source read once per pass, dpred read and written once (fp32)"""
    prog = trainer.program
    m, _ = prog.ms_ssim_desc
    plane = prog.B * prog.H * prog.W * 3 * 4
    n_feat = sum(m.ssim_weight[i] > 0 for i in range(m.n_features))
    n_comb = sum(m.comb_ssim_weight[k] > 0 for k in range(m.n_combined))
    n_img = m.n_image_combined * 3 + m.n_image_features if m.image_ssim_weight > 0 else 0
    parts = n_feat + 3 * n_comb + n_img                      # feature planes one pass over the sources reads (pred and target each)
    return {"sources": n_feat + n_comb + (1 if n_img else 0), "plane_bytes": plane, "forward_level0_read": 2 * parts * plane,
            "backward_level0_read": 3 * parts * plane, "backward_level0_write": parts * plane}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--groups", default="cfg2,ex")
    ap.add_argument("--profile", default="")
    ap.add_argument("--no-graph", action="store_true", help="with --profile: plain launches (counter passes)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run says nothing about step time"
    if args.profile:
        trainer = make(args.profile, args.tile, use_graph=not args.no_graph)
        if hasattr(trainer.program, "ms_ssim_desc"):
            print(json.dumps({"variant": args.profile, "algorithmic_bytes": algorithmic_bytes(trainer)}))
        for _ in range(args.warmup):
            trainer.step()
        print("step %.3f ms" % timed(trainer, args.steps))
        return
    result = {"device": torch.cuda.get_device_name(0), "tile": args.tile, "steps": args.steps, "rounds": args.rounds, "step_ms": {}}
    for group in args.groups.split(","):
        names = [n for n in variants() if n.startswith(group + "_")]
        trainers = {n: make(n, args.tile) for n in names}
        for n in names:
            for _ in range(args.warmup):
                trainers[n].step()
        times = {n: [] for n in names}
        for _ in range(args.rounds):
            for n in names:
                times[n].append(timed(trainers[n], args.steps))
        for n in names:
            t = sorted(times[n])
            result["step_ms"][n] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "loss": float(trainers[n].program.loss_buf)}
            print("%-14s step %.3f ms (min %.3f max %.3f)  added %.3f ms" % (n, t[len(t) // 2], t[0], t[-1],
                                                                          t[len(t) // 2] - result["step_ms"][names[0]]["median"]), flush=True)
        del trainers
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
