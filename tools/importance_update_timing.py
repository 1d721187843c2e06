"""Device time of one dd_importance_update launch (csrc/dd_importance_update.hip) at the bench's cfg-2 shape, next to the HBM copy rate of the
same box, and the training step with and without the launch.

    python tools/importance_update_timing.py [--batch 128] [--tile 128] [--cell 16] [--steps 20] [--warmup 3] [--rounds 5] [--block 10] [--out FILE]

The launch: the cfg-2 program (configs.cfg2_unet_kpcn, bench_training) on a synthetic resident bank (FrameBank.synthetic), a mini-batch cut
by the sampler at origins that are multiples of the cell -- every pixel of every tile lies in a whole cell, so the launch reads every
prediction and target sample of the colour passes once -- forwarded once, then scored `steps` times: HIP events around every launch after the
warm-up, the median is reported, once with every example drawn with rotate 0 and once with rotate 1 (a frame row of a cell is then a tile
column).  Bytes: B T T (pred 12 + target 12) per pass, what the kernel asks of memory.  The copy rate is measured in the same process
(bench.hbm_copy_rate); ms_at_copy_rate is what a plain copy of as many bytes takes at it.

The step: two trainers of the same architecture and seed in one process, one with an ImportanceScorer attached, both fed by their own
sampler with the same records (random origins; rotate, RGB permutation and normal rotation on, no flip); `rounds` alternations of `block` Trainer.step() calls
each (captured hipGraphs), HIP events around every block."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--out", default="", help="also append the result lines to this file")
    args = ap.parse_args()

    import bench
    import numpy as np
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.data_augmentation import DataAugmentation, DataAugmentationUsage
    from deepdenoiser_amd.frame_bank import FrameBank, TileSampler
    from deepdenoiser_amd.frame_importance import ImportanceMap, ImportanceScorer
    from deepdenoiser_amd.training import Trainer
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    B, T, G = args.batch, args.tile, args.cell
    tj = configs.bench_training()
    usage = DataAugmentationUsage(True, False, True, True)     # TrainingExample.json:17-23 (rotate, RGB permutation, normal rotation; no flip)
    lines = []

    def make(scored):
        arch = Architecture(configs.cfg2_unet_kpcn(), device=device, dtype=args.dtype, seed=2)
        trainer = Trainer(arch, tj, B, T, T, world_size=1, use_graph=True)
        bank = FrameBank.synthetic(arch, T, [(args.height, args.width)] * args.scenes, sources=1, device=device, seed=3)
        sampler = TileSampler(trainer.program, bank, usage)
        scorer = None
        if scored:
            imap = ImportanceMap(bank, cell=G)
            sampler.set_importance(imap)
            scorer = ImportanceScorer(trainer.program, sampler, imap)
        return trainer, sampler, scorer

    plain, plain_sampler, _ = make(False)
    scored, sampler, scorer = make(True)
    rng = random.Random(5)
    gen = torch.Generator().manual_seed(7)
    n_scenes = len(sampler.bank.scenes)

    def records(aligned):
        out = np.empty((B, 4), dtype=np.int32)
        for b in range(B):
            s = rng.randrange(n_scenes)
            y0, x0 = rng.randint(0, args.height - T), rng.randint(0, args.width - T)
            if aligned:
                y0, x0 = y0 // G * G, x0 // G * G
            out[b] = (sampler.bank.source_plane(s, 0), sampler.bank.target_plane(s), y0, x0)
        return out

    # ---- the launch alone
    copy_rate = bench.hbm_copy_rate(device)
    n_passes = len(scorer.passes)
    nbytes = B * T * T * n_passes * (12 + 12)
    stream = torch.cuda.current_stream().cuda_stream
    for rotate in (0, 1):
        draws = DataAugmentation.draw(B, gen)
        draws["rotate"] = np.full(B, rotate, dtype=np.int32)
        sampler.sample(records(aligned=True), draws)
        scored.program.zero_grads()
        scored.program.forward()
        times = []
        for step in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scorer.op(stream)
            e1.record()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times.append(e0.elapsed_time(e1))
        sums, counts = scorer.collect()
        assert int(counts.sum()) == (args.warmup + args.steps) * B * (T // G) ** 2
        ms = statistics.median(times)
        gbs = nbytes / (ms * 1e-3) / 1e9
        lines.append({"metric": "dd_importance_update: device ms per launch (one mini-batch, every cell whole)", "rotate": rotate,
                      "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "steps": args.steps, "warmup": args.warmup, "batch": B, "tile": T,
                      "cell": G, "passes": n_passes, "pred_ld": int(scored.program.predictions[0].ld), "bytes": nbytes, "GB_per_s": gbs,
                      "hbm_copy_rate_GB_per_s": copy_rate, "ms_at_copy_rate": nbytes / copy_rate / 1e6, "time_over_copy_time": copy_rate / gbs,
                      "mean_model_error": float((sums / 4294967296.0 / np.maximum(counts, 1)).mean()), "dtype": args.dtype})

    # ---- the step with and without it
    recs, draws = records(aligned=False), DataAugmentation.draw(B, gen)
    for s in (plain_sampler, sampler):
        s.sample(recs, draws)
    for tr in (plain, scored):
        for _ in range(args.warmup + 3):                       # (the capture happens at the third step)
            tr.step()
    torch.cuda.synchronize()
    per_step = {"plain": [], "scored": []}
    for _ in range(args.rounds):
        for name, tr in (("plain", plain), ("scored", scored)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.block):
                tr.step()
            e1.record()
            torch.cuda.synchronize()
            per_step[name].append(e0.elapsed_time(e1) / args.block)
    a, b = statistics.median(per_step["plain"]), statistics.median(per_step["scored"])
    lines.append({"metric": "Trainer.step(): device ms per step without / with the scoring launch (alternating blocks, one process)",
                  "plain_ms_median": a, "scored_ms_median": b, "difference_ms": b - a, "difference_percent": 100.0 * (b - a) / a,
                  "plain_ms": per_step["plain"], "scored_ms": per_step["scored"],
                  "plain_spread_percent": 100.0 * (max(per_step["plain"]) - min(per_step["plain"])) / a,
                  "scored_spread_percent": 100.0 * (max(per_step["scored"]) - min(per_step["scored"])) / b,
                  "rounds": args.rounds, "block": args.block, "batch": B, "tile": T, "cell": G, "dtype": args.dtype,
                  "tail_ops": len(scored.program.step_tail_ops), "plain_tail_ops": len(plain.program.step_tail_ops)})
    for line in lines:
        print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
