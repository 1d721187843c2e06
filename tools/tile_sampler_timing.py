"""Device time of one TileSampler.sample() (csrc/dd_tile_sampler.hip) at the benchmark's shape, next to the HBM copy rate of the same box.

    python tools/tile_sampler_timing.py [--batch 128] [--tile 128] [--scenes 10] [--steps 30] [--warmup 5] [--out FILE]

The pass set of configs.cfg2_unet_kpcn() (Emission + seven auxiliary passes as sources, Emission as target), 128 x 128 tiles, the batch
bench.py's augment_bench uses, ten synthetic 1920 x 1080 scenes resident on the device, random crops, the augmentation switches of the
example Training.json (rotate, RGB permutation, normal rotation; no flip).  Time: HIP events around every sample() -- the upload of the record
table and the one launch -- after the warm-up; the median is reported.  Bytes: 2 x 4 x elements (every element read once and written once).
The parent's path for the same batch is `python bench.py --mode augment` (one dd_augment launch per pass on tiles that are already cut and
uploaded): run it in the same session and set the two lines side by side."""
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
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="", help="also append the result line to this file")
    args = ap.parse_args()

    import bench
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.data_augmentation import DataAugmentation, DataAugmentationUsage
    from deepdenoiser_amd.frame_bank import FrameBank, TileSampler
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    arch = Architecture(configs.cfg2_unet_kpcn(), device=device, dtype="bf16", seed=2)
    B, T = args.batch, args.tile
    prog = arch.program(B, T, T, training_json=configs.bench_training())
    bank = FrameBank.synthetic(arch, T, [(args.height, args.width)] * args.scenes, sources=1, device=device, seed=3)
    usage = DataAugmentationUsage(True, False, True, True)              # TrainingExample.json:17-23
    sampler = TileSampler(prog, bank, usage)
    rng, gen = random.Random(0), torch.Generator().manual_seed(1)
    tuples = [[0]]
    times = []
    for step in range(args.warmup + args.steps):
        records = sampler.draw(rng, "random", tuples)
        if records is None:
            records = sampler.draw(rng, "random", tuples)
        draws = DataAugmentation.draw(B, gen)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sampler.sample(records, draws)
        e1.record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            times.append(e0.elapsed_time(e1))
    elements = sum(B * T * T * en.C for en in sampler.desc.pass_[:sampler.desc.n_passes])
    nbytes = 2 * 4 * elements
    ms = statistics.median(times)
    copy_rate = bench.hbm_copy_rate(device)                              # the figure `bench.py --full` reports as the practical HBM ceiling
    gbs = nbytes / (ms * 1e-3) / 1e9
    line = json.dumps({"metric": "dd_sample_tiles: device ms per sample() (crop + augmentation of every pass, one launch)",
                       "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "steps": args.steps, "warmup": args.warmup,
                       "batch": B, "tile": T, "passes": sampler.desc.n_passes, "channels": elements // (B * T * T), "bytes": nbytes, "GB_per_s": gbs,
                       "hbm_copy_rate_GB_per_s": copy_rate, "frac_of_copy_rate": gbs / copy_rate,
                       "resident_GB": bank.total_bytes / 1e9, "scenes": args.scenes, "frame": [args.height, args.width]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
