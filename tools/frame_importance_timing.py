"""Device time of one dd_importance_cells launch (csrc/dd_frame_importance.hip) over a resident bank, next to the HBM copy rate of the same box.

    python tools/frame_importance_timing.py [--tile 128] [--cell G] [--scenes 4] [--sources 2] [--steps 20] [--warmup 3] [--out FILE]

The pass set of configs.example_architecture() (all 16 colour passes are both a source and a target) on synthetic 1920 x 1080 scenes resident
on the device (FrameBank.synthetic), the cell table of deepdenoiser_amd.frame_importance.cell_table (every G x G cell of every scene, one
launch).  Time: HIP events around every launch after the warm-up; the median is reported.  Bytes: every sample of the colour passes in the
cells, source and target planes, once -- what the kernel asks of memory (the cell table and the doubles it writes are 24 bytes per cell).  The
copy rate is measured in the same process (bench.hbm_copy_rate)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--cell", type=int, default=None)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the result line to this file")
    args = ap.parse_args()

    import bench
    import numpy as np
    from deepdenoiser_amd import _lib as L
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.frame_bank import FrameBank
    from deepdenoiser_amd.frame_importance import EPSILON, cell_table, colour_passes, resolve_cell
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    arch = Architecture(configs.example_architecture(), device=device, dtype="bf16", seed=2)
    bank = FrameBank.synthetic(arch, args.tile, [(args.height, args.width)] * args.scenes, sources=args.sources, device=device, seed=3)
    names, G = colour_passes(bank), resolve_cell(args.tile, args.cell)
    table = cell_table(bank, G)
    desc = L.ImportanceDesc()
    desc.n_passes, desc.n_planes, desc.plane_hw, desc.n_sources, desc.epsilon = len(names), bank.n_planes, bank.plane_hw.data_ptr(), bank.S, EPSILON
    for en, name in zip(desc.pass_, names):
        en.planes = bank.pointers[name].data_ptr()
    nbytes = len(table) * G * G * 3 * 4 * len(names) * (args.sources + 1)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(device)
    out = torch.empty(len(table), dtype=torch.float64, device=device)
    lib = L.load()
    times = []
    for step in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.dd_importance_cells(ctypes.byref(desc), table_dev.data_ptr(), len(table), G, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        e1.record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    copy_rate = bench.hbm_copy_rate(device)
    gbs = nbytes / (ms * 1e-3) / 1e9
    mean = float(out.sum().item()) / (len(table) * G * G * 3 * len(names) * args.sources)
    line = json.dumps({"metric": "dd_importance_cells: device ms per launch (every cell of the resident bank, one launch)",
                       "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "steps": args.steps, "warmup": args.warmup,
                       "tile": args.tile, "cell": G, "cells": len(table), "passes": len(names), "bytes": nbytes, "GB_per_s": gbs,
                       "hbm_copy_rate_GB_per_s": copy_rate, "ms_at_copy_rate": nbytes / copy_rate / 1e6, "time_over_copy_time": copy_rate / gbs,
                       "resident_GB": bank.total_bytes / 1e9, "scenes": args.scenes, "sources": args.sources, "frame": [args.height, args.width],
                       "mean_smape": mean})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
