"""Device time of one dd_tile_statistics launch (csrc/dd_frame_statistics.hip) over a resident bank, next to the HBM copy rate of the same box.

    python tools/frame_statistics_timing.py [--tile 128] [--scenes 10] [--sources 2] [--steps 20] [--warmup 3] [--out FILE]

The pass set of configs.cfg2_unet_kpcn() (Emission + seven auxiliary passes as sources, Emission as target) on synthetic 1920 x 1080 scenes
resident on the device (FrameBank.synthetic), the windows of deepdenoiser_amd.statistics.window_table (the grid of 128 x 128 tiles, one window
per source rendering and one per target), every 3-channel pass masked by the target Emission plane, so the masked sums are computed as well.
Time: HIP events around every launch after the warm-up; the median is reported.  Bytes: every sample of every (window, pass) the planes hold
once, plus the mask window once per (window, masked pass) -- what the kernel asks of memory; the mask windows of a tile repeat over the passes
and come from cache.  The copy rate is measured in the same process (bench.hbm_copy_rate)."""
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
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the result line to this file")
    args = ap.parse_args()

    import bench
    from deepdenoiser_amd import _lib as L
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.frame_bank import FrameBank
    from deepdenoiser_amd.statistics import window_table
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    arch = Architecture(configs.cfg2_unet_kpcn(), device=device, dtype="bf16", seed=2)
    T = args.tile
    bank = FrameBank.synthetic(arch, T, [(args.height, args.width)] * args.scenes, sources=args.sources, device=device, seed=3)
    mask_pass = next(name for name, ch in bank.target_channels.items() if ch == 3)
    names = sorted(bank.planes)
    windows, _ = window_table([(s.height, s.width) for s in bank.scenes], T, 1, args.sources)
    desc = L.StatDesc()
    desc.n_passes, desc.n_planes, desc.plane_hw = len(names), bank.n_planes, bank.plane_hw.data_ptr()
    nbytes = 0
    for en, name in zip(desc.pass_, names):
        ch = int(next(t for t in bank.planes[name] if t is not None).shape[-1])
        en.planes, en.C, en.is_alpha = bank.pointers[name].data_ptr(), ch, int(name == "Alpha")
        en.mask_planes = bank.pointers[mask_pass].data_ptr() if ch == 3 else None
        held = sum(1 for p in windows["plane"].tolist() if bank.planes[name][p] is not None)
        nbytes += held * T * T * 4 * (ch + (3 if ch == 3 else 0))
    table = torch.from_numpy(windows.view("uint8").copy()).to(device)
    rows = torch.empty((len(windows), len(names), L.STAT_FIELDS), dtype=torch.float64, device=device)
    lib = L.load()
    times = []
    for step in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.dd_tile_statistics(ctypes.byref(desc), table.data_ptr(), len(windows), T, rows.data_ptr(), torch.cuda.current_stream().cuda_stream))
        e1.record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            times.append(e0.elapsed_time(e1))
    ms = statistics.median(times)
    copy_rate = bench.hbm_copy_rate(device)
    gbs = nbytes / (ms * 1e-3) / 1e9
    line = json.dumps({"metric": "dd_tile_statistics: device ms per launch (every window and pass of the resident bank, one launch)",
                       "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "steps": args.steps, "warmup": args.warmup,
                       "tile": T, "windows": len(windows), "passes": len(names), "bytes": nbytes, "GB_per_s": gbs,
                       "hbm_copy_rate_GB_per_s": copy_rate, "ms_at_copy_rate": nbytes / copy_rate / 1e6, "time_over_copy_time": copy_rate / gbs,
                       "resident_GB": bank.total_bytes / 1e9, "scenes": args.scenes, "sources": args.sources, "frame": [args.height, args.width]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
