"""Time per predict_frame() over a 1920 x 1080 frame sequence of the bench's inference configuration (cfg-2, fp16, tiles of 128 with overlap 14)
with and without the NaN / Inf scan and repair -- the A/B behind DESIGN.md section 3.19.  Wall time over `--frames` frames after `--warmup`, like
bench.py's inference mode, `--runs` times; the frames are bench.py's (device-resident, three buffer sets).  `--nonfinite keep` passes no
keyword this tool's commit added, so it also runs from a checkout of an older commit (run it with that checkout as the working directory).

    python tools/nonfinite_ab.py --nonfinite keep
    python tools/nonfinite_ab.py --nonfinite repair                       # clean frames: the scan, and a repair launch that returns at once
    python tools/nonfinite_ab.py --nonfinite repair --planted 1e-4        # 0.01 % of the pixels of every pass hold a NaN
    python tools/nonfinite_ab.py --nonfinite repair --parts               # also: device time of the copy, the scan and the repair on their own
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.getcwd())

from deepdenoiser_amd import configs                               # noqa: E402
from deepdenoiser_amd.architecture import Architecture             # noqa: E402
from deepdenoiser_amd.naming import Naming                         # noqa: E402
from deepdenoiser_amd.prediction import Predictor                  # noqa: E402

H, W = 1080, 1920


def event_ms(fn, reps):
    """device time of fn() per call: events around `reps` calls on the current stream"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def parts(frame, keys, channels, reps=20):
    """The copy of the pass tensors, the scan and the repair (on clean and on the given planes) on their own, in device milliseconds."""
    from deepdenoiser_amd.nonfinite import Scanner
    scanner = Scanner("cuda:0", [(k, tuple(frame[k].shape), channels[k]) for k in keys])
    work = {k: frame[k].clone() for k in keys}
    out = {"pass_bytes": sum(v.numel() * 4 for v in work.values()), "mask_bytes": len(keys) * H * W,
           "copy_ms": event_ms(lambda: [frame[k].clone() for k in keys], reps),
           "scan_ms": event_ms(lambda: scanner.scan(work), reps)}

    def scan_and_repair():
        for k in keys:
            work[k].copy_(frame[k])
        scanner.scan(work)
        scanner.repair(work, radius=2)
    out["copy_scan_repair_ms"] = event_ms(scan_and_repair, reps)
    for k in keys:
        work[k].copy_(frame[k])
    scanner.scan(work)
    out["repair_ms"] = event_ms(lambda: scanner.repair(work, radius=2), reps)      # (the masks of ONE scan: every call does the same work)
    out["report"] = {"values": sum(v["values"] for v in scanner.report().values()), "pixels": sum(v["pixels"] for v in scanner.report().values())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nonfinite", default="keep", choices=["keep", "repair"])
    ap.add_argument("--planted", type=float, default=0.0, help="fraction of the pixels of every pass that hold a NaN")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parts", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cuda:0", dtype=args.dtype, seed=2)
    kw = {"nonfinite": "repair"} if args.nonfinite == "repair" else {}
    pred = Predictor(arch, tile_size=128, tile_overlap_size=14, tiles_per_batch=256, **kw)
    g = torch.Generator().manual_seed(7)
    feats = arch.feature_predictions + arch.auxiliary_features
    frames = [{Naming.source_feature_name(f.name, index=0): torch.randn(H, W, f.number_of_channels, generator=g).abs().to("cuda:0") for f in feats}
              for _ in range(3)]
    if args.planted > 0.0:
        n = max(1, int(round(args.planted * H * W)))
        for fr in frames:
            for v in fr.values():
                idx = torch.randint(0, H * W, (n,), generator=g).to("cuda:0")
                v.view(H * W, -1)[idx, 0] = float("nan")
    for i in range(max(2, args.warmup)):
        pred.predict_frame(frames[i % len(frames)])
    ms = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.frames):
            out = pred.predict_frame(frames[i % len(frames)])
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.frames)
    res = {"label": args.label, "nonfinite": args.nonfinite, "planted": args.planted, "dtype": args.dtype, "ms_per_frame": [round(x, 4) for x in ms],
           "median_ms": round(sorted(ms)[len(ms) // 2], 4), "frames": args.frames,
           "output_finite": bool(all(torch.isfinite(v).all() for v in out.values()))}
    if args.nonfinite == "repair":
        rep = pred.nonfinite_report()
        res["report"] = {"values": sum(v["values"] for v in rep.values()), "pixels": sum(v["pixels"] for v in rep.values()), "passes": len(rep)}
    if args.parts:
        keys = list(dict.fromkeys(Naming.source_feature_name(f.name, index=0) for f in feats))
        channels = {Naming.source_feature_name(f.name, index=0): f.number_of_channels for f in feats}
        res["parts"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in parts(frames[0], keys, channels).items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
