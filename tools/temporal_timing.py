"""Device time of one TemporalStabilizer.stabilize (csrc/dd_temporal.hip: one stabilising and one finalize launch) for the passes of a
1920 x 1080 frame, next to the HBM copy rate of the same box.

    python tools/temporal_timing.py [--rgb 12] [--gray 3] [--guides 2] [--height 1080] [--width 1920] [--steps 3] [--warmup 2] [--out FILE]

15 passes as the Predictor hands them over: 12 RGB passes (dense [H,W,3]) and 3 one-channel passes as [..., :1] views of 3-wide frames; a dense
[H,W,3] motion pass with motions of up to 3 pixels and two 3-channel guides.  Time: HIP events around every stabilize() after the warm-up (the
guide copies it makes behind the launch included); the median is reported.  Bytes: per pass `current` and `history` read and `out` written
once (the used channels), the motion pass and both frames of every guide once per frame -- what the algorithm needs; the halo of a tile, the
second to fourth history tap and the unused channels of a 3-wide gray frame come on top and are served by the caches or paid for.  The copy
rate is measured in the same process (bench.hbm_copy_rate)."""
import argparse
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
    ap.add_argument("--rgb", type=int, default=12)
    ap.add_argument("--gray", type=int, default=3)
    ap.add_argument("--guides", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the result line to this file")
    args = ap.parse_args()

    import bench
    from deepdenoiser_amd.temporal import TemporalStabilizer
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    H, W = args.height, args.width
    gen = torch.Generator(device=device).manual_seed(3)

    # guides: blocks of 64 x 64 pixels on multiples of 0.5, the same in both frames: a pixel is rejected where it came from another block
    blocks = [torch.randint(0, 4, (H // 64 + 1, W // 64 + 1, 1), device=device, generator=gen).float().repeat_interleave(64, 0).repeat_interleave(64, 1)[:H, :W]
              .expand(H, W, 3).contiguous() * 0.5 for _ in range(args.guides)]

    def frame():
        predictions = {"rgb%d" % k: torch.randn((H, W, 3), device=device, generator=gen).abs() for k in range(args.rgb)}
        predictions.update({"gray%d" % k: torch.randn((H, W, 3), device=device, generator=gen).abs()[..., :1] for k in range(args.gray)})
        motion = torch.randint(-24, 25, (H, W, 3), device=device, generator=gen).float() / 8.0
        guides = {"guide%d" % k: blocks[k].clone() for k in range(args.guides)}
        return predictions, motion, guides
    frames = [frame() for _ in range(2)]
    stabilizer = TemporalStabilizer(device, guides=[("guide%d" % k, 0.25) for k in range(args.guides)])
    stabilizer.stabilize(*frames[0])                                             # the first frame passes through: it becomes the history
    times = []
    for step in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stabilizer.stabilize(*frames[(step + 1) % 2])
        e1.record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            times.append(e0.elapsed_time(e1))
    report = stabilizer.report()
    first = next(iter(report.values()))
    ms = statistics.median(times)
    nbytes = H * W * 4 * (3 * (3 * args.rgb + args.gray) + 3 + 2 * 3 * args.guides)
    copy_rate = bench.hbm_copy_rate(device)
    gbs = nbytes / (ms * 1e-3) / 1e9
    line = json.dumps({"metric": "TemporalStabilizer.stabilize: device ms per frame (all passes, one stabilising launch + finalize + guide copies)",
                       "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "steps": args.steps, "warmup": args.warmup,
                       "frame": [H, W], "rgb_passes": args.rgb, "gray_passes": args.gray, "guides": args.guides, "bytes": nbytes, "GB_per_s": gbs,
                       "hbm_copy_rate_GB_per_s": copy_rate, "ms_at_copy_rate": nbytes / copy_rate / 1e6, "time_over_copy_time": copy_rate / gbs,
                       "pixels_blended": first["pixels_blended"], "pixels": H * W})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
