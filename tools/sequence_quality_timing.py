"""Device time of one SequenceQuality.measure (csrc/dd_sequence_quality.hip: one scoring and one finalize launch, then the copies of the frame
into the previous-frame buffers and of the records to the host) for the passes of a 1920 x 1080 frame, next to the HBM copy rate of the same box.

    python tools/sequence_quality_timing.py [--rgb 12] [--gray 3] [--height 1080] [--width 1920] [--steps 3] [--warmup 2] [--out FILE]

15 passes as predict hands them over: 12 RGB passes (dense [H,W,3]) and 3 one-channel passes as [..., :1] views of 3-wide frames, each with a
target of the same form; a dense [H,W,3] motion pass with per-pixel random motions of up to 3 pixels (the least coherent tap pattern).  Time:
HIP events around every measure() after the warm-up; the median is reported, and next to it the median of the two launches alone (the same
frames, without the copies).  Bytes: per pair `pred`, `target`, `pred_previous` and `target_previous` read once (the used channels: 48 per
pixel of an RGB pair, 16 of a one-channel pair) and 8 bytes of motion per pixel and frame -- what the algorithm needs; the second to fourth
tap of the previous frames and the unused channels of a 3-wide gray frame come on top and are served by the caches or paid for; the copies of
measure() are not algorithmic bytes of the launch and are not counted.  The copy rate is measured in the same process (bench.hbm_copy_rate).
Nothing is gated: this is a record."""
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
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the result line to this file")
    args = ap.parse_args()

    import bench
    from deepdenoiser_amd.sequence_quality import SequenceQuality
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    H, W = args.height, args.width
    gen = torch.Generator(device=device).manual_seed(3)

    def images():
        out = {"rgb%d" % k: torch.randn((H, W, 3), device=device, generator=gen).abs() for k in range(args.rgb)}
        out.update({"gray%d" % k: torch.randn((H, W, 3), device=device, generator=gen).abs()[..., :1] for k in range(args.gray)})
        return out

    def frame():
        return images(), images(), torch.randint(-24, 25, (H, W, 3), device=device, generator=gen).float() / 8.0
    frames = [frame() for _ in range(2)]
    scorer = SequenceQuality(device)
    assert scorer.measure(*frames[0]) is None                                    # the first frame becomes the history

    def timed(call):
        times = []
        for step in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            result = call(*frames[(step + 1) % 2])
            e1.record()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times.append(e0.elapsed_time(e1))
        return times, result
    times, report = timed(scorer.measure)
    launch_times, _ = timed(lambda predictions, targets, motion: scorer._launch(list(predictions), predictions, targets, motion))
    first = next(iter(report.values()))
    ms, launch_ms = statistics.median(times), statistics.median(launch_times)
    nbytes = H * W * 4 * (4 * (3 * args.rgb + args.gray) + 2)
    copy_rate = bench.hbm_copy_rate(device)
    line = json.dumps({"metric": "SequenceQuality.measure: device ms per frame (all pairs: one scoring launch + finalize, then the history and record copies)",
                       "ms_median": ms, "ms_min": min(times), "ms_max": max(times), "launches_only_ms_median": launch_ms, "launches_only_ms_min": min(launch_times),
                       "launches_only_ms_max": max(launch_times), "steps": args.steps, "warmup": args.warmup, "frame": [H, W], "rgb_pairs": args.rgb,
                       "gray_pairs": args.gray, "bytes": nbytes, "GB_per_s": nbytes / (ms * 1e-3) / 1e9, "launches_only_GB_per_s": nbytes / (launch_ms * 1e-3) / 1e9,
                       "hbm_copy_rate_GB_per_s": copy_rate, "ms_at_copy_rate": nbytes / copy_rate / 1e6, "time_over_copy_time": ms * 1e-3 * copy_rate * 1e9 / nbytes,
                       "launches_only_time_over_copy_time": launch_ms * 1e-3 * copy_rate * 1e9 / nbytes, "pixels_valid": first["pixels_valid"], "pixels": H * W,
                       "note": "measured once, not gated"})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
