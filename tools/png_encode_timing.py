"""Wall time of writing a denoised frame's passes as 8-bit sRGB PNG files, encoded on the host (png.encode_host: numpy quantisation and filters,
zlib level 6) or on the device (png.DevicePngEncoder: csrc/dd_png_encode.hip), in one process.

    python tools/png_encode_timing.py [--rgb 12] [--gray 3] [--runs 3] [--height 1080] [--width 1920] [--out profiles/png_encode.txt]

The predictions are synthetic: `--rgb` three-channel and `--gray` one-channel fp32 planes on the device, a seeded smooth image plus mild noise,
like a denoised frame.  Timed, `--runs` times per mode after one warm-up run, the two modes alternating, the median reported:
openexr.save_predictions(png=True) with png_encode="host" and with png_encode="device" (the .npy files are written by both, as predict.py
does).  For the device mode further DevicePngEncoder.encode calls of the same planes, events around the launches, give the device time of
the pack launch and of the deflate launch, the deflate launch's GB/s in (the filtered bytes it reads) and out (the bytes it keeps), the
segments that came back RAW, and the host's share of that call (assembling and writing the files)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rgb", type=int, default=12)
    ap.add_argument("--gray", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--modes", default="host,device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.txt"), help="the result lines are appended to this file")
    args = ap.parse_args()

    from deepdenoiser_amd import openexr, png
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:args.height, 0:args.width].astype(np.float32)
    predictions = {}
    for k in range(args.rgb + args.gray):
        n = 3 if k < args.rgb else 1
        img = np.stack([0.05 + (k + 1) * 4e-5 * y + (c + 1) * 1.5e-4 * x for c in range(n)], axis=-1).astype(np.float32)
        img += 0.004 * rng.standard_normal(img.shape).astype(np.float32)
        predictions["prediction/Pass %02d" % k] = torch.from_numpy(img).to(device)
    samples = args.height * args.width * (3 * args.rgb + args.gray)
    modes = args.modes.split(",")
    lines = []
    with tempfile.TemporaryDirectory() as root:
        seconds, file_bytes = {m: [] for m in modes}, {m: 0 for m in modes}
        for run in range(args.runs + 1):                               # (the first run warms the allocator, the pinned buffers and the page cache)
            for mode in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = openexr.save_predictions(root, predictions, png=True, png_encode=mode)
                torch.cuda.synchronize()
                if run > 0:
                    seconds[mode].append(time.perf_counter() - t0)
                file_bytes[mode] = sum(os.path.getsize(p) for p in written if p.endswith(".png"))
        for mode in modes:
            s = seconds[mode]
            result = {"metric": "save_predictions(png=True): wall seconds (median of %d)" % args.runs, "png_encode": mode, "seconds_median": statistics.median(s),
                      "seconds_min": min(s), "seconds_max": max(s), "passes": [args.rgb, args.gray], "frame": [args.height, args.width],
                      "plane_GB": samples * 4 / 1e9, "png_file_GB": file_bytes[mode] / 1e9}
            if mode == "device":
                png.DevicePngEncoder.time_launches = True
                requests = [(os.path.join(root, "timed_%02d.png" % k), v, 1.0) for k, v in enumerate(predictions.values())]
                pack_ms, deflate_ms, wall, host = [], [], [], []
                encoder = png.DevicePngEncoder(device, threads=16)
                for run in range(args.runs + 1):
                    encoder.pack_events, encoder.deflate_events, encoder.host_seconds, encoder.raw_segments, encoder.segments = [], [], 0.0, 0, 0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    encoder.encode(requests)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if run > 0:
                        wall.append(dt)
                        host.append(encoder.host_seconds / dt)
                        pack_ms.append(sum(a.elapsed_time(b) for a, b in encoder.pack_events))
                        deflate_ms.append(sum(a.elapsed_time(b) for a, b in encoder.deflate_events))
                staged, kept, raw, segments = encoder.staged_bytes, encoder.body_bytes, encoder.raw_segments, encoder.segments
                encoder.release()
                png.DevicePngEncoder.time_launches = False
                ms = statistics.median(deflate_ms)
                result.update({"encode_call_seconds_median": statistics.median(wall), "pack_ms": statistics.median(pack_ms), "pack_ms_min": min(pack_ms),
                               "pack_ms_max": max(pack_ms), "deflate_ms": ms, "deflate_ms_min": min(deflate_ms), "deflate_ms_max": max(deflate_ms),
                               "deflate_in_GB": staged / 1e9, "deflate_out_GB": kept / 1e9, "deflate_in_GB_per_s": staged / (ms * 1e-3) / 1e9,
                               "deflate_out_GB_per_s": kept / (ms * 1e-3) / 1e9, "segments": segments, "raw_segments": raw,
                               "host_share_of_encode_call": statistics.median(host)})
            lines.append(json.dumps(result))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
