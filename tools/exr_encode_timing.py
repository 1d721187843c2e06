"""Wall time of writing a denoised frame's passes as EXR files, encoded on the host (openexr.write_image: the code before the device encoder,
unchanged) or on the device (openexr.DeviceEncoder: csrc/dd_exr_encode.hip, csrc/dd_exr_deflate.hip), in one process.

    python tools/exr_encode_timing.py [--passes 15] [--runs 3] [--height 1080] [--width 1920] [--type float|half] [--out profiles/exr_encode.txt]

The predictions are synthetic: `--passes` three-channel fp32 planes on the device, a smooth image plus noise.  Timed, `--runs` times per mode
after one warm-up run, the median reported: openexr.save_predictions(as_exr=True) with encode="host" and with encode="device" (the .npy
files are written by both, as predict.py does).  For the device mode one more DeviceEncoder.encode call of the same planes, events around
the launches, gives the device time of the pack launches and of the deflate launch, the deflate launch's GB/s in (the chunk bytes it reads)
and out (the stream bytes it keeps), the chunks stored raw, and the host's share of that call (assembling and writing the files)."""
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
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--type", default="float", choices=["float", "half"])
    ap.add_argument("--modes", default="host,device")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exr_encode.txt"), help="the result lines are appended to this file")
    args = ap.parse_args()

    from deepdenoiser_amd import openexr
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:args.height, 0:args.width].astype(np.float32)
    predictions = {}
    for k in range(args.passes):
        img = np.stack([0.2 + (k + 1) * 1e-3 * y + (c + 1) * 5e-4 * x for c in range(3)], axis=-1).astype(np.float32)
        img += 0.05 * np.abs(rng.standard_normal(img.shape)).astype(np.float32)
        predictions["prediction/Pass %02d" % k] = torch.from_numpy(img).to(device)
    plane_bytes = args.passes * args.height * args.width * 3 * 4
    lines = []
    with tempfile.TemporaryDirectory() as root:
        for mode in args.modes.split(","):
            seconds, file_bytes = [], 0
            for run in range(args.runs + 1):                       # (the first run warms the allocator, the pinned buffers and the page cache)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = openexr.save_predictions(root, predictions, as_exr=True, encode=mode, pixel_type=args.type)
                torch.cuda.synchronize()
                if run > 0:
                    seconds.append(time.perf_counter() - t0)
                file_bytes = sum(os.path.getsize(p) for p in written if p.endswith(".exr"))
            s = statistics.median(seconds)
            result = {"metric": "save_predictions(as_exr=True): wall seconds (median of %d)" % args.runs, "encode": mode, "type": args.type,
                      "seconds_median": s, "seconds_min": min(seconds), "seconds_max": max(seconds), "passes": args.passes,
                      "frame": [args.height, args.width], "plane_GB": plane_bytes / 1e9, "exr_file_GB": file_bytes / 1e9}
            if mode == "device":
                openexr.DeviceEncoder.time_launches = True
                requests = [(os.path.join(root, "timed_%02d.exr" % k), v, args.type) for k, v in enumerate(predictions.values())]
                pack_ms, deflate_ms, wall, host = [], [], [], []
                encoder = openexr.DeviceEncoder(device, threads=16)
                for run in range(args.runs + 1):
                    encoder.pack_events, encoder.deflate_events, encoder.host_seconds, encoder.raw_chunks = [], [], 0.0, 0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    paths = encoder.encode(requests)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if run > 0:
                        wall.append(dt)
                        host.append(encoder.host_seconds / dt)
                        pack_ms.append(sum(a.elapsed_time(b) for a, b in encoder.pack_events))
                        deflate_ms.append(sum(a.elapsed_time(b) for a, b in encoder.deflate_events))
                raw_chunks = encoder.raw_chunks
                encoder.release()
                openexr.DeviceEncoder.time_launches = False
                size = 2 if args.type == "half" else 4
                chunk_bytes = args.passes * args.height * args.width * 3 * size
                stream_bytes = sum(os.path.getsize(p) for p in paths)
                ms = statistics.median(deflate_ms)
                result.update({"encode_call_seconds_median": statistics.median(wall), "pack_ms_all_launches": statistics.median(pack_ms),
                               "deflate_ms": ms, "deflate_ms_min": min(deflate_ms), "deflate_ms_max": max(deflate_ms),
                               "deflate_in_GB": chunk_bytes / 1e9, "deflate_out_GB": stream_bytes / 1e9,
                               "deflate_in_GB_per_s": chunk_bytes / (ms * 1e-3) / 1e9, "deflate_out_GB_per_s": stream_bytes / (ms * 1e-3) / 1e9,
                               "raw_chunks": raw_chunks, "host_share_of_encode_call": statistics.median(host)})
            lines.append(json.dumps(result))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
