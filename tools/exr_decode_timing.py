"""Wall time of loading a frame bank from EXR files, decoded on the host, rebuilt on the device (openexr.DeviceDecoder,
csrc/dd_exr_decode.hip) or inflated and rebuilt on the device (csrc/dd_exr_inflate.hip), next to the HBM copy rate of the same box.

    python tools/exr_decode_timing.py [--decode host|device|device_inflate|both|all] [--threads 4] [--runs 3] [--height 1080] [--width 1920] [--out FILE]

A synthetic tree is written into a temporary directory: two scenes x (1 source + 1 target rendering) x 9 three-channel passes, FLOAT, ZIP, a
smooth image plus noise (the nine files of a rendering are written once and copied: what a decoder does does not depend on whose file it
is).  Timed: FrameBank.for_passes over the whole tree, `--runs` times per mode, the median reported; seconds, files / s and decoded GB / s (the
fp32 bytes of the planes).  Device mode also reports the device time of the dd_exr_reconstruct launches alone (HIP events around every
launch; the kernel reads the staged bytes twice where a chunk is coded, rewrites them once and writes the planes -- `kernel_GB_per_s` counts
staged bytes + plane bytes once, against bench.hbm_copy_rate of the same process) and the share of the wall time the loader spent waiting
for the inflate threads.  Mode device_inflate (decode on the device, inflate="device") adds the device time of the dd_exr_inflate launches
alone (events), as compressed GB/s (the stream bytes read) and inflated GB/s (the bytes written), the bytes uploaded and the files redone on
the host.  `both` is host + device, `all` (the default) the three modes in one process: the baseline of device_inflate is the `device` line
of the same call."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PASSES = ["Diffuse Color", "Diffuse Direct", "Diffuse Indirect", "Glossy Color", "Glossy Direct", "Glossy Indirect", "Transmission Color",
          "Transmission Direct", "Transmission Indirect"]
SPP, TARGET_SPP = 4, 64


def write_tree(root, height, width, scenes=2):
    from deepdenoiser_amd import openexr
    from deepdenoiser_amd.render_passes import _ORDERED
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    master = os.path.join(root, "master")
    os.makedirs(master)
    for k, name in enumerate(PASSES):
        img = np.stack([0.2 + (k + 1) * 1e-3 * y + (c + 1) * 5e-4 * x for c in range(3)], axis=-1).astype(np.float32)
        img += 0.05 * np.abs(rng.standard_normal(img.shape)).astype(np.float32)
        openexr.write_image(os.path.join(master, "render_%s_0001.exr" % name), img)
    names = []
    for s in range(scenes):
        scene = "scene%d" % s
        names.append(scene)
        for spp in (SPP, TARGET_SPP):
            shutil.copytree(master, os.path.join(root, "OpenEXR", scene, "%s_%d_0_0" % (scene, spp)))
    shutil.rmtree(master)
    flags = {"use_" + attr.lower(): (name in PASSES) for attr, name in _ORDERED}
    j = {"base_exr_directory": "OpenEXR", "base_tfrecords_directory": "TFRecords",
         "modes": {"training": {"group_by_samples_per_pixel": False, "tiles_height_width": 128, "examples_per_tfrecords": 16, "exr_directories": names}},
         "source": {"samples_per_pixel": [SPP], "number_of_sources_per_example": 1, "features": flags},
         "target": {"samples_per_pixel": TARGET_SPP, "features": flags}}
    path = os.path.join(root, "tfrecords.json")
    with open(path, "w") as f:
        json.dump(j, f)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", default="all", choices=["host", "device", "device_inflate", "both", "all"])
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default="", help="also append the result lines to this file")
    args = ap.parse_args()

    import bench
    from deepdenoiser_amd import openexr
    from deepdenoiser_amd.frame_bank import FrameBank, FrameSet
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    openexr.DeviceDecoder.time_launches = True                 # (events around every launch)
    channels = {name: 3 for name in PASSES}
    lines = []
    with tempfile.TemporaryDirectory() as root:
        frames_json = write_tree(root, args.height, args.width)
        frame_set = FrameSet.from_json(frames_json, "training", log=lambda m: None)
        n_files = len(frame_set.scenes) * 2 * len(PASSES)
        file_bytes = sum(os.path.getsize(os.path.join(d, n)) for d, _, ns in os.walk(root) for n in ns if n.endswith(".exr"))
        copy_rate = bench.hbm_copy_rate(device)
        modes = {"both": ["host", "device"], "all": ["host", "device", "device_inflate"]}.get(args.decode, [args.decode])
        stream_bytes = inflated_bytes = 0
        if "device_inflate" in modes:                          # (what the inflate launches read and write: from the plans, outside the timing)
            for d, _, ns in os.walk(root):
                for n in ns:
                    if n.endswith(".exr"):
                        table = openexr.plan_file(os.path.join(d, n)).source_layout()[1]
                        stream_bytes += int(table["src_bytes"].sum())
                        inflated_bytes += int(table["dst_bytes"].sum())
        for mode in modes:
            seconds, kernel_ms, inflate, launches, inflate_ms, uploaded, fallbacks, inflate_launches = [], [], [], 0, [], 0, 0, 0
            for run in range(args.runs + 1):                   # (the first run warms the page cache, the allocator and the pinned ring)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bank = FrameBank.for_passes(frame_set, channels, channels, SPP, device=device, threads=args.threads, log=lambda m: None,
                                            decode="host" if mode == "host" else "device", inflate="device" if mode == "device_inflate" else "host")
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                created = [bank.decoder] if bank.decoder is not None else []
                plane_bytes = bank.total_bytes
                assert len(bank.scenes) == len(frame_set.scenes)
                if run > 0:
                    seconds.append(dt)
                    if created:
                        kernel_ms.append(sum(a.elapsed_time(b) for d in created for a, b in d.events))
                        inflate.append(sum(d.inflate_seconds for d in created) / dt)
                        launches = sum(d.launches for d in created)
                        if mode == "device_inflate":
                            inflate_ms.append(sum(a.elapsed_time(b) for d in created for a, b in d.inflate_events))
                            uploaded, fallbacks = sum(d.uploaded_bytes for d in created), sum(d.host_fallbacks for d in created)
                            inflate_launches = sum(d.inflate_launches for d in created)
                del bank
            s = statistics.median(seconds)
            result = {"metric": "FrameBank from EXR files: wall seconds (median of %d)" % args.runs, "decode": mode, "threads": args.threads,
                      "seconds_median": s, "seconds_min": min(seconds), "seconds_max": max(seconds), "files": n_files, "files_per_s": n_files / s,
                      "frame": [args.height, args.width], "file_GB": file_bytes / 1e9, "decoded_GB": plane_bytes / 1e9, "decoded_GB_per_s": plane_bytes / s / 1e9,
                      "hbm_copy_rate_GB_per_s": copy_rate}
            if kernel_ms:
                ms = statistics.median(kernel_ms)
                result.update({"launches": launches, "kernel_ms_all_launches": ms, "kernel_GB_per_s": 2 * plane_bytes / (ms * 1e-3) / 1e9,
                               "kernel_time_over_copy_time": copy_rate / (2 * plane_bytes / (ms * 1e-3) / 1e9),
                               "inflate_share_of_wall": statistics.median(inflate)})
            if inflate_ms:
                ms = statistics.median(inflate_ms)
                result.update({"inflate_launches": inflate_launches, "inflate_ms_all_launches": ms, "inflate_ms_min": min(inflate_ms),
                               "inflate_ms_max": max(inflate_ms), "compressed_GB": stream_bytes / 1e9, "inflated_GB": inflated_bytes / 1e9,
                               "compressed_GB_per_s": stream_bytes / (ms * 1e-3) / 1e9, "inflated_GB_per_s": inflated_bytes / (ms * 1e-3) / 1e9,
                               "uploaded_GB": uploaded / 1e9, "host_fallbacks": fallbacks})
            lines.append(json.dumps(result))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
