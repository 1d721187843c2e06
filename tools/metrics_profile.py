"""What the tracked-metric launches cost (the measurement behind the DESIGN section on tracked metrics; bench.py is not changed).

    python tools/metrics_profile.py [--repeats 20] [--out FILE.json]                                  # HIP-event times per scale + total
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/metrics_profile.py --repeats 20           # kernel times, in a run of its own

Configurations (bf16 storage):
  example   the 17-pass example network (TrainingExample defaults: track_mean on all three levels, 3 scales), B = 8, 128 x 128
  example+  the same with track_variation and the masked means switched on as well (same launches: one per scale evaluates everything)
  cfg2      bench.py's cfg-2 (one pass), B = 128, 128 x 128
Next to every time: the algorithmic bytes (prediction and target of every loaded pass once per scale, 2 x 12 B per pixel) and the rate they
amount to."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import synthetic_inputs  # noqa: E402
from deepdenoiser_amd import configs  # noqa: E402
from deepdenoiser_amd.architecture import Architecture  # noqa: E402

LEVELS = ("features_training_settings", "combined_features_training_settings", "combined_image_training_settings")


def variants():
    plus = configs.training()
    for lv in LEVELS:
        plus[lv]["statistics"].update(track_mean=True, track_variation=True)
    no_alpha = {k: v for k, v in configs._FULL_COMBINED.items() if k != "Alpha"}
    for lv in LEVELS[:2]:
        plus[lv]["statistics_masked"].update(track_mean=True)
    return [("example", configs.example_architecture(), configs.training(), 8),
            ("example+", configs.architecture(combined=no_alpha), plus, 8),
            ("cfg2", configs.cfg2_unet_kpcn(), configs.bench_training(), 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = {}
    for name, aj, tj, B in variants():
        arch = Architecture(aj, device="cuda", dtype="bf16")
        H = W = args.tile
        prog = arch.program(B, H, W, training_json=tj)
        feats, labels = synthetic_inputs(arch, B, H, W, "cuda", 3)
        prog.set_inputs(feats, labels)
        prog.zero_grads()
        prog.forward()
        tracked = prog.tracking_metrics
        stream = prog.g.stream_ptr()
        loaded = sum(1 for f in prog.head if f.load_data)
        for op in tracked.launches:      # warm-up
            op(stream)
        torch.cuda.synchronize()
        per = []
        for j, op in enumerate(tracked.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.repeats):
                op(stream)
            e1.record()
            torch.cuda.synchronize()
            s = tracked.scales[j]
            nbytes = 2 * 12 * B * (H >> s) * (W >> s) * loaded
            us = 1e3 * e0.elapsed_time(e1) / args.repeats
            per.append({"scale": s, "us": us, "algorithmic_bytes": nbytes, "GB_per_s": nbytes / us * 1e-3})
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeats):
            prog.metric_table()
        e1.record()
        torch.cuda.synchronize()
        total_us = 1e3 * e0.elapsed_time(e1) / args.repeats
        import time
        t0 = time.perf_counter()
        for _ in range(args.repeats):
            prog.metrics()
        host_us = 1e6 * (time.perf_counter() - t0) / args.repeats
        total_bytes = sum(p["algorithmic_bytes"] for p in per)
        results[name] = {"B": B, "tile": H, "passes": len(prog.head), "loaded_passes": loaded, "metrics": len(tracked.plan), "per_scale": per,
                         "all_scales_us": total_us, "all_scales_GB_per_s": total_bytes / total_us * 1e-3, "metrics_call_with_copy_us": host_us}
        print("%-9s B=%d %dx%d %2d passes %3d metrics: %s | all scales %.1f us (%.0f GB/s algorithmic) | metrics() incl. copy and host %.0f us" % (
            name, B, H, W, len(prog.head), len(tracked.plan),
            "  ".join("1/%d %.1f us %.0f GB/s" % (1 << p["scale"], p["us"], p["GB_per_s"]) for p in per), total_us,
            results[name]["all_scales_GB_per_s"], host_us), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
