"""Time per predict_frame() over a 1920 x 1080 frame sequence of the bench's inference configuration (cfg-2, fp16, tiles of 128 with overlap 14)
with tile_blend "crop" and "feather", alternating in ONE process -- the A/B behind DESIGN.md section 3.21.  Wall time over `--frames` frames
after `--warmup`, like bench.py's inference mode, `--runs` times per mode, the modes taking turns; the frames are bench.py's (device-resident,
three buffer sets).  Also: the device time of the stitch launches of a frame on their own, and the sha256 of the last frame's outputs.
`--modes crop` passes no keyword this tool's commit added, so it also runs from a checkout of an older commit (run it with that checkout as
the working directory): the crop path must time inside the run's own spread there and here, and give the same sha256.

    python tools/stitch_blend_ab.py --out profiles/stitch_blend_ab.txt
    python tools/stitch_blend_ab.py --modes crop --label parent
"""
import argparse
import hashlib
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


def stitch_ms(pred, reps=50):
    """device time of the stitch launches of one frame (every tile batch), on the tiles the last forward left: events around `reps` frames' worth"""
    from deepdenoiser_amd import _lib as L
    plan, prog, chunks = pred._frame_plan(H, W)
    T, NF = plan.tile, prog.NF
    frames = torch.empty((NF, H, W, 3), dtype=torch.float32, device="cuda:0")
    stream = prog.g.stream_ptr()
    tiles = prog.predictions[0]
    blend = getattr(pred, "_blends", {}).get((H, W))

    def once():
        first = 0
        for oyx, tdev, n in chunks:
            if blend is None:
                L.check(pred.lib.dd_stitch(tiles.ptr, T, 3, frames.data_ptr(), H, W, 3, 3, tdev.data_ptr(), n, stream))
            else:
                blend.blend(pred.lib, tiles.ptr, 3, oyx.shape[0], frames, 3, first, n // NF, stream)
                first += n // NF
    once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="crop,feather")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tiles_per_batch", type=int, default=256)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="append the result line to this file")
    args = ap.parse_args()
    modes = args.modes.split(",")
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cuda:0", dtype=args.dtype, seed=2)
    preds = {m: Predictor(arch, tile_size=128, tile_overlap_size=14, tiles_per_batch=args.tiles_per_batch, **({} if m == "crop" else {"tile_blend": m}))
             for m in modes}
    g = torch.Generator().manual_seed(7)
    feats = arch.feature_predictions + arch.auxiliary_features
    frames = [{Naming.source_feature_name(f.name, index=0): torch.randn(H, W, f.number_of_channels, generator=g).abs().to("cuda:0") for f in feats}
              for _ in range(3)]
    for m in modes:
        for i in range(max(2, args.warmup)):
            preds[m].predict_frame(frames[i % len(frames)])
    ms = {m: [] for m in modes}
    digest = {}
    for _ in range(args.runs):
        for m in modes:                                            # the modes take turns: a drift of the machine hits both
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.frames):
                out = preds[m].predict_frame(frames[i % len(frames)])
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / args.frames)
            h = hashlib.sha256()
            for k in sorted(out):
                h.update(k.encode() + out[k].contiguous().cpu().numpy().tobytes())
            digest[m] = h.hexdigest()[:16]
    res = {"label": args.label, "dtype": args.dtype, "frames": args.frames, "runs": args.runs, "tiles_per_batch": args.tiles_per_batch}
    for m in modes:
        res[m] = {"ms_per_frame": [round(x, 4) for x in ms[m]], "median_ms": round(sorted(ms[m])[len(ms[m]) // 2], 4),
                  "stitch_ms": round(stitch_ms(preds[m]), 4), "output_sha256": digest[m],
                  "output_finite": bool(all(torch.isfinite(v).all() for v in preds[m].predict_frame(frames[0]).values()))}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
