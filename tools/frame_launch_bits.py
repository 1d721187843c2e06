"""The bits of the three frame-level launches (dd_temporal_stabilize, dd_sequence_quality, dd_frame_quality) on seeded inputs, as one sha256
per launch over the record bytes, the outputs (whole frames: the channels past nch included) and the SSIM maps.  Two libraries that print the
same lines compute the same thing: run it once per library (DD_LIB=<path to a libdd_hip.so> selects one; the C ABI must be the same).

    python tools/frame_launch_bits.py [--time] [--out FILE]

Inputs are built on the host (numpy, fixed seeds): radiances with a wide range and a few NaN / Inf, motions on multiples of 1/8 pixel of which
some leave the frame.  Shapes: 45 x 70 with mixed layouts (dense RGB, a [..., :1] view of a 3-wide frame, RGB at ld 5), 1 x 4097 (257 tiles
of 16: the second round of the finalize kernels' strided add) for the two motion launches, 11 x 8193 (257 tiles of 32) and 25 pairs of
270 x 480 for the quality launch.  --time adds the device time of dd_frame_quality for 15 passes of 1920 x 1080 (12 RGB, 3 one-channel views):
HIP events, the median of 3 after 2 warm-ups; a record, nothing is gated."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepdenoiser_amd import _lib, metrics  # noqa: E402

MIX = ((3, 3), (1, 3), (3, 5))      # (channels, ld) of the passes of a mixed call
SENTINEL = 77.0


def radiance(rng, H, W, C, sprinkle):
    v = (np.abs(rng.standard_normal((H, W, C))) * np.exp(rng.normal(0.0, 1.5, (H, W, 1)))).astype(np.float32)
    if sprinkle:
        flat = v.reshape(-1)
        flat[rng.integers(0, flat.size, 3)] = (np.nan, np.inf, -np.inf)
    return v


def motion(rng, H, W):
    """[H,W,3]: multiples of 1/8 pixel up to 3 pixels, a few far outside the frame and one NaN"""
    m = (rng.integers(-24, 25, (H, W, 3)) / 8.0).astype(np.float32)
    far = rng.integers(0, H * W, max(H * W // 50, 1))
    m.reshape(-1, 3)[far, 0] = 1e6
    m.reshape(-1, 3)[rng.integers(0, H * W), 1] = np.nan
    return m


def frame(values, ld, keep):
    """values [H,W,C] -> the [..., :C] view of a device [H,W,ld] frame (dense for ld == C); keep: collects the whole frames"""
    H, W, C = values.shape
    wide = np.full((H, W, ld), np.float32(SENTINEL), dtype=np.float32)
    wide[..., :C] = values
    whole = torch.from_numpy(wide).cuda()
    keep.append(whole)
    return whole[..., :C]


def buffers(scratch_bytes, record_type, n, H, W):
    nbytes = scratch_bytes(n, H, W)
    assert nbytes > 0
    return (torch.full((n * ctypes.sizeof(record_type),), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device="cuda"))


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def stream():
    return torch.cuda.current_stream().cuda_stream


def temporal(lib, H, W, seed):
    rng = np.random.default_rng(seed)
    keep, outs = [], []
    table = (_lib.TemporalPass * len(MIX))()
    for k, (C, ld) in enumerate(MIX):
        cur, his = frame(radiance(rng, H, W, C, True), ld, keep), frame(radiance(rng, H, W, C, k == 1), ld, keep)
        out = frame(np.full((H, W, C), SENTINEL, dtype=np.float32), ld, outs)
        table[k] = _lib.TemporalPass(cur.data_ptr(), his.data_ptr(), out.data_ptr(), cur.stride(1), his.stride(1), out.stride(1), C)
    guides = (_lib.TemporalGuide * 2)()
    for k, (C, ld) in enumerate(((3, 3), (1, 3))):
        a, b = (frame((rng.integers(0, 3, (H, W, C)) / 2.0).astype(np.float32), ld, keep) for _ in range(2))
        guides[k] = _lib.TemporalGuide(a.data_ptr(), b.data_ptr(), a.stride(1), b.stride(1), C, 0.25)
    mv = torch.from_numpy(motion(rng, H, W)).cuda()
    records, scratch = buffers(lib.dd_temporal_scratch_bytes, _lib.TemporalRecord, len(MIX), H, W)
    _lib.check(lib.dd_temporal_stabilize(table, len(MIX), guides, 2, H, W, mv.data_ptr(), mv.stride(1), -1.0, 1.0, 0.8, 1.0, records.data_ptr(),
                                         scratch.data_ptr(), stream()))
    return digest(records, *outs)


def sequence(lib, H, W, seed):
    rng = np.random.default_rng(seed)
    keep = []
    table = (_lib.SequenceQualityPair * len(MIX))()
    for k, (C, ld) in enumerate(MIX):
        p, pp, t, tp = (frame(radiance(rng, H, W, C, j == k), ld if j % 2 == 0 else C, keep) for j in range(4))
        table[k] = _lib.SequenceQualityPair(p.data_ptr(), pp.data_ptr(), t.data_ptr(), tp.data_ptr(), p.stride(1), pp.stride(1), t.stride(1), tp.stride(1), C)
    mv = torch.from_numpy(motion(rng, H, W)).cuda()
    thr = torch.from_numpy(metrics.preview_thresholds()).cuda()
    records, scratch = buffers(lib.dd_sequence_quality_scratch_bytes, _lib.SequenceQualityRecord, len(MIX), H, W)
    _lib.check(lib.dd_sequence_quality(table, len(MIX), H, W, mv.data_ptr(), mv.stride(1), -1.0, 1.0, thr.data_ptr(), 1.0, records.data_ptr(),
                                       scratch.data_ptr(), stream()))
    return digest(records)


def quality_call(lib, pairs, H, W, maps):
    """pairs: [(prediction view, target view)] -> (the function that makes the call, the records, the maps)"""
    n = len(pairs)
    table = (_lib.QualityPair * n)()
    for k, (p, t) in enumerate(pairs):
        table[k] = _lib.QualityPair(p.data_ptr(), t.data_ptr(), p.stride(1), t.stride(1), p.shape[2])
    thr = torch.from_numpy(metrics.preview_thresholds()).cuda()
    records, scratch = buffers(lib.dd_frame_quality_scratch_bytes, _lib.QualityRecord, n, H, W)
    out_maps = [torch.full((H - 10, W - 10), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(n if maps else 0)]
    ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in out_maps]) if maps else None

    def launch(_images=pairs):      # (the table holds addresses: the call keeps the images alive)
        _lib.check(lib.dd_frame_quality(table, n, H, W, thr.data_ptr(), 1.0, 1e-2, ptrs, records.data_ptr(), scratch.data_ptr(), stream()))
    return launch, records, out_maps


def quality(lib, H, W, seed, layouts):
    rng = np.random.default_rng(seed)
    keep = []
    pairs = [(frame(radiance(rng, H, W, C, k % 2 == 1), pld, keep), frame(radiance(rng, H, W, C, False), tld, keep)) for k, (C, pld, tld) in enumerate(layouts)]
    launch, records, maps = quality_call(lib, pairs, H, W, True)
    launch()
    return digest(records, *maps)


def quality_ms(lib, H=1080, W=1920, rgb=12, gray=3, steps=3, warmup=2):
    gen = torch.Generator(device="cuda").manual_seed(3)

    def images():
        return [torch.randn((H, W, 3), device="cuda", generator=gen).abs()[..., :C] for C in [3] * rgb + [1] * gray]
    launch = quality_call(lib, list(zip(images(), images())), H, W, False)[0]
    times = []
    for step in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if step >= warmup:
            times.append(e0.elapsed_time(e1))
    return {"metric": "dd_frame_quality: device ms per call (scoring launch + finalize)", "ms_median": statistics.median(times),
            "ms_min": min(times), "ms_max": max(times), "steps": steps, "warmup": warmup, "frame": [H, W], "rgb_pairs": rgb, "gray_pairs": gray,
            "note": "measured once, not gated"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="also time dd_frame_quality on 15 passes of 1920 x 1080")
    ap.add_argument("--out", default="", help="also append the printed lines to this file")
    args = ap.parse_args()
    lib = _lib.load()
    torch.cuda.set_device(0)
    mixed = [(3, 3, 3), (1, 3, 1), (3, 4, 3)]
    lines = ["library %s" % lib.dd_version().decode(),
             "temporal 45x70 mixed       %s" % temporal(lib, 45, 70, 1),
             "temporal 1x4097            %s" % temporal(lib, 1, 4097, 2),
             "sequence 45x70 mixed       %s" % sequence(lib, 45, 70, 3),
             "sequence 1x4097            %s" % sequence(lib, 1, 4097, 4),
             "quality 45x70 mixed        %s" % quality(lib, 45, 70, 5, mixed),
             "quality 11x8193            %s" % quality(lib, 11, 8193, 6, mixed[:2]),
             "quality 270x480 25 pairs   %s" % quality(lib, 270, 480, 7, [mixed[k % 3] for k in range(25)])]
    if args.time:
        lines.append(json.dumps(quality_ms(lib)))
    for line in lines:
        print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
