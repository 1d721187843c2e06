"""What the tracked metrics cost a validation pass (the ratio recorded in DESIGN): times train.run_validation on a synthetic validation set of
the 17-pass example network (TrainingExample defaults: track_mean on all three levels, 3 scales), bf16, B = 8, 64 x 64 tiles, 32 examples.

    python tools/validation_cost.py --data DIR --make                      # write the data set once
    python tools/validation_cost.py --data DIR [--root TREE] [--passes 3]  # time the validation pass of the package in TREE (default: this tree)

Run it alternately on two checkouts (--root) in one session to compare them; a tree without tracked metrics runs its plain validation."""
import argparse
import inspect
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--data", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--make", action="store_true")
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--threads", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepdenoiser_amd import configs, tfrecords  # noqa: E402
from deepdenoiser_amd.architecture import Architecture  # noqa: E402
from deepdenoiser_amd.naming import Naming  # noqa: E402

T, SPP, B, EXAMPLES, FILES = 64, 16, 8, 32, 4
aj, tj = configs.example_architecture(), configs.training()
tj["number_of_source_index_tuples"] = 1

if args.make:
    arch = Architecture(aj, device="cpu")
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(args.data, "validation"), exist_ok=True)
    json.dump({"tiles_height_width": T, "number_of_sources_per_example": 1, "source_samples_per_pixel_list": [SPP]},
              open(os.path.join(args.data, "validation.json"), "w"))
    passes = {f.name: f.number_of_channels for f in arch.feature_predictions + arch.auxiliary_features if f.load_data}
    targets = [f.name for f in arch.feature_predictions if f.load_data and f.is_target]
    for n in range(FILES):
        records = []
        for _ in range(EXAMPLES // FILES):
            feats = {}
            for name, ch in passes.items():
                clean = rng.random((T, T, ch), dtype=np.float32)
                feats[Naming.source_feature_name(name, samples_per_pixel=SPP, index=0)] = (clean * (1 + 0.3 * rng.standard_normal((T, T, ch), dtype=np.float32))).tobytes()
                if name in targets:
                    feats[Naming.target_feature_name(name)] = clean.tobytes()
            records.append(tfrecords.serialize_example(feats))
        tfrecords.write_records(os.path.join(args.data, "validation", "validation_%d.tfrecords.gz" % n), records)
    print("wrote %d examples to %s" % (EXAMPLES, args.data))
    sys.exit(0)

from deepdenoiser_amd import train  # noqa: E402
from deepdenoiser_amd.training import Trainer  # noqa: E402

arch = Architecture(aj, device="cuda", dtype="bf16")
trainer = Trainer(arch, tj, B, T, T)
tracked = "metrics_out" in inspect.signature(train.run_validation).parameters
times = []
for k in range(args.passes + 1):
    out = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = train.run_validation(trainer, arch, tj, args.data, B, 0, 1, args.threads, **({"metrics_out": out} if tracked else {}))
    torch.cuda.synchronize()
    if k:      # (the first pass builds the launches)
        times.append(time.perf_counter() - t0)
print("RESULT root=%s tracked=%d metrics=%d loss=%.6f seconds_per_pass=%s median=%.4f" % (
    args.root, tracked, len(next(iter(out.values()), [])), res[0][1], ",".join("%.4f" % t for t in times), sorted(times)[len(times) // 2]), flush=True)
