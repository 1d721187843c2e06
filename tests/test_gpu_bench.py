"""-m gpu: what every benchmark run relies on -- a plain `bench.py` line carries the headline only, and `--dump-outputs` writes what the last
timed step hands its caller (the loss and the weights after its Adam update; that step starts from the seeded state) as float32 .npy files,
which two runs with the same arguments reproduce up to the rounding of the unordered fp32 reductions, without changing the timed path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS, WARMUP = 8, 10, 3


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--batch", str(B)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_and_dump_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    plain = _bench()
    assert plain["unit"] == "tiles/s" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert plain["steps"] == STEPS and plain["warmup"] == WARMUP and plain["ms_per_step"] > 0
    assert abs(plain["value"] - B * 1e3 / plain["ms_per_step"]) <= 1e-9 * plain["value"]
    assert not {"roofline", "allreduce", "extras", "cpu_baseline"} & set(plain)          # --full only
    runs = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("run1", "run2")]
    for rec in runs:       # writing outputs changes neither the line nor the timed path
        assert set(rec) == set(plain) and set(rec["config"]) == set(plain["config"])
        assert rec["ms_per_step"] < 3.0 * plain["ms_per_step"], (rec["ms_per_step"], plain["ms_per_step"])
    files = sorted(os.listdir(tmp_path / "run1"))
    assert files == ["loss.npy", "params.npy"] and sorted(os.listdir(tmp_path / "run2")) == files
    a = {f: np.load(tmp_path / "run1" / f) for f in files}
    b = {f: np.load(tmp_path / "run2" / f) for f in files}
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in list(a.values()) + list(b.values()))
    assert float(a["loss.npy"][0]) == runs[0]["config"]["final_loss"] and float(b["loss.npy"][0]) == runs[1]["config"]["final_loss"]
    # the weights after the last step's first Adam update from the seeded state: every element moved by at most the learning rate, most by about it
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cuda:0", dtype="bf16", seed=2)
    arch.program(B, 128, 128, training_json=configs.bench_training())
    w0 = arch.params.values.cpu().numpy()
    lr = configs.bench_training()["learning_rate"]
    step = np.abs(a["params.npy"].astype(np.float64) - w0)
    assert a["params.npy"].shape == w0.shape and step.max() <= 1.001 * lr and np.median(step) > 0.5 * lr, (step.max(), np.median(step))
    # two runs: the same up to the rounding of the unordered reductions
    assert abs(float(a["loss.npy"][0]) - float(b["loss.npy"][0])) <= 1e-5 * abs(float(a["loss.npy"][0]))
    d = np.abs(a["params.npy"].astype(np.float64) - b["params.npy"])
    assert np.linalg.norm(d) <= 1e-5 * np.linalg.norm(a["params.npy"]) and d.max() <= 0.1 * lr, (np.linalg.norm(d), d.max())
