"""-m gpu: the dynamic loss scale under data parallelism -- two Trainer processes on one GPU (gloo transport, as tests/test_gpu_distributed.py).
The non-finite scan reads the arena AFTER the all-reduce, where an inf / NaN of either rank is an inf / NaN of the sum, so both ranks must skip
the same steps without exchanging anything more: identical scaler records and bit-identical parameters after 20 steps that start at 2^40.

The backoff is 1/8 here: 13 skipped steps take 2^40 down to 2, where the stored gradients are twice the unscaled ones, so at least 7 of the 20 steps
are APPLIED whatever the gradients' size (with the conventional 1/2 all 20 could be skips, and equal parameters would show nothing)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_distributed import _free_port
from test_gpu_loss_scale import INIT, _arch, _batch

pytestmark = pytest.mark.gpu

STEPS, BACKOFF = 20, 0.125
GLOBAL_B, H, W = 4, 32, 32


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from deepdenoiser_amd.training import Trainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        arch, tj = _arch({"init": INIT, "backoff": BACKOFF})                                  # identical replica on every rank
        B = GLOBAL_B // world
        trainer = Trainer(arch, tj, B, H, W, world_size=world, n_buckets=3, force_segments=True)
        g = torch.Generator().manual_seed(100 + rank)                     # every rank its own shard
        feats, labels = _batch(arch)
        feats = {k: (v.cpu() * (1.0 + torch.rand(v.shape, generator=g))).cuda() for k, v in feats.items()}
        trainer.program.set_inputs(feats, labels)
        for _ in range(STEPS):
            trainer.step()
        torch.cuda.synchronize()
        assert trainer._graphs is not None and len(trainer._segments) == 3
        torch.save({"state": trainer.program.scaler.state(), "values": arch.params.values.cpu().clone()}, "%s.%d" % (out, rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_take_the_same_skip_decisions(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = str(tmp_path / "rank")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    print("rank 0:", r0["state"], " rank 1:", r1["state"])
    st = r0["state"]
    assert st == r1["state"]
    assert st["skipped_total"] >= 1 and st["adam_t"] >= 7 and st["adam_t"] + st["skipped_total"] == STEPS
    assert st["scale"] == max(INIT * BACKOFF ** st["skipped_total"], 1.0)
    assert torch.equal(r0["values"], r1["values"]), "replicas diverged"
    assert bool(torch.isfinite(r0["values"]).all())
