"""The refresh of the importance map under data parallelism, on CPU with gloo and world_size 2 (as tests/test_distributed.py): two ranks hold
different integer tables; after frame_importance.reduce_tables -- the one all_reduce(SUM) of int64 ImportanceScorer.collect issues -- and
ImportanceMap.fold both hold the same `cells` bytes, equal to a fold of the summed tables in one process."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepdenoiser_amd.frame_importance import ImportanceMap, reduce_tables

T, G = 8, 4
SIZES = [(24, 40), (18, 20)]
N_CELLS = 80


class _Scene:
    def __init__(self, h, w):
        self.height, self.width = h, w


class _Bank:
    def __init__(self):
        self.tile, self.scenes = T, [_Scene(h, w) for h, w in SIZES]


def _map():
    rng = np.random.default_rng(1)
    return ImportanceMap.from_cells(_Bank(), [rng.random((h // G, w // G)) ** 4 for h, w in SIZES], cell=G)


def _tables(rank):
    """A rank's tables: about half of the cells visited, some by both ranks; one sum above 2^53 (a float64 all-reduce would round it)."""
    rng = np.random.default_rng(100 + rank)
    counts = np.where(rng.random(N_CELLS) < 0.5, rng.integers(1, 4, N_CELLS), 0).astype(np.uint32)
    sums = np.array([sum(int(np.rint(rng.random() * 2.0 ** 32)) for _ in range(int(c))) for c in counts], dtype=np.uint64)
    counts[3], sums[3] = 3000000 + rank, np.uint64(2 ** 53 + 1)
    return sums, counts


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _map()
        sums, counts = reduce_tables(*_tables(rank), dist)
        folded = m.fold(sums, counts, 0.5)
        torch.save({"sums": sums, "counts": counts, "folded": folded, "cells": [c.tobytes() for c in m.cells], "cdf": m.cdf.tobytes()},
                   "%s.%d" % (out, rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_fold_the_same_summed_tables(tmp_path):
    out = str(tmp_path / "rank")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [torch.load("%s.%d" % (out, r), weights_only=False) for r in range(2)]
    (s0, c0), (s1, c1) = _tables(0), _tables(1)
    assert ((c0 > 0) & (c1 > 0)).any() and ((c0 > 0) != (c1 > 0)).any()
    sums = np.array([int(a) + int(b) for a, b in zip(s0, s1)], dtype=np.uint64)          # exact: Python integers
    counts = (c0.astype(np.int64) + c1.astype(np.int64)).astype(np.uint32)
    assert int(sums[3]) == 2 ** 54 + 2 and float(int(sums[3])) != int(sums[3])           # no float64 holds this sum
    want = _map()
    folded = want.fold(sums, counts, 0.5)
    for g in got:
        assert g["sums"].dtype == np.uint64 and g["counts"].dtype == np.uint32
        assert g["sums"].tobytes() == sums.tobytes() and g["counts"].tobytes() == counts.tobytes()
        assert g["folded"] == folded == int((counts > 0).sum())
        assert g["cells"] == [c.tobytes() for c in want.cells] and g["cdf"] == want.cdf.tobytes()
