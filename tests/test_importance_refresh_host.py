"""Importance scores refreshed from the model's error, host side (no GPU): ImportanceMap.fold on a two-scene map made with from_cells, the
command line, and where Program.train_step and the Trainer's first segment run Program.step_tail_ops -- on stand-ins that record the
launches, and on the cfg-2 program built on the CPU device with its launch lists replaced by recorders."""
import random

import numpy as np
import pytest

from deepdenoiser_amd.frame_importance import DEFAULT_RATE, ImportanceMap

T, G = 8, 4
SIZES = [(24, 40), (18, 20)]
TUPLES = [[0], [1]]


class _Scene:
    def __init__(self, h, w):
        self.height, self.width = h, w


class _Bank:
    def __init__(self):
        self.tile, self.scenes = T, [_Scene(h, w) for h, w in SIZES]


def _cells():
    rng = np.random.default_rng(1)
    out = [rng.random((h // G, w // G)) ** 4 for h, w in SIZES]
    out[0][:2, :3] = 0.0
    return out


def _tables(seed=7):
    """Integer tables over the 60 + 20 cells: a third of the cells visited 1 .. 5 times, with mean errors in [0, 1]."""
    rng = np.random.default_rng(seed)
    n = sum((h // G) * (w // G) for h, w in SIZES)
    assert n == 80
    counts = np.where(rng.random(n) < 1.0 / 3.0, rng.integers(1, 6, n), 0).astype(np.uint32)
    sums = np.zeros(n, dtype=np.uint64)
    for k in np.nonzero(counts)[0]:
        sums[k] = sum(int(np.rint(rng.random() * 2.0 ** 32)) for _ in range(int(counts[k])))
    assert 10 < (counts > 0).sum() < 50
    return sums, counts


@pytest.mark.parametrize("rate", [0.5, 0.125, 1.0])
def test_fold_moves_visited_cells_and_rebuilds_the_density(rate):
    before = _cells()
    m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G, floor=0.25)
    sums, counts = _tables()
    folded = m.fold(sums, counts, rate)
    assert folded == int((counts > 0).sum())
    at = 0
    want = []
    for c in before:
        new = c.copy()
        for k in range(c.size):
            i, j = divmod(k, c.shape[1])
            if counts[at + k] > 0:
                mean = float(int(sums[at + k])) / 2.0 ** 32 / float(int(counts[at + k]))
                new[i, j] = (1.0 - rate) * c[i, j] + rate * mean
                if rate == 1.0:
                    assert new[i, j] == mean                    # rate = 1 replaces
        at += c.size
        want.append(new)
    for have, new, old in zip(m.cells, want, before):
        assert have.dtype == np.float64 and have.tobytes() == new.tobytes()
    # unvisited cells keep their bytes
    flat_old, flat_new = np.concatenate([c.reshape(-1) for c in before]), np.concatenate([c.reshape(-1) for c in m.cells])
    assert flat_old[counts == 0].tobytes() == flat_new[counts == 0].tobytes()
    assert (flat_old[counts > 0] != flat_new[counts > 0]).any()
    # the rebuilt density is the one from_cells makes of the new cells
    fresh = ImportanceMap.from_cells(_Bank(), want, cell=G, floor=0.25)
    assert m.total == fresh.total and m.cdf.tobytes() == fresh.cdf.tobytes() and m.n_lattice == fresh.n_lattice
    assert (m.offsets == fresh.offsets).all() and (m.tile, m.cell, m.floor, m.sizes) == (fresh.tile, fresh.cell, fresh.floor, fresh.sizes)
    for a, b in zip(m.weights, fresh.weights):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(m.probabilities(), fresh.probabilities()):
        assert a.tobytes() == b.tobytes()
    ra, rb = random.Random(11), random.Random(11)
    assert [m.draw(ra, TUPLES) for _ in range(500)] == [fresh.draw(rb, TUPLES) for _ in range(500)]
    assert ra.random() == rb.random()                           # the same number of calls on the generator
    assert m.describe() == fresh.describe()


def test_fold_without_visits_changes_nothing_and_bad_arguments_raise():
    m = ImportanceMap.from_cells(_Bank(), _cells(), cell=G)
    cdf = m.cdf.tobytes()
    assert m.fold(np.zeros(80, dtype=np.uint64), np.zeros(80, dtype=np.uint32), 0.5) == 0
    assert m.cdf.tobytes() == cdf and all(a.tobytes() == b.tobytes() for a, b in zip(m.cells, _cells()))
    sums, counts = _tables()
    for rate in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rate"):
            m.fold(sums, counts, rate)
    assert m.cdf.tobytes() == cdf                               # a refused fold leaves the map alone
    with pytest.raises(ValueError, match="80 cells"):
        m.fold(sums[:79], counts[:79], 0.5)
    # int64 tables (what the all-reduce over the ranks returns) fold like the unsigned ones
    a, b = ImportanceMap.from_cells(_Bank(), _cells(), cell=G), ImportanceMap.from_cells(_Bank(), _cells(), cell=G)
    a.fold(sums, counts, 0.5)
    b.fold(sums.astype(np.int64), counts.astype(np.int64), 0.5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.cells, b.cells))


# ---------------------------------------------------------------------------------------------------- the command line
def test_parser_flags(capsys):
    from deepdenoiser_amd import train
    assert "frames_importance_refresh" in train.IMPORTANCE_FLAGS and DEFAULT_RATE == 0.5
    args = train.parser().parse_args(["t.json"])
    assert (args.frames_importance_refresh, args.frames_importance_rate) == (None, 0.5)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_crops", "importance"])
    assert (args.frames_importance_refresh, args.frames_importance_rate) == (None, 0.5)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_crops", "importance", "--frames_importance_refresh", "25"])
    assert (args.frames_importance_refresh, args.frames_importance_rate) == (25, 0.5)
    args = train.parser().parse_args(["t.json", "--frames", "f.json", "--frames_crops", "importance", "--frames_importance_refresh", "1",
                                      "--frames_importance_rate", "0.125"])
    assert (args.frames_importance_refresh, args.frames_importance_rate) == (1, 0.125)
    for crops in ("random", "grid"):
        with pytest.raises(SystemExit):
            train.parser().parse_args(["t.json", "--frames_crops", crops, "--frames_importance_refresh", "4"])
        assert "--frames_importance_refresh needs --frames_crops importance" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parser().parse_args(["t.json", "--frames_importance_refresh", "4"])
    assert "--frames_importance_refresh needs --frames_crops importance" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parser().parse_args(["t.json", "--frames_crops", "importance", "--frames_importance_rate", "0.25"])
    assert "--frames_importance_rate needs --frames_importance_refresh" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parser().parse_args(["t.json", "--frames_importance_rate", "0.25"])
    assert "--frames_importance_rate needs --frames_importance_refresh" in capsys.readouterr().err
    for n in ("0", "-3"):
        with pytest.raises(SystemExit):
            train.parser().parse_args(["t.json", "--frames_crops", "importance", "--frames_importance_refresh", n])
        assert "--frames_importance_refresh" in capsys.readouterr().err
    for a in ("0", "1.5", "nan"):
        with pytest.raises(SystemExit):
            train.parser().parse_args(["t.json", "--frames_crops", "importance", "--frames_importance_refresh", "2", "--frames_importance_rate", a])
        assert "--frames_importance_rate" in capsys.readouterr().err
    text = train.parser().format_help()
    assert "a choice, not a measured optimum" in " ".join(text.split()).split("--frames_importance_rate")[-1]


# ---------------------------------------------------------------------------------------------------- Program.step_tail_ops
class _Graph:
    """The launch lists of engine.Graph; run() calls the launches with a stream of None."""

    def __init__(self, log):
        def op(name):
            def run(stream):
                log.append(name)
            return run
        self.pack_ops, self.fwd_ops, self.bwd_ops = [op("pack")], [op("fwd0"), op("fwd1")], [op("bwd0"), op("bwd1")]

    def run(self, ops, stream=None):
        for f in ops:
            f(stream)


def _program(log):
    from deepdenoiser_amd.program import Program

    class Recorded(Program):
        def zero_grads(self):
            log.append("zero")

        def adam(self, **kwargs):
            log.append("adam")

    p = Recorded.__new__(Recorded)
    p.g, p.label_ops, p.masked, p.mask_reduce, p.grad_hook, p.loss_buf = _Graph(log), [], False, None, None, "loss"
    p.step_tail_ops, p.step_tail_frozen = [], False
    return p


def test_train_step_runs_the_tail_between_forward_and_backward():
    log = []
    p = _program(log)
    assert p.train_step() == "loss"
    assert log == ["zero", "pack", "fwd0", "fwd1", "bwd0", "bwd1", "adam"]      # an empty list: the step as it always was
    del log[:]

    def tail(stream):
        log.append("tail")
    p.add_step_tail_op(tail)
    assert p.step_tail_ops == [tail] and tail.tag == "pointwise"
    p.forward()
    assert log == ["pack", "fwd0", "fwd1"]                      # forward() does not score a batch
    del log[:]
    p.train_step()
    assert log == ["zero", "pack", "fwd0", "fwd1", "tail", "bwd0", "bwd1", "adam"]
    assert log.count("tail") == 1


def test_trainer_puts_the_tail_behind_the_forward_of_segment_0_and_freezes_it():
    from types import SimpleNamespace
    from deepdenoiser_amd.training import Trainer
    for n_tail in (0, 1):
        log = []
        p = _program(log)

        def tail(stream):
            log.append("tail")
        if n_tail:
            p.add_step_tail_op(tail, "importance_update")
        t = Trainer.__new__(Trainer)
        t.program, t.n_buckets, t._reduce_masks = p, 1, False
        t.arch = SimpleNamespace(params=SimpleNamespace(params=[], values=SimpleNamespace(numel=lambda: 4)))
        t._build_segments()
        assert len(t._segments) == 1
        ops, _ = t._segments[0]
        p.g.run(ops)
        assert log == ["pack", "fwd0", "fwd1"] + ["tail"] * n_tail + ["bwd0", "bwd1"]
        with pytest.raises(RuntimeError, match="after the trainer had built its segments"):
            p.add_step_tail_op(tail)
        assert len(p.step_tail_ops) == n_tail


def test_a_real_program_on_the_cpu_device_wires_the_tail(lib):
    """The cfg-2 training program built on the CPU device (as tests/test_bind_at_finalize.py builds it): its launch lists are replaced by
    recording closures -- nothing can be launched without a GPU -- and the step runs through Program and Trainer as it is."""
    from deepdenoiser_amd import configs
    from deepdenoiser_amd.architecture import Architecture
    from deepdenoiser_amd.training import Trainer
    arch = Architecture(configs.cfg2_unet_kpcn(), device="cpu", dtype="bf16", seed=2)
    trainer = Trainer(arch, configs.bench_training(), 2, 64, 64, use_graph=False)
    prog = trainer.program
    assert prog.step_tail_ops == [] and prog.step_tail_frozen is False      # nothing attached: the lists of a step are what they were
    log = []

    def recorder(name):
        def run(stream):
            log.append(name)
        return run
    n_fwd, n_bwd = len(prog.g.fwd_ops), len(prog.g.bwd_ops)
    assert n_fwd > 0 and n_bwd > 0
    prog.g.pack_ops[:] = [recorder("pack")]
    prog.label_ops[:] = [recorder("label")]
    prog.g.fwd_ops[:] = [recorder("fwd")] * n_fwd
    prog.g.bwd_ops[:] = [recorder("bwd")] * n_bwd
    prog.adam = lambda **kwargs: log.append("adam")
    prog.g.stream_ptr = lambda: None                            # (no device: there is no stream to ask for)
    prog.add_step_tail_op(recorder("tail"), "importance_update")
    assert prog.step_tail_ops[0].tag == "importance_update"
    prog.forward()
    assert log == ["pack", "label"] + ["fwd"] * n_fwd
    del log[:]
    prog.train_step()
    assert log == ["pack", "label"] + ["fwd"] * n_fwd + ["tail"] + ["bwd"] * n_bwd + ["adam"]
    del log[:]
    trainer.step()
    assert log == ["pack", "label"] + ["fwd"] * n_fwd + ["tail"] + ["bwd"] * n_bwd + ["adam"]
    with pytest.raises(RuntimeError, match="after the trainer had built its segments"):
        prog.add_step_tail_op(recorder("late"))
    prog.step_tail_ops.append(recorder("late"))                 # past the method: the next step notices
    with pytest.raises(RuntimeError, match="changed after the trainer had built its segments"):
        trainer.step()
