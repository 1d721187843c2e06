"""-m gpu: gradient clipping by global norm with per-variable norms (csrc/dd_grad_norm.hip, deepdenoiser_amd/grad_clip.py).

Op level: the segmented reduction against the float64 restatement tests/grad_clip_ref.py (sums at 1e-9 relative: a double sum of at most 2^21
terms is off by at most 2^21 * 2^-53 = 2.3e-10 in any order; the float grad_norm and coef at 1e-6), its run-to-run bytes, the non-finite rule, the
clipped Adam launches against oracle.tf_ops.adam_step at the gates of test_gpu_ops.py::test_adam_tf_form (2e-6 abs on p, 1e-6 on m, 1e-4 on v)
and, at coef == 1, bit for bit against the unclipped launches.  Model level: the tiny U-Net of tests/test_gpu_loss_scale.py in f32; the
dynamic loss scale with clipping (no host synchronisation); two ranks on one GPU; the command line."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (the child process of the bit-identity test runs this file as a script)
    sys.path.insert(0, ROOT)

import grad_clip_ref as R                                         # noqa: E402
from deepdenoiser_amd import _lib as L                            # noqa: E402
from deepdenoiser_amd import configs, summaries                   # noqa: E402
from deepdenoiser_amd import grad_clip as GC                      # noqa: E402
from deepdenoiser_amd import loss_scale as LS                     # noqa: E402
from gpu_util import check, gate                                  # noqa: E402
from oracle import tf_ops as T                                    # noqa: E402
from test_gpu_loss_scale import B, H, W, _batch, _tiny            # noqa: E402

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
SUM_GATE, FLOAT_GATE = 1e-9, 1e-6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scaler(scale):
    return LS.LossScaler(LS.parse({"init": scale, "growth_interval": 1000}, "f16"), "cuda")


# ---------------------------------------------------------------------------------------------------------------- 1. reduction vs reference
@pytest.fixture(scope="module")
def arena():
    """The issue's sizes in one arena with ParamStore's alignment, NaN in every padding word of both arenas; host copies and device tensors,
    shared and left unchanged."""
    _need_gpu()
    params, total = R.layout()
    g, w = R.arenas(params, total)
    return {"params": params, "total": total, "g": g, "w": w, "gd": torch.from_numpy(g).cuda(), "wd": torch.from_numpy(w).cuda()}


def _rel(got, want):
    return abs(got - want) / want if want != 0 else (0.0 if got == 0 else INF)


def _compare(name, rep, ref):
    worst_g = max(_rel(rep["variables"][n]["grad_sq"], ref["variables"][n]["grad_sq"]) for n in ref["variables"])
    worst_w = max(_rel(rep["variables"][n]["weight_sq"], ref["variables"][n]["weight_sq"]) for n in ref["variables"])
    total = 0.0
    for n in ref["variables"]:      # (variable order, like the device)
        total += rep["variables"][n]["grad_sq"]
    print("%s: worst per-variable rel. error grad_sq %.3e weight_sq %.3e, total %.3e" % (name, worst_g, worst_w, _rel(total, ref["grad_sq_total"])))
    gate(name + ": per-variable grad_sq (worst rel)", worst_g, SUM_GATE)
    gate(name + ": per-variable weight_sq (worst rel)", worst_w, SUM_GATE)
    gate(name + ": total grad_sq (rel)", _rel(total, ref["grad_sq_total"]), SUM_GATE)
    assert [rep["variables"][n]["nonfinite"] for n in ref["variables"]] == [ref["variables"][n]["nonfinite"] for n in ref["variables"]]
    assert rep["nonfinite_total"] == ref["nonfinite_total"] and rep["nonfinite_variables"] == ref["nonfinite_variables"]


@pytest.mark.parametrize("clip", ["below", "above", "zero"])
@pytest.mark.parametrize("mode", ["by_value", "scaler"])
def test_reduction_matches_the_reference(arena, mode, clip):
    a = arena
    gs = 0.5 if mode == "by_value" else 0.5 / 4096.0
    norm = R.reference(a["params"], a["g"], a["w"], gs, None)["grad_norm"]
    assert 0 < norm < 3.4e38 / 1.25
    clip_norm = {"below": float(np.float32(0.25 * norm)), "above": float(np.float32(1.25 * norm)), "zero": None}[clip]
    ref = R.reference(a["params"], a["g"], a["w"], gs, clip_norm)
    clipper = GC.GradientClipper(a["params"], a["gd"], a["wd"], clip_norm)
    sc = _scaler(4096.0) if mode == "scaler" else None
    clipper.measure(0.5, _stream(), scaler_ptr=sc.ptr if sc else None)
    rep = clipper.report()
    name = "grad norms %s clip %s" % (mode, clip)
    _compare(name, rep, ref)
    print("%s: grad_norm %.9g (ref %.9g) coef %.9g (ref %.9g)" % (name, rep["grad_norm"], ref["grad_norm"], rep["coef"], ref["coef"]))
    assert rep["grad_factor"] == gs
    gate(name + ": grad_norm (rel)", _rel(rep["grad_norm"], ref["grad_norm"]), FLOAT_GATE)
    gate(name + ": coef (rel)", _rel(rep["coef"], ref["coef"]), FLOAT_GATE)
    if clip == "below":
        assert rep["coef"] < 0.26
    else:
        assert rep["coef"] == 1.0      # exactly: the clipped Adam launch is then the unclipped one, bit for bit
    one = "v0_1"                       # the one-element variable whose gradient is a denormal
    assert rep["variables"][one]["grad_sq"] > 0 and ref["variables"][one]["grad_sq"] < 1e-80
    if sc is not None:
        assert sc.state() == {"scale": 4096.0, "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 0}      # read only
    assert torch.equal(a["gd"].cpu().view(torch.int32), torch.from_numpy(a["g"]).view(torch.int32))                        # so are the arenas


# ---------------------------------------------------------------------------------------------------------------- 2. run to run
def test_same_input_twice_gives_the_same_bytes(arena):
    a = arena
    clipper = GC.GradientClipper(a["params"], a["gd"], a["wd"], 1.0)
    clipper.measure(0.5, _stream())
    first = clipper.tables() + (clipper._partials.cpu().numpy().tobytes(),)
    clipper._var_norms.fill_(-1), clipper._clip.fill_(-1), clipper._partials.fill_(-1)      # every word is rewritten by a call
    clipper.measure(0.5, _stream())
    second = clipper.tables() + (clipper._partials.cpu().numpy().tobytes(),)
    other = GC.GradientClipper(a["params"], a["gd"].clone(), a["wd"].clone(), 1.0)            # other allocations, the same values
    other.measure(0.5, _stream())
    third = other.tables() + (other._partials.cpu().numpy().tobytes(),)
    assert first == second == third
    assert len(first[0]) == 24 * len(a["params"]) and len(first[1]) == 20


# ---------------------------------------------------------------------------------------------------------------- 3. non-finite gradients
def test_nonfinite_elements_are_counted_and_left_out(arena):
    a = arena
    off = {size: o for _, o, size in reversed(a["params"])}      # the first variable of every size
    g = a["g"].copy()
    g[off[5] + 2] = INF
    g[off[8195] + 4100] = NAN
    g[off[4097] + 4096] = -INF                                    # the last element of a 4097-element variable: the element tail of its second chunk
    ref = R.reference(a["params"], g, a["w"], 0.5, 1e-3)
    assert ref["nonfinite_total"] == 3 and ref["nonfinite_variables"] == 3
    clipper = GC.GradientClipper(a["params"], torch.from_numpy(g).cuda(), a["wd"], 1e-3)
    clipper.measure(0.5, _stream())
    rep = clipper.report()
    _compare("grad norms with inf / NaN", rep, ref)               # (the counts exactly, the sums as computed without those elements)
    names = {size: n for n, _, size in reversed(a["params"])}
    assert [rep["variables"][names[s]]["nonfinite"] for s in (5, 8195, 4097)] == [1, 1, 1]
    assert sum(v["nonfinite"] for v in rep["variables"].values()) == 3
    assert rep["coef"] == 1.0 and rep["grad_norm"] == INF and rep["nonfinite_variables"] == 3 and rep["nonfinite_total"] == 3


# ---------------------------------------------------------------------------------------------------------------- 4. the clipped Adam launches
def _clip_record(coef):
    rec = L.GradClip(grad_norm=1.0, coef=coef, grad_factor=0.5, nonfinite_variables=0, nonfinite_total=0)
    return torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.int32).copy()).cuda()


def _draw(gen, n):
    gr = torch.randn(n, generator=gen) * torch.exp(3 * torch.randn(n, generator=gen))      # gradients over many magnitudes (test_adam_tf_form)
    gr[::17] = 0.0
    return gr


@pytest.mark.parametrize("entry", ["static", "scaled"])
def test_clipped_adam_tf_form(entry):
    _need_gpu()
    lib = L.load()
    gen = torch.Generator().manual_seed(5)
    n, S = 10007, 512.0
    coef = float(np.float32(0.37))
    p0 = torch.randn(n, generator=gen)
    p = p0.clone().cuda(); m = torch.zeros(n).cuda(); v = torch.zeros(n).cuda()
    po = [p0.double().clone()]; mo = [torch.zeros(n, dtype=torch.float64)]; vo = [torch.zeros(n, dtype=torch.float64)]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    clip = _clip_record(coef)
    sc = _scaler(S)
    for step in range(1, 5):
        gr = _draw(gen, n)
        if entry == "static":
            lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
            L.check(lib.dd_adam_step_clipped(p.data_ptr(), gr.cuda().data_ptr(), m.data_ptr(), v.data_ptr(), n, lr_t, b1, b2, eps, 0.5, clip.data_ptr(),
                                             _stream()))
        else:
            g = (gr * S).cuda()                                     # what a backward under the loss scale S leaves in the arena (x 512: exact)
            L.check(lib.dd_grads_nonfinite(g.data_ptr(), n, sc.ptr, _stream()))
            L.check(lib.dd_adam_step_scaled_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, 0.5, sc.ptr,
                                                    clip.data_ptr(), _stream()))
            L.check(lib.dd_scaler_update(sc.ptr, 2.0, 0.5, 1000, 1.0, 2.0 ** 24, _stream()))
        T.adam_step(po, [coef * 0.5 * gr.double()], mo, vo, step, lr)
        torch.cuda.synchronize()
        err = float((p.double().cpu() - po[0]).abs().max())
        print("%s step %d: max |p - oracle| %.3e" % (entry, step, err))
        gate("clipped adam (%s) p, step %d (abs)" % (entry, step), err, 2e-6)
        check("clipped adam (%s) m, step %d" % (entry, step), m.cpu(), mo[0], 1e-6)
        check("clipped adam (%s) v, step %d" % (entry, step), v.cpu(), vo[0], 1e-4)
    assert float((p.cpu() - p0).abs().max()) > 1e-4
    if entry == "scaled":
        assert sc.state()["adam_t"] == 4


def test_clipped_adam_at_coef_one_is_the_unclipped_launch_bit_for_bit():
    _need_gpu()
    lib = L.load()
    gen = torch.Generator().manual_seed(6)
    n, S = 10007, 512.0
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    one = _clip_record(1.0)
    p0 = torch.randn(n, generator=gen)
    state = {k: [p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()] for k in ("plain", "clipped", "scaled", "scaled_clipped")}
    sa, sb = _scaler(S), _scaler(S)
    for step in range(1, 5):
        gr = _draw(gen, n).cuda()
        lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        x = state["plain"]
        L.check(lib.dd_adam_step(x[0].data_ptr(), gr.data_ptr(), x[1].data_ptr(), x[2].data_ptr(), n, lr_t, b1, b2, eps, 0.5, _stream()))
        x = state["clipped"]
        L.check(lib.dd_adam_step_clipped(x[0].data_ptr(), gr.data_ptr(), x[1].data_ptr(), x[2].data_ptr(), n, lr_t, b1, b2, eps, 0.5, one.data_ptr(),
                                         _stream()))
        gS = gr * S
        x = state["scaled"]
        L.check(lib.dd_adam_step_scaled(x[0].data_ptr(), gS.data_ptr(), x[1].data_ptr(), x[2].data_ptr(), n, lr, b1, b2, eps, 0.5, sa.ptr, _stream()))
        L.check(lib.dd_scaler_update(sa.ptr, 2.0, 0.5, 1000, 1.0, 2.0 ** 24, _stream()))
        x = state["scaled_clipped"]
        L.check(lib.dd_adam_step_scaled_clipped(x[0].data_ptr(), gS.data_ptr(), x[1].data_ptr(), x[2].data_ptr(), n, lr, b1, b2, eps, 0.5, sb.ptr,
                                                one.data_ptr(), _stream()))
        L.check(lib.dd_scaler_update(sb.ptr, 2.0, 0.5, 1000, 1.0, 2.0 ** 24, _stream()))
        torch.cuda.synchronize()
        for a, b in (("plain", "clipped"), ("scaled", "scaled_clipped")):
            for i, what in enumerate("pmv"):
                assert torch.equal(state[a][i], state[b][i]), (step, a, b, what)
    assert float((state["clipped"][0].cpu() - p0).abs().max()) > 1e-4 and sb.state()["adam_t"] == 4


def test_clipped_adam_writes_nothing_on_a_skipped_step():
    _need_gpu()
    lib = L.load()
    gen = torch.Generator().manual_seed(7)
    n = 10007
    p = torch.randn(n, generator=gen).cuda(); m = torch.full((n,), 0.25).cuda(); v = torch.full((n,), 0.5).cuda()
    before = (p.clone(), m.clone(), v.clone())
    g = torch.randn(n, generator=gen)
    g[n // 2] = NAN
    g = g.cuda()
    sc = _scaler(512.0)
    clip = _clip_record(0.5)
    L.check(lib.dd_grads_nonfinite(g.data_ptr(), n, sc.ptr, _stream()))
    assert sc.state()["found_nonfinite"] == 1
    L.check(lib.dd_adam_step_scaled_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.5, sc.ptr,
                                            clip.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for a, b in zip(before, (p, m, v)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 5. model level
def _arch(dtype="f32", **kw):
    from deepdenoiser_amd.architecture import Architecture
    aj, tj = _tiny()
    return Architecture(aj, device="cuda:0", dtype=dtype, seed=2, **kw), tj      # (the seed fixes the weights: every model here starts equal)


def _program(**kw):
    arch, tj = _arch(**kw)
    prog = arch.program(B, H, W, training_json=tj)
    prog.set_inputs(*_batch(arch))
    return arch, tj, prog


def _first_norm():
    arch, tj, prog = _program(clip_norm=None, track_gradient_norms=True)
    prog.train_step()
    rep = prog.gradient_report()
    assert rep["coef"] == 1.0 and 0 < rep["grad_norm"] < INF and rep["nonfinite_total"] == 0
    return rep["grad_norm"]


def test_model_without_either_has_no_clipper():
    _need_gpu()
    arch, tj, prog = _program()
    assert prog.clipper is None and arch.grad_clipper is None and prog.gradient_report() is None


def test_model_clipped_steps_follow_tf_adam_on_the_clipped_gradients():
    _need_gpu()
    norm0 = _first_norm()
    arch, tj, prog = _program(clip_norm=0.5 * norm0)
    ps, lr = arch.params, tj["learning_rate"]
    layout = [(q.name, q.offset, q.size) for q in ps.params]
    assert len(layout) > 8 and prog.clipper is arch.grad_clipper
    po, mo, vo = [ps.values.double().cpu()], [ps.m.double().cpu()], [ps.v.double().cpu()]
    for step in range(1, 4):
        w_before = ps.values.cpu().numpy()
        prog.train_step()
        rep = prog.gradient_report()
        g = ps.grads.cpu()                                          # the device's own gradients of this step (f32: loss scale 1)
        assert prog.loss_scale == 1.0 and rep["grad_factor"] == 1.0
        print("step %d: grad_norm %.6g coef %.6g" % (step, rep["grad_norm"], rep["coef"]))
        assert rep["coef"] < 1.0 and rep["nonfinite_total"] == 0
        if step == 1:
            gate("model: first clipped norm vs the tracked run (rel; fp32 atomics order)", _rel(rep["grad_norm"], norm0), 1e-4)
            assert abs(rep["coef"] - 0.5) < 1e-3
        ref = R.reference(layout, g.numpy(), w_before, 1.0, 0.5 * norm0)
        worst = max(max(_rel(rep["variables"][n]["grad_norm"], ref["variables"][n]["grad_norm"]),
                        _rel(rep["variables"][n]["weight_norm"], ref["variables"][n]["weight_norm"])) for n, _, _ in layout)
        gate("model: per-variable norms vs the arena on the host, step %d (worst rel)" % step, worst, 1e-5)
        gate("model: grad_norm vs host, step %d (rel)" % step, _rel(rep["grad_norm"], ref["grad_norm"]), 1e-5)
        gate("model: coef vs host, step %d (rel)" % step, _rel(rep["coef"], ref["coef"]), 1e-5)
        T.adam_step(po, [rep["coef"] * g.double()], mo, vo, step, lr)
        gate("model: clipped adam p, step %d (abs)" % step, float((ps.values.double().cpu() - po[0]).abs().max()), 2e-6)
        check("model: clipped adam m, step %d" % step, ps.m.cpu(), mo[0], 1e-6)
        check("model: clipped adam v, step %d" % step, ps.v.cpu(), vo[0], 1e-4)
    assert arch.adam_step == 3


def _three_steps(**kw):
    arch, tj, prog = _program(**kw)
    for _ in range(3):
        prog.train_step()
    torch.cuda.synchronize()
    return arch.params.values.cpu().clone(), prog


def test_model_clip_norm_far_above_the_norm_changes_no_bit(tmp_path):
    """DD_DETERMINISTIC=1 (read once per process: a child) makes the runs' gradients bit-equal; with clip_norm at 100 x the norm coef is exactly 1
    and the clipped Adam launch is the unclipped one, so three steps end in the weights of a run with clip_norm=None, bit for bit."""
    _need_gpu()
    out = str(tmp_path / "runs.pt")
    env = dict(os.environ, DD_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child failed\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:])
    runs = torch.load(out)
    assert runs["coef"] == 1.0 and 0 < runs["norm_after"] < 100 * runs["norm0"]
    assert float((runs["plain"] - runs["initial"]).abs().max()) > 1e-5
    assert torch.equal(runs["plain"], runs["far"])
    assert not torch.equal(runs["plain"], runs["half"])      # (and the comparison can tell: half the norm moves the weights elsewhere)


# ---------------------------------------------------------------------------------------------------------------- 6. dynamic scale + clipping
STEPS, INIT = 60, 2.0 ** 40


def test_dynamic_scale_with_clipping():
    """fp16, an initial scale of 2^40 that overflows until it has backed off, clip_norm set: the skip is the scaler's as before, a skipped step
    writes nothing, and the step makes no host synchronisation."""
    _need_gpu()
    from deepdenoiser_amd.training import Trainer
    arch, tj = _arch(dtype="f16", loss_scale={"init": INIT}, clip_norm=1e-6)
    trainer = Trainer(arch, tj, B, H, W)
    trainer.program.set_inputs(*_batch(arch))
    ps = arch.params
    ps.m.fill_(0.25), ps.v.fill_(0.5)
    before = (ps.values.clone(), ps.m.clone(), ps.v.clone())
    trainer.step()
    rep = trainer.program.gradient_report()
    assert rep["coef"] == 1.0 and rep["grad_norm"] == INF and rep["nonfinite_variables"] >= 1      # which variables overflowed is now on record
    assert rep["nonfinite_total"] == int((~torch.isfinite(ps.grads)).sum())
    for a, b in zip(before, (ps.values, ps.m, ps.v)):
        assert torch.equal(a, b), "step 1 (scale 2^40) must have been skipped without a write"
    for _ in range(STEPS - 1):
        trainer.step()
    assert trainer._graphs is not None
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            trainer.step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    st = trainer.program.scaler.state()
    rep = trainer.program.gradient_report()
    print("state after %d steps: %s; grad_norm %.6g coef %.6g" % (STEPS + 3, st, rep["grad_norm"], rep["coef"]))
    assert st["adam_t"] + st["skipped_total"] == STEPS + 3
    assert st["skipped_total"] >= 1 and st["adam_t"] >= 1 and st["scale"] == INIT * 0.5 ** st["skipped_total"]
    assert rep["grad_factor"] == np.float32(1.0) / np.float32(st["scale"])
    assert rep["nonfinite_total"] == 0 and 0 < rep["coef"] < 1.0 and rep["coef"] == pytest.approx(1e-6 / rep["grad_norm"], rel=1e-5)
    assert bool(torch.isfinite(ps.values).all()) and not torch.equal(ps.values, before[0])


# ---------------------------------------------------------------------------------------------------------------- 7. two ranks on one GPU
def _rank(rank, world, port, out):
    import torch.distributed as dist
    from deepdenoiser_amd.training import Trainer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        arch, tj = _arch(clip_norm=1e-4)
        trainer = Trainer(arch, tj, B // world, H, W, world_size=world, n_buckets=3)
        feats, labels = _batch(arch)
        shard = slice(rank * (B // world), (rank + 1) * (B // world))
        trainer.program.set_inputs({k: v[shard] for k, v in feats.items()}, {k: v[shard] for k, v in labels.items()})
        records = []
        for _ in range(3):
            trainer.step()
            records.append(trainer.program.clipper.tables())
        torch.cuda.synchronize()
        torch.save({"records": records, "report": trainer.program.gradient_report(), "values": arch.params.values.cpu().clone()}, "%s.%d" % (out, rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_agree_to_the_byte(tmp_path):
    _need_gpu()
    import torch.multiprocessing as mp
    from test_gpu_distributed import _free_port
    out = str(tmp_path / "rank")
    mp.spawn(_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert r0["records"] == r1["records"] and len(r0["records"]) == 3      # per-variable tables and clip records (coef, grad_norm) of every step
    assert r0["report"]["coef"] == r1["report"]["coef"] < 1.0 and r0["report"]["grad_norm"] == r1["report"]["grad_norm"] > 1e-4
    assert r0["report"]["grad_factor"] == 0.5                               # the mean over the two ranks
    assert torch.equal(r0["values"], r1["values"]), "replicas diverged"


# ---------------------------------------------------------------------------------------------------------------- 8. the command line
def test_cli_writes_the_gradient_scalars(tmp_path):
    _need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    from test_gpu_end_to_end import SPP, T as TILE, _write_dataset
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE")
    aj["model_directory"] = "model"
    tj = configs.training(learning_rate=2e-3, batch_size=4)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "data", "modes": ["training"], "number_of_source_index_tuples": 1,
               "gradient_clip_norm": 1e-3})
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    json.dump(tj, open(tmp_path / "training.json", "w"))
    arch = Architecture(aj, device="cuda")
    base = str(tmp_path / "data")
    _write_dataset(base, arch)
    json.dump({"tiles_height_width": TILE, "number_of_sources_per_example": 1, "source_samples_per_pixel_list": [SPP]}, open(os.path.join(base, "training.json"), "w"))
    arch.program(4, TILE, TILE, training_json=tj)
    names = [p.name for p in arch.params.params]
    assert len(names) > 8
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "deepdenoiser_amd.train", str(tmp_path / "training.json"), "--train_epochs", "1", "--dtype", "f32",
                        "--clip_norm", "0.001", "--gradient_norms", "--summary_steps", "1"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "epoch 1: global_step 2" in p.stdout, p.stdout
    files = summaries.event_files(str(tmp_path / "model"))
    assert len(files) == 1
    scalars = summaries.read_scalars(files[0])
    for step in (1, 2):
        got = {tag: value for s, tag, value in scalars if s == step}
        assert 0 < got["gradient_norm"] < INF and got["gradient_clip_coefficient"] == pytest.approx(1e-3 / got["gradient_norm"], rel=1e-5)
        assert got["gradient_clip_coefficient"] < 1.0 and got["gradient_nonfinite_variables"] == 0
        assert sorted(t for t in got if t.startswith("gradient_norm/")) == sorted("gradient_norm/" + n for n in names)
        assert sorted(t for t in got if t.startswith("weight_norm/")) == sorted("weight_norm/" + n for n in names)
        total = math.sqrt(sum(got["gradient_norm/" + n] ** 2 for n in names))
        assert total == pytest.approx(got["gradient_norm"], rel=1e-5)
        assert "loss" in got and all(got["weight_norm/" + n] >= 0 for n in names)


if __name__ == "__main__":      # the child of test_model_clip_norm_far_above_the_norm_changes_no_bit
    initial = _program()[0].params.values.cpu().clone()
    norm0 = _first_norm()
    plain, _ = _three_steps()
    far, prog = _three_steps(clip_norm=100.0 * norm0)
    rep = prog.gradient_report()
    half, _ = _three_steps(clip_norm=0.5 * norm0)
    torch.save({"initial": initial, "norm0": norm0, "plain": plain, "far": far, "half": half, "coef": rep["coef"], "norm_after": rep["grad_norm"]}, sys.argv[1])
