"""-m gpu: dynamic loss scaling on the device (csrc/dd_loss_scale.hip, deepdenoiser_amd/loss_scale.py).

Op level: the non-finite scan (exact), the guarded Adam update against oracle.tf_ops.adam_step at the gates of test_gpu_ops.py::test_adam_tf_form
(2e-6 abs on p, 1e-6 rel-L2 on m, 1e-4 on v), the record update against test_loss_scale.scaler_update_ref (exact: every factor is a power of
two), and the *_dscale loss launches against their by-value twins (bit-identical dpred).  Model level: a tiny fp16 U-Net whose initial scale of
2^40 overflows -- inf / NaN as ordinary IEEE arithmetic, nothing faults -- until the scale has backed off; the static skip path; no host
synchronisation in the dynamic step; the checkpoint round trip."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (the child process of the static-vs-dynamic test runs this file as a script)
    sys.path.insert(0, ROOT)

import loss_ref as R                                              # noqa: E402
from deepdenoiser_amd import _lib as L                            # noqa: E402
from deepdenoiser_amd import configs, tf_checkpoint               # noqa: E402
from deepdenoiser_amd import loss_scale as LS                     # noqa: E402
from deepdenoiser_amd.naming import Naming                        # noqa: E402
from gpu_util import check, gate                                  # noqa: E402
from oracle import tf_ops as T                                    # noqa: E402
from test_loss_scale import scaler_update_ref                     # noqa: E402

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scaler(scale=1.0, **settings):
    return LS.LossScaler(LS.parse(dict(settings, init=scale), "f16"), "cuda")


# ---------------------------------------------------------------------------------------------------------------- 1. the non-finite scan
def _finite(n):
    """+-0, denormals, +-3.4e38 and ordinary values, in every position of a 16-byte vector over the length of the tensor"""
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-40, 3.4e38, -3.4e38, 1.0, -2.5, 1e-38], dtype=torch.float32)
    x = special.repeat(n // len(special) + 1)[:n].clone()
    noise = torch.randn(n, generator=torch.Generator().manual_seed(n))
    return torch.where(torch.arange(n) % 3 == 2, noise, x)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 10007, 2097152 + 5])
def test_nonfinite_scan(n):
    _need_gpu()
    lib = L.load()
    base = _finite(n)
    assert bool(torch.isfinite(base).all()) and (n < 9 or (bool((base == 0).any()) and float(base.abs().max()) == pytest.approx(3.4e38)
                                                           and bool(((base != 0) & (base.abs() < 1.1e-38)).any())))
    base = base.cuda()
    sc = _scaler()

    def flag(x):
        L.check(lib.dd_grads_nonfinite(x.data_ptr(), n, sc.ptr, _stream()))
        return sc.state()["found_nonfinite"]

    assert flag(base) == 0
    last4 = ((n - 1) // 4) * 4                                      # the last multiple of 4 (first element of the tail or of the last vector)
    for pos in sorted({0, n - 1, last4, min(last4 + 1, n - 1)}):
        for bad in (INF, -INF, NAN):
            x = base.clone()
            x[pos] = bad
            assert flag(x) == 1, (pos, bad)
            assert flag(base) == 1, "a set flag must stay set until dd_scaler_update"
            sc.set_state({"found_nonfinite": 0})
            assert flag(base) == 0
    assert sc.state() == {"scale": 1.0, "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 0}      # nothing else was written


# ---------------------------------------------------------------------------------------------------------------- 2. the guarded Adam update
def test_adam_scaled_tf_form_and_skip():
    _need_gpu()
    lib = L.load()
    gen = torch.Generator().manual_seed(5)
    n, S = 10007, 512.0
    p0 = torch.randn(n, generator=gen)
    p = p0.clone().cuda(); m = torch.zeros(n).cuda(); v = torch.zeros(n).cuda()
    po = [p0.double().clone()]; mo = [torch.zeros(n, dtype=torch.float64)]; vo = [torch.zeros(n, dtype=torch.float64)]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    settings = dict(growth=2.0, backoff=0.5, growth_interval=1000, min_scale=1.0, max_scale=2.0 ** 24)
    sc = _scaler(S, growth_interval=1000)
    want = {"scale": S, "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 0}

    def device_step(gr):
        g = (gr * S).cuda()                                         # what a backward under the loss scale S leaves in the arena (x 512: exact)
        L.check(lib.dd_grads_nonfinite(g.data_ptr(), n, sc.ptr, _stream()))
        L.check(lib.dd_adam_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, 0.5, sc.ptr, _stream()))
        after_adam = (p.clone(), m.clone(), v.clone())
        L.check(lib.dd_scaler_update(sc.ptr, settings["growth"], settings["backoff"], settings["growth_interval"], settings["min_scale"],
                                     settings["max_scale"], _stream()))
        torch.cuda.synchronize()
        return after_adam

    for step in range(1, 5):
        gr = torch.randn(n, generator=gen) * torch.exp(3 * torch.randn(n, generator=gen))      # gradients over many magnitudes
        gr[::17] = 0.0
        device_step(gr)
        T.adam_step(po, [0.5 * gr.double()], mo, vo, step, lr)
        want = scaler_update_ref(want, **settings)
        err = float((p.double().cpu() - po[0]).abs().max())
        print("step %d: max |p - oracle| %.3e" % (step, err))
        gate("scaled adam p, step %d (abs)" % step, err, 2e-6)
        check("scaled adam m, step %d" % step, m.cpu(), mo[0], 1e-6)
        check("scaled adam v, step %d" % step, v.cpu(), vo[0], 1e-4)
        assert sc.state() == want and want["adam_t"] == step
        if step == 2:      # one call with a NaN among the gradients: nothing is written, the step does not count, the scale backs off
            before = (p.clone(), m.clone(), v.clone())
            bad = torch.randn(n, generator=gen)
            bad[n // 2] = NAN
            after = device_step(bad)
            for a, b in zip(before, after):
                assert torch.equal(a, b)
            for a, b in zip(before, (p, m, v)):
                assert torch.equal(a, b)
            want = scaler_update_ref(dict(want, found_nonfinite=1), **settings)
            assert sc.state() == want and want["adam_t"] == 2 and want["skipped_total"] == 1 and want["scale"] == S / 2
            S = S / 2


# ---------------------------------------------------------------------------------------------------------------- 3. the update rule
def test_update_rule_follows_the_restatement():
    _need_gpu()
    lib = L.load()
    settings = dict(growth=2.0, backoff=0.5, growth_interval=3, min_scale=2.0, max_scale=16.0)
    # growth at 3 and 6 good steps, the max clamp at 9, four backoffs down to the min clamp, a good step after it
    pattern = [False] * 9 + [True] * 4 + [False]
    sc = _scaler(4.0, **settings)
    good, bad = torch.ones(4, device="cuda"), torch.tensor([1.0, -INF, 0.0, 2.0], device="cuda")
    want = {"scale": 4.0, "good_steps": 0, "found_nonfinite": 0, "adam_t": 0, "skipped_total": 0}
    scales = []
    for step, overflow in enumerate(pattern):
        L.check(lib.dd_grads_nonfinite((bad if overflow else good).data_ptr(), 4, sc.ptr, _stream()))
        assert sc.state()["found_nonfinite"] == int(overflow)
        L.check(lib.dd_scaler_update(sc.ptr, settings["growth"], settings["backoff"], settings["growth_interval"], settings["min_scale"],
                                     settings["max_scale"], _stream()))
        want = scaler_update_ref(dict(want, found_nonfinite=int(overflow)), **settings)
        assert sc.state() == want, (step, sc.state(), want)
        scales.append(want["scale"])
    assert scales == [4.0, 4.0, 8.0, 8.0, 8.0, 16.0, 16.0, 16.0, 16.0, 8.0, 4.0, 2.0, 2.0, 2.0]      # (by hand: growth, max clamp, backoff, min clamp)
    assert want["adam_t"] == 10 and want["skipped_total"] == 4


# ---------------------------------------------------------------------------------------------------------------- 4. device-scale loss launches
# features-only (flat-stream kernel), a combined triple and the image without variation (per-pixel kernel), variation terms (older kernel), the
# fused inverse standardization in both kernels that have it
DSCALE_CASES = [("flat_2_features", 0), ("pixel_combined_image_features", 1), ("older_variation_with_mean", 2), ("flat_fused_log1p", 0),
                ("pixel_fused_next_to_combined", 1)]


@pytest.mark.parametrize("S", [1.0, 4096.0])
@pytest.mark.parametrize("name,path", DSCALE_CASES)
def test_loss_head_dscale_is_bit_identical_to_the_by_value_launch(name, path, S):
    _need_gpu()
    from test_gpu_loss_ops import LOSS_GATE, Dev
    lib = L.load()
    case = R.BY_NAME[name]
    kind = "SMAPE" if "SMAPE" in case["kinds"] else case["kinds"][0]
    x, t = R.make_inputs(case)
    a, b = Dev(case, kind, x, t, grad_scale=S), Dev(case, kind, x, t, grad_scale=S)
    assert a.run() == path
    scale = torch.tensor([S], dtype=torch.float32, device="cuda")
    assert not b.masked
    before = [lib.dd_loss_head_path_count(k) for k in range(3)]
    L.check(lib.dd_loss_head_dscale(C.byref(b.desc), b.B, b.H, b.W, b.loss.data_ptr(), scale.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert [lib.dd_loss_head_path_count(k) - before[k] for k in range(3)] == [int(k == path) for k in range(3)]
    for f in range(len(a.dpred)):
        assert torch.equal(a.dpred[f], b.dpred[f]), (name, f)
    assert any(float(g.abs().max()) > 0 and not bool((g == 12345.0).any()) for g in a.dpred)
    for f in a.pred_inv:
        assert torch.equal(a.pred_inv[f], b.pred_inv[f]), (name, f)
    # the loss sum ends in one fp32 atomic per workgroup (the per-pixel case runs three): compared at the op-level loss gate of test_gpu_loss_ops.py
    ref = R.evaluate(case, kind, x, t)
    gate("loss, dscale vs by value, %s S %g" % (name, S), abs(float(a.loss) - float(b.loss)) / ref["abs_sum"], LOSS_GATE)
    assert scale.item() == S      # read only


@pytest.mark.parametrize("S", [1.0, 4096.0])
def test_msssim_bwd_dscale_is_bit_identical_to_the_by_value_launch(S):
    _need_gpu()
    from test_gpu_msssim import _Op, _op_inputs
    B, H, W = 2, 44, 44
    pred, tgt = _op_inputs(2, B, H, W, 0.1, seed=9)
    a, b = _Op("features_only", pred, tgt, B, H, W), _Op("features_only", pred, tgt, B, H, W)
    scale = torch.tensor([S], dtype=torch.float32, device="cuda")
    a.forward(), a.backward(S), b.forward()
    L.check(L.load().dd_loss_msssim_bwd_dscale(C.byref(b.desc), B, H, W, b.scratch.data_ptr(), scale.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(a.loss, b.loss)
    for f in range(2):
        assert float(a.dpred[f].abs().max()) > 0 and torch.equal(a.dpred[f], b.dpred[f]), f


# ---------------------------------------------------------------------------------------------------------------- 5. model level
B, H, W = 2, 32, 32
STEPS, INIT = 60, 2.0 ** 40


def _tiny():
    """The smallest network the engine accepts in fp16: a 2-level U-Net, 3 x 3 kernel prediction, one noisy pass + the normals."""
    aj = configs.architecture(filters=(16, 24), convs=1, kernel_size=3, flag_mode="NONE",
                              combined={"Emission": {"Color": "Emission", "Direct": "", "Indirect": ""}})
    return aj, configs.bench_training()


def _arch(loss_scale):
    from deepdenoiser_amd.architecture import Architecture
    aj, tj = _tiny()
    return Architecture(aj, device="cuda:0", dtype="f16", seed=2, loss_scale=loss_scale), tj      # (the seed fixes the weights: every model here starts equal)


def _batch(arch):
    g = torch.Generator().manual_seed(0)
    feats = {Naming.source_feature_name(f.name, index=0): torch.randn(B, H, W, f.number_of_channels, generator=g).abs().cuda()
             for f in arch.feature_predictions + arch.auxiliary_features}
    labels = {Naming.target_feature_name(f.name): torch.randn(B, H, W, f.number_of_channels, generator=g).abs().cuda() for f in arch.feature_predictions}
    return feats, labels


def _trainer(loss_scale):
    from deepdenoiser_amd.training import Trainer
    arch, tj = _arch(loss_scale)
    trainer = Trainer(arch, tj, B, H, W)
    trainer.program.set_inputs(*_batch(arch))
    return arch, tj, trainer


def test_static_scale_that_overflows_warns_and_skips():
    """program.Program.adam, static fp16 path: a gradient arena with an inf / NaN -> UserWarning, and values, m, v and arch.adam_step stay."""
    _need_gpu()
    arch, tj = _arch(INIT)
    prog = arch.program(B, H, W, training_json=tj)
    assert prog.scaler is None and prog.loss_scale == INIT
    prog.set_inputs(*_batch(arch))
    ps = arch.params
    ps.m.fill_(0.25), ps.v.fill_(0.5)
    before = (ps.values.clone(), ps.m.clone(), ps.v.clone())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loss = prog.train_step()
        torch.cuda.synchronize()
    assert not bool(torch.isfinite(ps.grads).all()), ("a loss scale of 2^40 did not overflow the fp16 gradients (max |grad| %.3e): this test "
                                                      "checks nothing" % float(ps.grads.abs().max()))
    assert [w for w in caught if issubclass(w.category, UserWarning) and "overflowed" in str(w.message)], [str(w.message) for w in caught]
    assert bool(torch.isfinite(loss).all())
    for a, b in zip(before, (ps.values, ps.m, ps.v)):
        assert torch.equal(a, b)
    assert getattr(arch, "adam_step", 0) == 0 and prog.skipped_steps == 1


@pytest.fixture(scope="module")
def dynamic_run():
    """60 Trainer steps (hipGraph replays from the third) from an initial scale of 2^40; the state is read back ONCE, at the end."""
    _need_gpu()
    arch, tj, trainer = _trainer({"init": INIT})
    values0 = arch.params.values.clone()
    losses, values1 = [], None
    for step in range(STEPS):
        losses.append(trainer.step().clone())
        if step == 0:
            values1 = arch.params.values.clone()
    state = trainer.program.scaler.state()
    return {"arch": arch, "tj": tj, "trainer": trainer, "state": state, "losses": [float(x) for x in losses], "values0": values0, "values1": values1}


def test_dynamic_scale_backs_off_then_trains(dynamic_run):
    r, st = dynamic_run, dynamic_run["state"]
    print("state after %d steps: %s; loss %.5f -> %.5f" % (STEPS, st, r["losses"][0], r["losses"][-1]))
    assert r["trainer"]._graphs is not None
    assert st["skipped_total"] >= 1 and st["adam_t"] >= 1 and st["adam_t"] + st["skipped_total"] == STEPS
    assert st["scale"] == INIT * 0.5 ** st["skipped_total"] and st["found_nonfinite"] == 0
    assert torch.equal(r["values1"], r["values0"]), "step 1 (scale 2^40) must have been skipped without a write"
    # (the weights stand still through the leading skipped steps: the loss of the first APPLIED step is the loss of step 1 up to the order of
    #  its fp32 atomics)
    assert all(x == x and abs(x) != INF for x in r["losses"]) and r["losses"][-1] < r["losses"][0]
    assert bool(torch.isfinite(r["arch"].params.values).all()) and not torch.equal(r["arch"].params.values, r["values0"])
    assert r["trainer"].program.loss_scale == st["scale"] and r["trainer"].program.scaler.skipped_steps == st["skipped_total"]


def _five_steps(loss_scale):
    arch, tj = _arch(loss_scale)
    prog = arch.program(B, H, W, training_json=tj)
    prog.set_inputs(*_batch(arch))
    for _ in range(5):
        prog.train_step()
    torch.cuda.synchronize()
    return arch.params.values.cpu().clone(), prog


def test_dynamic_at_4096_matches_the_static_default(tmp_path):
    """DD_DETERMINISTIC=1 (read once per process: a child) makes the two runs' gradients bit-equal, so what is left between a static 4096 and a
    dynamic scale that stays at 4096 is the lr_t derived on the device: the parameters agree within the op-level gate on p (2e-6 abs)."""
    _need_gpu()
    out = str(tmp_path / "runs.pt")
    env = dict(os.environ, DD_DETERMINISTIC="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "child failed\n%s\n%s" % (p.stdout[-2000:], p.stderr[-2000:])
    runs = torch.load(out)
    assert runs["state"] == {"scale": 4096.0, "good_steps": 5, "found_nonfinite": 0, "adam_t": 5, "skipped_total": 0} and runs["static_adam_step"] == 5
    moved = float((runs["static"] - runs["initial"]).abs().max())
    err = float((runs["dynamic"] - runs["static"]).abs().max())
    print("5 steps: parameters moved by up to %.3e; dynamic vs static max abs difference %.3e" % (moved, err))
    assert moved > 1e-4
    gate("dynamic(4096) vs static 4096 parameters after 5 steps (abs)", err, 2e-6)


# ---------------------------------------------------------------------------------------------------------------- 6. no host sync
def _steps_under_sync_debug(trainer, n=3):
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(n):
            trainer.step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()


def test_dynamic_step_makes_no_host_sync():
    _need_gpu()
    arch, tj, trainer = _trainer("dynamic")
    for _ in range(4):
        trainer.step()
    assert trainer._graphs is not None
    _steps_under_sync_debug(trainer)
    st = trainer.program.scaler.state()
    assert st["adam_t"] + st["skipped_total"] == 7


def test_static_fp16_step_is_what_the_sync_check_flags():
    """The same block on the static path raises: the check sees the synchronising overflow test the dynamic mode removes."""
    _need_gpu()
    arch, tj, trainer = _trainer(None)
    for _ in range(4):
        trainer.step()
    try:
        _steps_under_sync_debug(trainer)
    except RuntimeError as e:
        assert "synchroniz" in str(e).lower(), e
        return
    pytest.skip("torch.cuda.set_sync_debug_mode('error') of this torch build does not flag bool(tensor) on ROCm")


# ---------------------------------------------------------------------------------------------------------------- 7. checkpoint round trip
def test_checkpoint_round_trip(dynamic_run, tmp_path):
    r = dynamic_run
    prefix = tf_checkpoint.save_variables(r["arch"], str(tmp_path), global_step=STEPS)
    assert r["arch"].adam_step == r["state"]["adam_t"]
    saved = r["arch"].params.values.cpu()
    # a fresh dynamic program takes the whole record
    arch, tj = _arch({"init": INIT})
    prog = arch.program(B, H, W, training_json=tj)
    info = tf_checkpoint.load_variables(arch, prefix)
    assert prog.scaler.state() == r["state"]
    assert arch.adam_step == info["adam_step"] == r["state"]["adam_t"] and info["unused"] == [] and info["missing"] == []
    assert torch.equal(arch.params.values.cpu(), saved)
    # a static program does not know the two tensors
    arch, tj = _arch(None)
    prog = arch.program(B, H, W, training_json=tj)
    info = tf_checkpoint.load_variables(arch, prefix)
    assert sorted(info["unused"]) == sorted([tf_checkpoint.SCALE_KEY, tf_checkpoint.STEPS_KEY]) and info["missing"] == []
    assert prog.scaler is None and prog.loss_scale == 4096.0 and arch.adam_step == r["state"]["adam_t"]
    assert torch.equal(arch.params.values.cpu(), saved)


def test_static_checkpoint_has_no_extra_tensors(tmp_path):
    _need_gpu()
    arch, tj = _arch(None)
    arch.program(B, H, W, training_json=tj)
    prefix = tf_checkpoint.save_variables(arch, str(tmp_path), global_step=0)
    assert not [k for k in tf_checkpoint.read_checkpoint(prefix) if k.startswith("dd_loss_scale")]


if __name__ == "__main__":      # the child of test_dynamic_at_4096_matches_the_static_default
    initial = _arch(None)[0]
    initial.program(B, H, W, training_json=_tiny()[1])
    static, sprog = _five_steps(None)
    dynamic, dprog = _five_steps({"init": 4096.0, "growth_interval": 1000})
    torch.save({"initial": initial.params.values.cpu().clone(), "static": static, "dynamic": dynamic, "state": dprog.scaler.state(),
                "static_adam_step": sprog.arch.adam_step}, sys.argv[1])
