"""Gradient clipping, host side (no GPU): the numpy restatement tests/grad_clip_ref.py against a hand-computed case and against
tf.clip_by_global_norm's formula, the chunk planner of deepdenoiser_amd/grad_clip.py, and the settings (Architecture(clip_norm=...), the
train.py options, the Training.json key against the command line)."""
import math

import numpy as np
import pytest

import grad_clip_ref as R
from deepdenoiser_amd import configs
from deepdenoiser_amd import grad_clip as GC

INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_reference_by_hand():
    """Two variables, [3, 4] and [12], with one padding word each side that holds garbage: norms 5 and 12, global 13."""
    params = [("a", 0, 2), ("b", 4, 1)]
    g = np.array([3, 4, NAN, 77, 12, NAN, NAN, NAN], dtype=np.float32)
    w = np.array([1, 2, NAN, NAN, -2, 5, 5, 5], dtype=np.float32)
    r = R.reference(params, g, w, 1.0, 6.5)
    assert r["variables"]["a"] == {"grad_sq": 25.0, "weight_sq": 5.0, "nonfinite": 0, "grad_norm": 5.0, "weight_norm": math.sqrt(5.0)}
    assert r["variables"]["b"]["grad_norm"] == 12.0 and r["variables"]["b"]["weight_norm"] == 2.0
    assert r["grad_norm"] == 13.0 and r["coef"] == 0.5 and r["nonfinite_total"] == 0 and r["nonfinite_variables"] == 0
    # the factor of the true gradient scales the norm, not the stored sums
    h = R.reference(params, g, w, -0.5, 6.5)
    assert h["grad_norm"] == 6.5 and h["coef"] == 1.0 and h["variables"]["a"]["grad_sq"] == 25.0 and h["variables"]["a"]["grad_norm"] == 2.5
    # measure only
    for off in (None, 0, 0.0, -1.0):
        assert R.reference(params, g, w, 1.0, off)["coef"] == 1.0 and R.reference(params, g, w, 1.0, off)["grad_norm"] == 13.0


def test_reference_is_clip_by_global_norm():
    """t * clip_norm / max(global_norm, clip_norm) for every tensor t (tf.clip_by_global_norm), below and above the norm."""
    rng = np.random.default_rng(0)
    params, total = R.layout([5, 17, 1, 4096 + 3])
    g = rng.standard_normal(total).astype(np.float32)
    w = rng.standard_normal(total).astype(np.float32)
    tensors = [g[o:o + n].astype(np.float64) for _, o, n in params]
    global_norm = math.sqrt(sum(float(np.sum(t ** 2)) for t in tensors))
    for clip_norm in (0.25 * global_norm, 4.0 * global_norm):
        r = R.reference(params, g, w, 1.0, clip_norm)
        assert r["grad_norm"] == pytest.approx(global_norm, rel=1e-14)
        for t in tensors:
            np.testing.assert_allclose(t * r["coef"], t * clip_norm / max(global_norm, clip_norm), rtol=1e-14)
        assert (r["coef"] == 1.0) == (clip_norm > global_norm)
        clipped = math.sqrt(sum(float(np.sum((t * r["coef"]) ** 2)) for t in tensors))
        assert clipped == pytest.approx(min(global_norm, clip_norm), rel=1e-12)


def test_reference_nonfinite_rule():
    params = [("a", 0, 3), ("b", 4, 2), ("c", 8, 1)]
    g = np.array([1, INF, 2, 0, NAN, -INF, 0, 0, 2, 0, 0, 0], dtype=np.float32)
    r = R.reference(params, g, np.ones(12, dtype=np.float32), 1.0, 0.5)
    assert r["grad_norm"] == INF and r["coef"] == 1.0 and r["nonfinite_total"] == 3 and r["nonfinite_variables"] == 2
    assert [r["variables"][n]["nonfinite"] for n in "abc"] == [1, 2, 0]
    assert [r["variables"][n]["grad_sq"] for n in "abc"] == [5.0, 0.0, 4.0]      # the sums leave the non-finite elements out


def test_arenas_hold_what_the_gpu_tests_rely_on():
    params, total = R.layout()
    g, w = R.arenas(params, total)
    covered = np.zeros(total, dtype=bool)
    for _, o, n in params:
        covered[o:o + n] = True
    assert (~covered).sum() > 300 and np.isnan(g[~covered]).all() and np.isnan(w[~covered]).all()
    inside = g[covered].astype(np.float64)
    assert np.isfinite(inside).all() and np.isfinite(w[covered]).all()
    assert (inside == np.float32(3.4e38)).sum() == 1 and (inside == np.float32(-3.4e38)).sum() == 1
    assert ((inside != 0) & (np.abs(inside) < 1.1e-38)).sum() >= 5 and (inside == 0).sum() >= 4
    assert math.log10(np.abs(inside[inside != 0]).max() / np.abs(inside[inside != 0]).min()) > 40
    r = R.reference(params, g, w, 0.5, None)
    assert np.isfinite(np.float32(r["grad_norm"]))           # the float of the clip record can hold the true norm at gs = 0.5


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_planner_tiles_every_variable_and_nothing_else():
    params, total = R.layout()
    assert [n for _, _, n in params] == [1, 3, 4, 5, 4095, 4096, 4097, 8195] + [1] * 300
    chunks, var_first = GC.plan_chunks(params)
    assert len(var_first) == len(params) + 1 and var_first[0] == 0 and var_first[-1] == len(chunks)
    covered = np.zeros(total, dtype=np.int32)
    for v, (name, off, size) in enumerate(params):
        mine = chunks[var_first[v]:var_first[v + 1]]
        assert mine and all(c[2] == v for c in mine)
        pos = off
        for o, n, _ in mine:                       # in order, gap-free, inside the variable
            assert o == pos and 1 <= n <= GC.CHUNK == 4096
            pos += n
        assert pos == off + size
        assert all(n == GC.CHUNK for _, n, _ in mine[:-1])
        assert len(mine) == -(-size // GC.CHUNK)
    for o, n, _ in chunks:
        covered[o:o + n] += 1
    want = np.zeros(total, dtype=np.int32)
    for _, off, size in params:
        want[off:off + size] = 1
    assert np.array_equal(covered, want)           # every element once, no padding word at all
    assert [c[2] for c in chunks] == sorted(c[2] for c in chunks)
    assert [len(chunks[var_first[v]:var_first[v + 1]]) for v in range(8)] == [1, 1, 1, 1, 1, 1, 2, 3]
    assert chunks[var_first[7] + 2][1] == 3 and chunks[var_first[6] + 1][1] == 1


def test_planner_follows_the_store_layout():
    """Over a real ParamStore (no device memory: the layout exists before finalize)."""
    from deepdenoiser_amd.engine import ParamStore
    ps = ParamStore()
    for i, shape in enumerate([(3, 3, 7, 5), (5,), (1,), (2, 2, 64, 33)]):
        ps.get("p%d" % i, shape)
    chunks, var_first = GC.plan_chunks([(p.name, p.offset, p.size) for p in ps.params])
    assert [sum(n for _, n, _ in chunks[var_first[v]:var_first[v + 1]]) for v in range(4)] == [315, 5, 1, 8448]
    assert all(o % 4 == 0 for o, _, _ in chunks)   # 16-byte aligned variables and 4096-element pieces: every chunk starts on a vector
    assert max(o + n for o, n, _ in chunks) <= ps.total
    with pytest.raises(ValueError):
        GC.plan_chunks([("bad", -4, 3)])


# ---------------------------------------------------------------------------------------------------------------- the settings
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, INF, -INF, NAN, "1.0", "dynamic", True, False, [1.0]])
def test_architecture_refuses(bad):
    from deepdenoiser_amd.architecture import Architecture
    with pytest.raises(ValueError, match="clip_norm"):
        Architecture(configs.architecture(filters=(16, 24), convs=1), device="cpu", clip_norm=bad)


def test_architecture_accepts():
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.architecture(filters=(16, 24), convs=1)
    a = Architecture(aj, device="cpu")
    assert a.clip_norm is None and a.track_gradient_norms is False and a.grad_clipper is None
    assert Architecture(aj, device="cpu", clip_norm=None).clip_norm is None
    assert Architecture(aj, device="cpu", clip_norm=2).clip_norm == 2.0
    b = Architecture(aj, device="cpu", clip_norm=0.125, loss_scale="dynamic", track_gradient_norms=True)
    assert b.clip_norm == 0.125 and b.track_gradient_norms is True


def test_parser_accepts_both_options():
    from deepdenoiser_amd import train
    args = train.parser().parse_args(["t.json"])
    assert args.clip_norm is None and args.gradient_norms is False
    args = train.parser().parse_args(["t.json", "--clip_norm", "0.5", "--gradient_norms", "--summary_steps", "1"])
    assert args.clip_norm == 0.5 and args.gradient_norms is True
    assert train.parser().parse_args(["t.json", "--clip_norm", "0"]).clip_norm == 0.0
    for bad in ("-1", "inf", "nan", "dynamic"):
        with pytest.raises(SystemExit):
            train.parser().parse_args(["t.json", "--clip_norm", bad])


def test_json_key_against_the_command_line():
    r = GC.resolve_clip_norm
    assert r(None, {}) is None and r(None, {"gradient_clip_norm": None}) is None and r(None, {"gradient_clip_norm": 0}) is None
    assert r(None, {"gradient_clip_norm": 2.5}) == 2.5 and r(None, {"gradient_clip_norm": 3}) == 3.0
    assert r(1.5, {}) == 1.5 and r(1.5, {"gradient_clip_norm": 2.5}) == 1.5 and r(1.5, {"gradient_clip_norm": None}) == 1.5      # the command line wins
    assert r(0.0, {"gradient_clip_norm": 2.5}) is None                                                                        # ... also to switch it off
    for bad in (-1.0, "2.5", True, INF, NAN):
        with pytest.raises(ValueError):
            r(None, {"gradient_clip_norm": bad})


def test_summary_tags():
    from deepdenoiser_amd import train
    rep = {"grad_norm": 13.0, "coef": 0.5, "nonfinite_variables": 0, "nonfinite_total": 0,
           "variables": {"a/kernel": {"grad_norm": 5.0, "weight_norm": 1.0, "nonfinite": 0}, "a/bias": {"grad_norm": 12.0, "weight_norm": 2.0, "nonfinite": 0}}}
    assert train.gradient_scalars(rep) == [("gradient_norm", 13.0), ("gradient_clip_coefficient", 0.5)]
    assert train.gradient_scalars(rep, per_variable=True) == [
        ("gradient_norm", 13.0), ("gradient_clip_coefficient", 0.5), ("gradient_nonfinite_variables", 0),
        ("gradient_norm/a/kernel", 5.0), ("gradient_norm/a/bias", 12.0), ("weight_norm/a/kernel", 1.0), ("weight_norm/a/bias", 2.0)]
