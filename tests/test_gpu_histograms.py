"""-m gpu: the tracked histograms on the device -- dd_histogram_values / dd_loss_histograms (csrc/dd_histogram.hip) against
tests/histogram_ref.py (a numpy restatement of TensorFlow's histogram) on the five cases of tests/golden/metrics_golden.*,
Program.histograms() against the tracked scalars of the same forward, and the training command line's event file.

Gates.  The binning primitive is exact: counts, num, min, max equal the reference, sum / sum_squares differ by at most n 2^-53 sum|term|
(the bound for reordering a double sum).  The fused launch forms its values in fp32 where the reference has float64, so a value within
tau of a bucket limit may fall on either side of it: for every limit e the device's cumulative count below e lies between the reference's
cumulative counts below e - tau and below e + tau, tau = ACC32["f32"] * S with S the size of the terms (3 for SMAPE: each channel term is at
most 1; the largest per-pixel sum_c(|p| + |t|) of the source for ABSOLUTE; doubled for the variation kind)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import histogram_ref as HR
import metrics_util as U
import test_gpu_metrics as TM
from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs, summaries
from deepdenoiser_amd import metrics as M
from gpu_util import ACC32, gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(U.GOLDEN, "histogram_golden.json")))
NB = len(HR.LIMITS)
REC = L.histogram_record_bytes(NB)
FLT_MAX = float(np.finfo(np.float32).max)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def limits_dev():
    TM._need_gpu()
    return torch.from_numpy(HR.LIMITS).cuda()


def _garbage(n_records):
    """records the entries promise to overwrite: every byte set"""
    return torch.full((n_records * REC,), 0xAB, dtype=torch.uint8, device="cuda")


def _values_table(values, limits_dev):
    lib = L.load()
    v = torch.from_numpy(np.asarray(values, dtype=np.float32)).cuda()
    rec = _garbage(1)
    scratch = torch.full((L.HISTOGRAM_VALUES_SCRATCH_BYTES // 8,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.dd_histogram_values(v.data_ptr(), v.numel(), limits_dev.data_ptr(), NB, rec.data_ptr(), scratch.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return M.decode_histogram_records(rec.cpu().numpy(), 1, NB), rec


def _check_exact(name, values, got):
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    h = HR.Histogram(v)
    fin = v[np.isfinite(v)]
    assert np.array_equal(got["counts"][0], h.counts), name
    assert int(got["num"][0]) == h.num and int(got["nonfinite"][0]) == h.nonfinite, name
    assert got["min"][0] == h.min and got["max"][0] == h.max, (name, got["min"][0], h.min, got["max"][0], h.max)
    n = max(fin.size, 1)
    for key, terms in (("sum", fin), ("sum_squares", fin * fin)):
        bound = n * 2.0 ** -53 * float(np.abs(terms).sum())
        err = abs(float(got[key][0]) - float(getattr(h, key)))
        print("%-28s %-12s %.17g (reference %.17g) |diff| %.3e bound %.3e" % (name, key, got[key][0], getattr(h, key), err, bound))
        assert err <= bound, (name, key, err, bound)


def _edge_values():
    """float32(limit) and its two fp32 neighbours for every limit inside the fp32 range, zeros, denormals, the ends of the range"""
    lim = HR.LIMITS[np.abs(HR.LIMITS) <= FLT_MAX]
    f = lim.astype(np.float32)
    edges = np.concatenate([f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))])
    tiny = np.float32(1e-45)
    special = np.array([0.0, -0.0, tiny, -tiny, 1e-40, -1e-40, 1e-30, -1e-30, 1e30, -1e30, FLT_MAX, -FLT_MAX], dtype=np.float32)
    assert special[2] > 0 and special[4] > 0      # (denormals survive the conversion)
    return np.concatenate([special, edges]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the primitive
def test_values_exact(limits_dev):
    """1: every fp32 at and next to a bucket limit, zeros, denormals, +-FLT_MAX; lengths 1, 63, 65 and 100 003 (more than one workgroup)."""
    edge = _edge_values()
    rng = np.random.default_rng(3)
    body = (rng.standard_normal(100003 - edge.size) * 10.0 ** rng.uniform(-14, 20, 100003 - edge.size)).astype(np.float32)
    long = rng.permutation(np.concatenate([edge, body]))
    assert long.size == 100003 and np.isfinite(long).all()
    for name, v in (("one", edge[5:6]), ("63", edge[100:163]), ("65", edge[1200:1265]), ("100003", long), ("edges in order", edge)):
        got, _ = _values_table(v, limits_dev)
        _check_exact(name, v, got)
    again, rec2 = _values_table(long, limits_dev)
    _, rec1 = _values_table(long, limits_dev)
    assert torch.equal(rec1, rec2), "two runs differ"


def test_values_single_bin(limits_dev):
    """1: a million zeros, the case the wave-level fold exists for"""
    v = np.zeros(1 << 20, dtype=np.float32)
    got, _ = _values_table(v, limits_dev)
    _check_exact("1M zeros", v, got)
    assert int(got["counts"][0][776]) == 1 << 20


def test_values_nonfinite(limits_dev):
    """1: NaN and inf are counted and touch nothing else"""
    rng = np.random.default_rng(4)
    clean = (rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 6, 5000)).astype(np.float32)
    dirty = np.insert(clean, [0, 2500, 4999], [np.nan, np.inf, np.nan]).astype(np.float32)
    a, _ = _values_table(clean, limits_dev)
    b, _ = _values_table(dirty, limits_dev)
    assert int(b["nonfinite"][0]) == 3 and int(a["nonfinite"][0]) == 0
    _check_exact("clean", clean, a)
    _check_exact("with 2 NaN + inf", dirty, b)
    assert np.array_equal(a["counts"], b["counts"]) and a["num"][0] == b["num"][0] and a["min"][0] == b["min"][0] and a["max"][0] == b["max"][0]
    only, _ = _values_table(np.array([np.nan, -np.inf], dtype=np.float32), limits_dev)      # nothing finite: an empty histogram
    assert int(only["num"][0]) == 0 and int(only["nonfinite"][0]) == 2 and not only["counts"].any()
    assert only["min"][0] == HR.DBL_MAX and only["max"][0] == -HR.DBL_MAX and only["sum"][0] == 0.0


def test_values_bad_arguments_return_a_status(limits_dev):
    lib = L.load()
    v = torch.zeros(64, device="cuda")
    rec = _garbage(1)
    scratch = torch.zeros(L.HISTOGRAM_VALUES_SCRATCH_BYTES // 8, dtype=torch.float64, device="cuda")
    ok = (v.data_ptr(), 64, limits_dev.data_ptr(), NB, rec.data_ptr(), scratch.data_ptr())
    for i, bad, word in ((0, None, b"null"), (2, None, b"null"), (4, None, b"null"), (5, None, b"null"), (0, ok[0] + 2, b"aligned"),
                         (2, ok[2] + 4, b"aligned"), (4, ok[4] + 4, b"aligned"), (5, ok[5] + 4, b"aligned"), (1, 0, b"n = 0"), (1, 1 << 32, b"2^32"), (3, NB + 1, b"bucket"),
                         (3, 1, b"bucket")):
        args = list(ok)
        args[i] = bad
        assert lib.dd_histogram_values(*args, _stream()) == -1, (i, bad)
        assert word in lib.dd_last_error(), (i, lib.dd_last_error())
    torch.cuda.synchronize()
    assert (rec == 0xAB).all(), "a refused call wrote"
    assert lib.dd_loss_histograms_scratch_bytes(0, 4, 4, 1) < 0 and lib.dd_loss_histograms_scratch_bytes(2, 4, 4, 0) < 0
    assert lib.dd_loss_histograms(None, 2, 4, 4, None, 1, None, NB, None, None, _stream()) == -1


# ---------------------------------------------------------------------------------------------------------------- the fused launch
def _run_loss_histograms(d, B, h, w, sel_pairs, limits_dev):
    lib = L.load()
    n = len(sel_pairs)
    sel = (C.c_int * (2 * n))(*[x for pair in sel_pairs for x in pair])
    nbytes = lib.dd_loss_histograms_scratch_bytes(B, h, w, n)
    assert nbytes > 0
    scratch = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    rec = _garbage(n)
    L.check(lib.dd_loss_histograms(C.byref(d), B, h, w, sel, n, limits_dev.data_ptr(), NB, rec.data_ptr(), scratch.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize("case", U.CASES)
def test_loss_histograms_against_the_reference(case, limits_dev):
    """2: every histogram of every fixture case (B = 2; 16 x 16 with scales 16 / 8 / 4, 48 x 44: clipped tiles, images narrower than a tile),
    one prediction with pixel stride 4, the 1-channel pass as in test_gpu_metrics.py."""
    c = U.Case(case)
    tj = HR.with_histogram_flags(c.tj, GOLDEN["cases"][case]["masked"])
    plan = M.histogram_plan(c.arch, tj)
    assert [e.tag for e in plan] == GOLDEN["cases"][case]["tags"]
    kind = tj["loss_difference"]
    assert kind in ("SMAPE", "ABSOLUTE")
    op = TM._CaseOp(c)
    delta = ACC32["f32"]
    worst = {"min/max": 0.0, "sum": 0.0}
    moved = 0
    for s in sorted({e.scale_index for e in plan}):
        h, w = c.dims[s]
        entries = [e for e in plan if e.scale_index == s]
        d = op.desc(s)
        pairs = [(c.slot_of[e.source], M.HISTOGRAM_KINDS.index(e.kind)) for e in entries]
        rec = _run_loss_histograms(d, c.B, h, w, pairs, limits_dev)
        assert torch.equal(rec, _run_loss_histograms(d, c.B, h, w, pairs, limits_dev)), "scale %d: two runs differ" % s
        got = M.decode_histogram_records(rec.cpu().numpy(), len(entries), NB)
        src = c.sources(s)
        for r, e in enumerate(entries):
            p, y, m = src[e.source]
            ref = np.sort(HR.source_values(p, y, m, e.kind, kind))
            S = 3.0 if kind == "SMAPE" else float((p.abs() + y.abs()).sum(dim=3).max())
            tau = delta * S * (2.0 if e.kind == "variation_difference" else 1.0)
            pairs_n = c.B * (h * (w - 1) + (h - 1) * w)
            assert int(got["num"][r]) == ref.size == (pairs_n if e.kind == "variation_difference" else c.B * h * w), e.tag
            assert int(got["nonfinite"][r]) == 0 and int(got["counts"][r].sum()) == ref.size, e.tag
            if e.kind == "masked_difference":      # the zeros of the mask are values too: they sit in the bucket of 0.0
                zeros = int((m == 0).sum())
                assert zeros < ref.size and (zeros > 0 or s > 0) and int(got["counts"][r][776]) >= zeros, e.tag      # (pooling fills the holes)
            cum = np.cumsum(got["counts"][r])                       # values below limit j
            lo = np.searchsorted(ref, HR.LIMITS - tau, side="left")
            hi = np.searchsorted(ref, HR.LIMITS + tau, side="left")
            assert ((lo <= cum) & (cum <= hi)).all(), (e.tag, int(np.argmax((cum < lo) | (cum > hi))))
            moved += int((cum != np.searchsorted(ref, HR.LIMITS, side="left")).sum())
            worst["min/max"] = max(worst["min/max"], abs(got["min"][r] - ref[0]) / tau, abs(got["max"][r] - ref[-1]) / tau)
            worst["sum"] = max(worst["sum"], abs(got["sum"][r] - ref.sum()) / (ref.size * tau))
    print("%s: %d histograms, %d cumulative counts differ from the float64 reference's; min / max error %.3g tau, sum error %.3g num tau"
          % (case, len(plan), moved, worst["min/max"], worst["sum"]))
    gate("%s: histogram min / max error in units of tau" % case, worst["min/max"], 1.0)
    gate("%s: histogram sum error in units of num tau" % case, worst["sum"], 1.0)


def test_loss_histograms_refuses_bad_selections(limits_dev):
    c = U.Case("alpha_unmasked")
    op = TM._CaseOp(c)
    lib = L.load()
    d = op.desc(0, masked=False)
    scratch = torch.zeros(lib.dd_loss_histograms_scratch_bytes(c.B, c.H, c.W, 2) // 8, dtype=torch.float64, device="cuda")
    rec = _garbage(2)

    def call(*pairs):
        sel = (C.c_int * (2 * len(pairs)))(*[x for pr in pairs for x in pr])
        return lib.dd_loss_histograms(C.byref(d), c.B, c.H, c.W, sel, len(pairs), limits_dev.data_ptr(), NB, rec.data_ptr(), scratch.data_ptr(), _stream())
    assert call((0, L.HISTOGRAM_MASKED_DIFFERENCE)) == -1 and b"no mask feature" in lib.dd_last_error()
    assert call((0, 0), (0, 0)) == -1 and b"repeats" in lib.dd_last_error()
    assert call((len(c.head), 0)) == -1 and b"does not have" in lib.dd_last_error()
    assert call((0, 3)) == -1 and b"kind" in lib.dd_last_error()
    assert call((L.MAX_FEATURES + L.MAX_COMBINED, 0)) == -1      # this case builds no combined image
    torch.cuda.synchronize()
    assert (rec == 0xAB).all()


# ---------------------------------------------------------------------------------------------------------------- whole program
def test_program_histograms_agree_with_the_tracked_scalars():
    """3: the 17-pass network, B = 4, f32: per tag sum / num is the track_mean / track_variation scalar of the same forward; the masked
    difference's sum is the masked sum of the metric table."""
    TM._need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    B, H, W = 4, 32, 32
    aj = configs.architecture(filters=(16, 24), convs=1)
    tj = configs.training()
    for lv in TM.LEVELS:
        tj[lv]["statistics"].update(track_mean=True, track_variation=True, track_difference_histogram=True, track_variation_difference_histogram=True)
    # (the network has an Alpha pass: no masking on the features level, Training.py:103-113)
    tj[TM.LEVELS[1]]["statistics_masked"].update(track_mean=True, track_difference_histogram=True)
    arch = Architecture(aj, device="cuda", dtype="f32")
    prog = arch.program(B, H, W, training_json=tj)
    prog.write_histograms = True
    n_fwd = len(prog.g.fwd_ops)
    feats, labels = TM._program_inputs(arch, B, H, W)
    prog.set_inputs(feats, labels)
    prog.zero_grads()
    prog.forward()
    said = []
    histos = prog.histograms(out=said.append)
    scalars = dict(zip([e.name for e in prog.metric_plan()], prog.metrics()))
    table = prog.metric_table().cpu().numpy()
    torch.cuda.synchronize()
    assert len(prog.g.fwd_ops) == n_fwd, "histograms() must not add to the forward program"
    plan = prog.histogram_plan()
    assert said == [] and [t for t, _ in histos] == [e.tag for e in plan] == [e.tag for e in M.histogram_plan(arch, tj)]
    assert {(e.source[0], e.kind) for e in plan} == {(a, k) for a in ("feature", "combined", "image") for k in M.HISTOGRAM_KINDS[:2]} | \
        {("combined", "masked_difference")}
    assert {e.scale_index for e in plan} == {0, 1} and len(plan) == 2 * (17 * 2 + 4 * 3 + 2)
    st = prog.tracking_metrics
    worst = 0.0
    for e, (tag, h) in zip(plan, histos):
        hh, ww = prog.dims[e.scale_index]
        assert h["num"] == (B * hh * ww if e.kind != "variation_difference" else B * (hh * (ww - 1) + (hh - 1) * ww)), tag
        assert sum(h["bucket"]) == h["num"] and h["min"] <= h["sum"] / h["num"] <= h["max"]
        if e.kind == "difference":
            want = scalars[tag.replace("_difference", "_mean")]
        elif e.kind == "variation_difference":
            want = scalars[tag.replace("_variation_difference", "_variation_mean")]
        else:      # sum of difference * mask over the batch, from the metric table of that scale
            rows = table[st.scales.index(e.scale_index) * st.rows:][:st.rows].reshape(L.METRIC_SOURCES, B, 4)
            want = float(rows[st.slot_of[e.source], :, 2].astype(np.float64).sum()) / h["num"]
            assert h["bucket"][h["bucket_limit"].index(1e-12)] >= 4 * 12 * 12 >> (2 * e.scale_index)      # the hole of _program_inputs
        err = abs(h["sum"] / h["num"] - want) / abs(want)
        worst = max(worst, err)
    gate("Program.histograms(): sum / num against the tracked scalars", worst, ACC32["f32"])
    assert torch.equal(prog.histogram_table().clone(), prog.histogram_table()), "two runs differ"


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_writes_histograms(tmp_path):
    """4: one epoch of `python -m deepdenoiser_amd.train --histograms --summary_steps 1` on the data set of test_cli_writes_event_files."""
    TM._need_gpu()
    from deepdenoiser_amd.architecture import Architecture
    aj = configs.architecture(filters=(16, 24), convs=1, flag_mode="NONE", combined=TM.NO_ALPHA)
    aj["model_directory"] = "model"
    tj = configs.training(learning_rate=2e-3, batch_size=4)
    tj.update({"architecture": "architecture.json", "base_tfrecords_directory": "data", "modes": ["training"], "number_of_source_index_tuples": 1})
    tj["data_augmentation"] = {"use_rotate_90": True, "use_flip_left_right": False, "use_rgb_permutation": True, "use_normal_rotation": False}
    for lv in TM.LEVELS:
        tj[lv]["statistics"].update(track_mean=True, track_variation=True, track_difference_histogram=True, track_variation_difference_histogram=True)
    for lv in TM.LEVELS[:2]:
        tj[lv]["statistics_masked"].update(track_mean=True, track_difference_histogram=True)
    json.dump(aj, open(tmp_path / "architecture.json", "w"))
    json.dump(tj, open(tmp_path / "training.json", "w"))
    arch = Architecture(aj, device="cpu")
    TM._write_dataset(str(tmp_path / "data"), arch, "training", 2, 4, 0)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "deepdenoiser_amd.train", str(tmp_path / "training.json"), "--histograms", "--summary_steps", "1",
                        "--train_epochs", "1", "--dtype", "f32"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "epoch 1: global_step 2" in p.stdout and "not written" not in p.stdout, p.stdout
    names = [e.name for e in M.metric_plan(arch, tj, out=lambda *a: None)]
    tags = [e.tag for e in M.histogram_plan(arch, tj)]
    assert len(tags) > 100 and not set(tags) & set(names)
    (train_file,) = summaries.event_files(str(tmp_path / "model"))
    events = [e for e in summaries.read_events(train_file) if e["file_version"] is None]
    assert [e["step"] for e in events] == [1, 2]      # ONE event per step
    for e in events:
        assert e["tags"] == ["loss", "learning_rate", "batch_size"] + tags + names
        # the scalars are those of a run without the flag: same tags, same order
        assert [t for t, _ in e["scalars"]] == ["loss", "learning_rate", "batch_size"] + names
        assert all(np.isfinite(v) for _, v in e["scalars"])
        by = dict(e["scalars"])
        for tag, h in e["histograms"]:
            assert h["num"] > 0 and sum(h["bucket"]) == h["num"] and len(h["bucket"]) == len(h["bucket_limit"]) and h["bucket_limit"][-1] == HR.DBL_MAX
            assert h["bucket_limit"] == sorted(h["bucket_limit"]) and set(h["bucket_limit"]) <= set(HR.LIMITS.tolist())
        for tag, h in e["histograms"]:      # the event stores the scalar as an fp32
            if "_masked/" in tag or "variation" in tag:
                continue
            want = by[tag.replace("_difference", "_mean")]
            assert abs(h["sum"] / h["num"] - want) <= (ACC32["f32"] + 2.0 ** -23) * abs(want), tag
    # (of "the scalars of a run without the flag" only tags and order are pinned, above: the values of two training runs differ in the last
    #  bits of the step's unordered fp32 atomics)
    assert [(s, t) for s, t, _ in summaries.read_scalars(train_file)] == [(s, t) for s in (1, 2) for t in ["loss", "learning_rate", "batch_size"] + names]
    assert [(s, t) for s, t, _ in summaries.read_histograms(train_file)] == [(s, t) for s in (1, 2) for t in tags]
