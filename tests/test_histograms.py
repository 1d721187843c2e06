"""The host side of the tracked histograms (deepdenoiser_amd/metrics.py, summaries.py) without a GPU: the plan against
tests/golden/histogram_golden.json (the reference's own training branch, executed: tests/golden/make_histogram_golden.py), TensorFlow's
bucket limits and EncodeToProto against hand-worked examples and tests/histogram_ref.py, the event bytes against a message assembled by hand
from the .proto field numbers, the merge of two tables, and the statistics of the reference's float64 tensors."""
import json
import os
import struct

import numpy as np
import pytest

import histogram_ref as HR
import metrics_util as U
from deepdenoiser_amd import metrics as M
from deepdenoiser_amd import summaries
from deepdenoiser_amd import tfrecords as R

GOLDEN = json.load(open(os.path.join(U.GOLDEN, "histogram_golden.json")))
DBL_MAX = 1.7976931348623157e308


def _case(name):
    c = U.Case(name)
    tj = HR.with_histogram_flags(c.tj, GOLDEN["cases"][name]["masked"])
    return c, tj, M.histogram_plan(c.arch, tj)


def reference_table(c, plan, loss_difference):
    """histogram_ref over the float64 values of Case.sources(), rows in plan order."""
    src = {s: c.sources(s) for s in sorted({e.scale_index for e in plan})}
    return HR.table_of([HR.Histogram(HR.source_values(*src[e.scale_index][e.source], e.kind, loss_difference)) for e in plan])


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("case", U.CASES)
def test_plan_is_the_reference_call_order(case):
    c, tj, plan = _case(case)
    assert [e.tag for e in plan] == GOLDEN["cases"][case]["tags"]
    assert len(plan) > 0 and {e.kind for e in plan} <= set(M.HISTOGRAM_KINDS)
    if not tj["use_multiscale_metrics"]:
        assert {e.scale_index for e in plan} == {0}


def test_plan_refuses_what_the_reference_cannot_run():
    c = U.Case("full_multiscale_smape")
    g = GOLDEN["masked_variation_difference_histogram"]
    assert g["fails_in_reference"] and g["case"] == "full_multiscale_smape"
    for level in HR.LEVELS[:2]:
        tj = HR.with_histogram_flags(c.tj, True)
        tj[level]["statistics_masked"]["track_variation_difference_histogram"] = True
        with pytest.raises(ValueError, match=level + ".statistics_masked.track_variation_difference_histogram"):
            M.histogram_plan(c.arch, tj)
    assert g["key"] == "features_training_settings.statistics_masked.track_variation_difference_histogram"
    a = U.Case("alpha_unmasked")
    tj = HR.with_histogram_flags(a.tj, True)
    with pytest.raises(Exception, match="alpha pass"):
        M.histogram_plan(a.arch, tj)


def test_metric_plan_message_only_without_histograms():
    c = U.Case("full_scale0_absolute")
    tj = HR.with_histogram_flags(c.tj, True)
    said = []
    M._said_histograms.clear()
    plan = M.metric_plan(c.arch, tj, out=said.append, histograms=True)
    assert said == [] and [e.name for e in plan] == c.names
    M.metric_plan(c.arch, tj, out=said.append)
    M.metric_plan(c.arch, tj, out=said.append)
    assert len(said) == 1 and "histograms are not written" in said[0]


# ---------------------------------------------------------------------------------------------------------------- limits
def test_limits():
    lim = M.histogram_limits()
    assert lim.dtype == np.float64 and len(lim) == 1551
    assert (np.diff(lim) > 0).all()
    assert lim[775] == 0.0 and lim[776] == 1e-12
    assert np.array_equal(lim, -lim[::-1])
    assert lim[-1] == DBL_MAX
    assert lim[777] == 1e-12 * 1.1 and lim[778] == 1e-12 * 1.1 * 1.1      # multiplied up, not 1e-12 * 1.1 ** k
    assert lim[-2] < 1e20 <= lim[-2] * 1.1
    assert np.array_equal(lim, HR.LIMITS)


# ---------------------------------------------------------------------------------------------------------------- encoding
def _encode(values):
    h = HR.Histogram(values)
    got = M.compress_buckets(M.histogram_limits(), h.counts)
    assert got == h.encode()
    return got


def test_encoding_against_hand_worked_examples():
    lim = M.histogram_limits()
    # empty: one entry (DBL_MAX, 0)
    assert _encode([]) == ([DBL_MAX], [0.0])
    # one value, 0.0: bucket 776 (limit 1e-12); the run of empty buckets before it ends at limit 0.0, the run after it at DBL_MAX
    assert _encode([0.0]) == ([0.0, 1e-12, DBL_MAX], [0.0, 1.0, 0.0])
    assert _encode([-0.0]) == _encode([0.0])
    # two values separated by a run of empty buckets: 1.0 lies in [lim[k-1], lim[k]) with k = upper_bound
    k = int(np.searchsorted(lim, 1.0, side="right"))
    assert lim[k - 1] <= 1.0 < lim[k]
    assert _encode([0.0, 1.0]) == ([0.0, 1e-12, lim[k - 1], lim[k], DBL_MAX], [0.0, 1.0, 0.0, 1.0, 0.0])
    # values in adjacent buckets (a limit itself belongs to the bucket ABOVE it): lim[k-1] and 1.0 share bucket k, lim[k] is in k + 1
    assert _encode([lim[k], lim[k - 1], 1.0]) == ([lim[k - 1], lim[k], lim[k + 1], DBL_MAX], [0.0, 2.0, 1.0, 0.0])
    # beyond the last finite limit on both sides: bucket 0 (limit -DBL_MAX) stays empty, -1e30 is in bucket 1, 1e30 in the last one
    assert _encode([-1e30, 1e30]) == ([lim[0], lim[1], lim[-2], DBL_MAX], [0.0, 1.0, 0.0, 1.0])


def test_histogram_values_fields_and_nonfinite():
    plan = [M.HistogramEntry("a/1", ("feature", "A"), "difference", 0), M.HistogramEntry("b/1", ("feature", "B"), "difference", 0)]
    table = HR.table_of([HR.Histogram([0.5, 2.0, 2.0]), HR.Histogram([1.0, float("nan"), float("inf")])])
    said = []
    M._said_nonfinite.clear()
    got = M.histogram_values(plan, table, out=said.append)
    assert [t for t, _ in got] == ["a/1"]
    h = got[0][1]
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (0.5, 2.0, 3.0, 4.5, 8.25)
    assert sum(h["bucket"]) == 3.0 and len(h["bucket"]) == len(h["bucket_limit"])
    assert len(said) == 1 and "b/1" in said[0] and "2 value" in said[0]
    M.histogram_values(plan, table, out=said.append)
    assert len(said) == 1      # once per tag


# ---------------------------------------------------------------------------------------------------------------- event bytes
def _varint(n):
    out = b""
    while True:
        b, n = n & 0x7F, n >> 7
        out += bytes([b | (0x80 if n else 0)])
        if not n:
            return out


def _ld(num, payload):
    return _varint((num << 3) | 2) + _varint(len(payload)) + payload


def _f64(num, v):
    return _varint((num << 3) | 1) + struct.pack("<d", v)


def test_event_bytes_assembled_by_hand(tmp_path):
    h = {"min": -1.5, "max": 2.0, "num": 3.0, "sum": 0.75, "sum_squares": 6.3125, "bucket_limit": [0.0, 1e-12, DBL_MAX], "bucket": [1.0, 2.0, 0.0]}
    histo = (_f64(1, -1.5) + _f64(2, 2.0) + _f64(3, 3.0) + _f64(4, 0.75) + _f64(5, 6.3125)
             + _ld(6, struct.pack("<3d", 0.0, 1e-12, DBL_MAX)) + _ld(7, struct.pack("<3d", 1.0, 2.0, 0.0)))

    def scalar(tag, v):
        return _ld(1, _ld(1, tag.encode()) + _varint((2 << 3) | 5) + struct.pack("<f", v))
    value_h = _ld(1, _ld(1, b"diffuse_difference/1") + _ld(5, histo))
    want = _f64(1, 12.5) + _varint(2 << 3) + _varint(7) + _ld(5, scalar("loss", 0.25) + scalar("batch_size", 4.0) + value_h + scalar("x_mean/1", 1.0))
    got = summaries.encode_event(12.5, step=7, scalars=[("loss", 0.25), ("batch_size", 4.0)], histograms=[("diffuse_difference/1", h)],
                                 tracked=[("x_mean/1", 1.0)])
    assert got == want
    # without tracked scalars the histograms follow the scalars; without scalars they stand alone
    assert summaries.encode_event(1.0, step=1, scalars=[("loss", 0.25)], histograms=[("diffuse_difference/1", h)]) == \
        _f64(1, 1.0) + _varint(2 << 3) + _varint(1) + _ld(5, scalar("loss", 0.25) + value_h)
    assert summaries.encode_event(1.0, step=1, histograms=[("diffuse_difference/1", h)]) == _f64(1, 1.0) + _varint(2 << 3) + _varint(1) + _ld(5, value_h)
    # round trip through a file
    with summaries.EventFileWriter(str(tmp_path)) as w:
        w.add_summaries(7, [("loss", 0.25), ("batch_size", 4.0)], [("diffuse_difference/1", h)], [("x_mean/1", 1.0)], wall_time=12.5)
        w.add_scalars(8, [("loss", 0.5)])
    (path,) = summaries.event_files(str(tmp_path))
    assert summaries.read_histograms(path) == [(7, "diffuse_difference/1", h)]
    assert summaries.read_scalars(path) == [(7, "loss", 0.25), (7, "batch_size", 4.0), (7, "x_mean/1", 1.0), (8, "loss", 0.5)]
    ev = summaries.read_events(path)
    assert ev[1]["tags"] == ["loss", "batch_size", "diffuse_difference/1", "x_mean/1"] and ev[2]["histograms"] == []
    records = list(R.read_records(path))
    assert bytes(records[1]) == want


def test_event_without_histograms_is_what_it_was():
    """encode_event as it was before histograms existed, restated: same arguments, same bytes."""
    def before(wall_time, step=None, file_version=None, scalars=None):
        out = summaries._key(1, 1) + struct.pack("<d", float(wall_time))
        if step is not None:
            out += summaries._key(2, 0) + R._enc_varint(int(step) & 0xFFFFFFFFFFFFFFFF)
        if file_version is not None:
            out += R._ld(3, file_version.encode("utf-8"))
        if scalars is not None:
            summary = b"".join(R._ld(1, R._ld(1, tag.encode("utf-8")) + summaries._key(2, 5) + struct.pack("<f", float(value))) for tag, value in scalars)
            out += R._ld(5, summary)
        return out
    sc = [("loss", 0.125), ("learning_rate", 1e-4), ("batch_size", 8), ("diffuse_color_mean/1", 0.3)]
    for kw in ({"step": 3, "scalars": sc}, {"file_version": summaries.FILE_VERSION}, {"step": -1, "scalars": []}, {"step": 5}):
        assert summaries.encode_event(2.5, **kw) == before(2.5, **kw)
        assert summaries.encode_event(2.5, histograms=None, **kw) == before(2.5, **kw)
        assert summaries.encode_event(2.5, histograms=[], **kw) == before(2.5, **kw)


# ---------------------------------------------------------------------------------------------------------------- merge, statistics
def test_merge_is_the_histogram_of_all_values():
    rng = np.random.default_rng(5)
    a = [rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000), np.zeros(10)]
    b = [rng.standard_normal(500), rng.random(7) + 3.0]
    ta, tb = HR.table_of([HR.Histogram(v) for v in a]), HR.table_of([HR.Histogram(v) for v in b])
    both = HR.table_of([HR.Histogram(np.concatenate([x, y])) for x, y in zip(a, b)])
    got = M.merge_histogram_tables([ta, tb])
    # the vectors train.py all-reduces (SUM, MAX) are the merge: pack, reduce, unpack
    (a1, e1), (a2, e2) = M.histogram_reduce_pack(ta), M.histogram_reduce_pack(tb)
    assert a1.dtype == e1.dtype == np.float64 and a1.size == 2 * 1551 + 8 and e1.size == 4
    by_hand = M.histogram_reduce_unpack(a1 + a2, np.maximum(e1, e2), 2, 1551)
    assert all(np.array_equal(by_hand[k], got[k]) for k in got) and by_hand["counts"].dtype == np.int64
    alone = M.histogram_reduce_unpack(a1, e1, 2, 1551)
    assert all(np.array_equal(alone[k], ta[k]) for k in ta)
    for k in ("counts", "num", "nonfinite", "min", "max"):
        assert np.array_equal(got[k], both[k]), k
    for k in ("sum", "sum_squares"):
        assert np.allclose(got[k], both[k], rtol=1e-12, atol=0)
    # with an empty one (a rank without values): min / max stay
    empty = HR.table_of([HR.Histogram(), HR.Histogram()])
    again = M.merge_histogram_tables([ta, empty])
    assert np.array_equal(again["min"], ta["min"]) and np.array_equal(again["max"], ta["max"]) and np.array_equal(again["counts"], ta["counts"])


def test_decode_records_layout():
    """The record layout of include/dd_hip.h, assembled by hand."""
    nb = 5
    off = (nb + 1) // 2 * 8
    assert off == 24
    rec = struct.pack("<5I", 1, 0, 7, 0, 2) + b"\xaa" * 4 + struct.pack("<4d", -1.0, 2.0, 3.5, 9.0) + struct.pack("<2Q", 10, 1)
    assert len(rec) == off + 48
    t = M.decode_histogram_records(np.frombuffer(rec + rec, dtype=np.uint8), 2, nb)
    assert t["counts"].tolist() == [[1, 0, 7, 0, 2]] * 2 and t["num"].tolist() == [10, 10] and t["nonfinite"].tolist() == [1, 1]
    assert (t["min"][1], t["max"][1], t["sum"][1], t["sum_squares"][1]) == (-1.0, 2.0, 3.5, 9.0)


@pytest.mark.parametrize("case", U.CASES)
def test_statistics_of_the_reference_tensors(case):
    c, tj, plan = _case(case)
    table = reference_table(c, plan, tj["loss_difference"])
    got = M.histogram_values(plan, table)
    want = GOLDEN["cases"][case]["stats"]
    assert [t for t, _ in got] == GOLDEN["cases"][case]["tags"]
    for tag, h in got:
        w = want[tag]
        assert h["num"] == w["num"] and sum(h["bucket"]) == w["num"]
        for k in ("min", "max", "sum", "sum_squares"):
            assert abs(h[k] - w[k]) <= 1e-12 * abs(w[k]), (tag, k, h[k], w[k])
