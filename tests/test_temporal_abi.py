"""dd_temporal_stabilize without a GPU: the ctypes mirrors of its structs against a C compile of include/dd_hip.h, the exported symbols, the
build lists, every host-side refusal (validation reads the HOST tables and fails before any launch; the device pointers are never
dereferenced), and the option rules of predict that are checked in main."""
import ctypes
import os
import re
import subprocess

import pytest

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structs_and_constants_match_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dd_hip.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_temporal_pass), offsetof(dd_temporal_pass, current), offsetof(dd_temporal_pass, history),
  offsetof(dd_temporal_pass, out), offsetof(dd_temporal_pass, current_ld), offsetof(dd_temporal_pass, history_ld), offsetof(dd_temporal_pass, out_ld),
  offsetof(dd_temporal_pass, nch));
  printf(" %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_temporal_guide), offsetof(dd_temporal_guide, current), offsetof(dd_temporal_guide, previous),
  offsetof(dd_temporal_guide, current_ld), offsetof(dd_temporal_guide, previous_ld), offsetof(dd_temporal_guide, nch), offsetof(dd_temporal_guide, tolerance));
  printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(dd_temporal_record), offsetof(dd_temporal_record, pixels_offscreen), offsetof(dd_temporal_record, pixels_guide),
  offsetof(dd_temporal_record, pixels_nonfinite), offsetof(dd_temporal_record, pixels_blended), offsetof(dd_temporal_record, values_clamped),
  offsetof(dd_temporal_record, change), offsetof(dd_temporal_record, flicker_before), offsetof(dd_temporal_record, flicker_after));
  printf(" %d %d %d\n", DD_TEMPORAL_MAX_PASSES, DD_TEMPORAL_MAX_GUIDES, DD_TEMPORAL_TILE); return 0; }
'''
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P, G, R = _lib.TemporalPass, _lib.TemporalGuide, _lib.TemporalRecord
    assert have[:8] == [ctypes.sizeof(P), P.current.offset, P.history.offset, P.out.offset, P.current_ld.offset, P.history_ld.offset, P.out_ld.offset,
                        P.nch.offset] == [40, 0, 8, 16, 24, 28, 32, 36]
    assert have[8:15] == [ctypes.sizeof(G), G.current.offset, G.previous.offset, G.current_ld.offset, G.previous_ld.offset, G.nch.offset,
                          G.tolerance.offset] == [32, 0, 8, 16, 20, 24, 28]
    assert have[15:24] == [ctypes.sizeof(R)] + [getattr(R, name).offset for name, _ in R._fields_] == [64, 0, 8, 16, 24, 32, 40, 48, 56]
    assert have[24:] == [_lib.TEMPORAL_MAX_PASSES, _lib.TEMPORAL_MAX_GUIDES, _lib.TEMPORAL_TILE] and have[24:26] == [32, 4]


def test_symbols_are_declared_built_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    for name in ("dd_temporal_stabilize", "dd_temporal_scratch_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint dd_temporal_stabilize\(const dd_temporal_pass\* passes, int n_passes, const dd_temporal_guide\* guides, int n_guides, int H, int W,", header)
    assert re.search(r"\blong dd_temporal_scratch_bytes\(int n_passes, int H, int W\);", header)
    comment = header[header.index("(csrc/dd_temporal.hip)"):header.index("#define DD_TEMPORAL_MAX_PASSES")]
    for word in ("The reference has no such step", "offscreen takes precedence", "bit for bit", "Refused with a negative status", "No host sync"):
        assert word in comment, word
    from deepdenoiser_amd import build
    assert "dd_temporal.hip" in build.SOURCES
    assert build.NO_SCRATCH["dd_temporal.hip"] == ("temporal_stabilize_kernel", "temporal_finalize_kernel")
    source = open(os.path.join(build.CSRC, "dd_temporal.hip")).read()
    assert "asm" not in source.replace("assembly", "") and "atomic" not in source.replace("No atomics", "").replace("floating-point atomics", "")
    T = _lib.TEMPORAL_TILE
    tiles = lambda n: (n + T - 1) // T                                              # noqa: E731
    assert lib.dd_temporal_scratch_bytes(15, 1080, 1920) == 15 * tiles(1080) * tiles(1920) * 64
    assert lib.dd_temporal_scratch_bytes(1, 1, 1) == 64
    for bad in ((0, 4, 4), (33, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.dd_temporal_scratch_bytes(*bad) < 0 and b"dd_temporal_scratch_bytes" in lib.dd_last_error()


def test_host_side_refusals(lib):
    """every pointer is a fake address: a call that got as far as a launch, or read one of them, would not return a clean negative status"""
    fake = lambda k: k << 20                                                        # noqa: E731
    motion, records, scratch = fake(1), fake(2), fake(3)

    def tables(n=2, g=1):
        passes = (_lib.TemporalPass * max(n, 1))()
        for k, p in enumerate(passes):
            p.current, p.history, p.out, p.current_ld, p.history_ld, p.out_ld, p.nch = fake(10 + 3 * k), fake(11 + 3 * k), fake(12 + 3 * k), 3, 3, 3, 3 if k % 2 == 0 else 1
        guides = (_lib.TemporalGuide * max(g, 1))()
        for k, q in enumerate(guides):
            q.current, q.previous, q.current_ld, q.previous_ld, q.nch, q.tolerance = fake(200 + 2 * k), fake(201 + 2 * k), 3, 3, 3, 0.25
        return passes, guides

    def call(passes, guides, n=2, g=1, H=20, W=30, mv=motion, motion_ld=3, sx=-1.0, sy=1.0, alpha=0.8, gamma=1.0, rec=records, scr=scratch):
        return lib.dd_temporal_stabilize(passes, n, guides, g, H, W, mv, motion_ld, sx, sy, alpha, gamma, rec, scr, None)

    def refused(word, change=None, **k):
        passes, guides = tables(max(k.get("n", 2), 2), max(k.get("g", 1), 1))
        if change:
            change(passes, guides)
        assert call(passes, guides, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()

    def setter(what, index, field, value):
        def change(passes, guides):
            setattr((passes if what == "pass" else guides)[index], field, value)
        return change
    passes, guides = tables()
    assert call(None, guides) < 0 and b"null pass table" in lib.dd_last_error()
    assert call(passes, None) < 0 and b"null guide table" in lib.dd_last_error()
    for n in (0, -1, 33):
        refused(b"n_passes = %d" % n, n=n)
    for g in (-1, 5):
        refused(b"n_guides = %d" % g, g=g)
    refused(b"bad shape", H=0)
    refused(b"bad shape", W=0)
    refused(b"bad shape", W=-3)
    refused(b"motion is null", mv=None)
    refused(b"aligned", mv=fake(1) + 2)
    for ld in (1, 0, -2):
        refused(b"motion_ld = %d" % ld, motion_ld=ld)
    for alpha in (-0.01, 1.01, float("nan"), float("inf")):
        refused(b"alpha", alpha=alpha)
    for gamma in (-0.5, float("nan"), float("inf")):
        refused(b"gamma", gamma=gamma)
    refused(b"motion scale", sx=float("nan"))
    refused(b"motion scale", sy=float("-inf"))
    refused(b"records is null", rec=None)
    refused(b"records is null or not 8-byte aligned", rec=fake(2) + 4)
    refused(b"scratch is null", scr=None)
    refused(b"scratch is null or not 8-byte aligned", scr=fake(3) + 4)
    for field in ("current", "history", "out"):
        refused(b"pass 1 has a null", setter("pass", 1, field, None))
        refused(b"pass 0 is not 4-byte aligned", setter("pass", 0, field, fake(50) + 1))
    for nch in (0, 2, 4, -1):
        refused(b"pass 1 has %d channels" % nch, setter("pass", 1, "nch", nch))
    for field in ("current_ld", "history_ld", "out_ld"):
        refused(b"pass 0 has a pixel stride", setter("pass", 0, field, 2))
    refused(b"out of pass 0 is current or history of pass 0", setter("pass", 0, "out", fake(10)))          # in place
    refused(b"out of pass 0 is current or history of pass 0", setter("pass", 0, "out", fake(11)))
    refused(b"out of pass 1 is current or history of pass 0", setter("pass", 1, "out", fake(11)))          # across the passes of the call
    refused(b"out of pass 0 is current or history of pass 1", setter("pass", 0, "out", fake(13)))
    for field in ("current", "previous"):
        refused(b"guide 0 has a null", setter("guide", 0, field, None))
        refused(b"guide 0 is not 4-byte aligned", setter("guide", 0, field, fake(60) + 2))
    refused(b"guide 0 has 2 channels", setter("guide", 0, "nch", 2))
    refused(b"guide 0 has a pixel stride", setter("guide", 0, "previous_ld", 1))
    for tolerance in (-1.0, float("nan"), float("inf")):
        refused(b"guide 0 has tolerance", setter("guide", 0, "tolerance", tolerance))
    refused(b"guide 3 has 0 channels", setter("guide", 3, "nch", 0), g=4)


def test_predict_option_rules_are_checked_in_main(capsys):
    from deepdenoiser_amd import predict
    parser = predict.parser()
    args = parser.parse_args(["a.json"])                                            # what existing tests parse: no --input, and it must keep parsing
    assert (args.temporal, args.input, args.input_sequence) == (False, None, None)
    assert (args.temporal_alpha, args.temporal_gamma, args.motion_scale, args.temporal_guide) == (None, None, None, None)
    args = parser.parse_args(["a.json", "--input_sequence", "shots", "--temporal", "--temporal_alpha", "0.5", "--temporal_gamma", "2", "--motion_scale", "1", "-1",
                              "--temporal_guide", "Normal:0.25", "--temporal_guide", "Depth:0.1"])
    assert (args.temporal, args.temporal_alpha, args.temporal_gamma, args.motion_scale, args.temporal_guide) == (True, 0.5, 2.0, [1.0, -1.0], ["Normal:0.25", "Depth:0.1"])
    assert predict.check_option_rules(args) is None
    for extra, text in (([], "exactly one of --input / --input_sequence must be given"),
                        (["--input", "a", "--input_sequence", "b"], "exactly one of --input / --input_sequence must be given"),
                        (["--input", "a", "--temporal"], "--temporal and its options need --input_sequence"),
                        (["--input", "a", "--temporal_alpha", "0.5"], "--temporal and its options need --input_sequence"),
                        (["--input", "a", "--motion_scale", "1", "1"], "--temporal and its options need --input_sequence"),
                        (["--input", "a", "--temporal_guide", "Normal:1"], "--temporal and its options need --input_sequence"),
                        (["--input_sequence", "b", "--temporal_gamma", "2"], "--temporal_gamma needs --temporal"),
                        (["--input_sequence", "b", "--target", "t"], "--target needs --input (scoring sequences is out of scope)")):
        with pytest.raises(SystemExit) as e:
            predict.main(parser.parse_args(["does_not_exist.json"] + extra))        # (the rules come before anything is opened)
        assert str(e.value) == text
    for option in ("--input_sequence", "--temporal", "--temporal_alpha", "--temporal_gamma", "--motion_scale", "--temporal_guide"):
        assert option in parser.format_help()
