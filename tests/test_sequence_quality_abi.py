"""dd_sequence_quality without a GPU: the ctypes mirrors of its structs against a C compile of include/dd_hip.h, the exported symbols, the build
lists, every host-side refusal (validation reads the HOST table and fails before any launch; the device pointers are never dereferenced),
and the option rules of predict around --target_sequence."""
import ctypes
import os
import re
import subprocess

import pytest

from deepdenoiser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structs_and_constants_match_header(tmp_path):
    pair = ("pred", "pred_previous", "target", "target_previous", "pred_ld", "pred_previous_ld", "target_ld", "target_previous_ld", "nch")
    rec = ("pixels_offscreen", "pixels_nonfinite", "pixels_valid", "change_prediction", "change_target", "temporal_error", "ldr_change_prediction",
           "ldr_change_target", "ldr_temporal_error")
    lines = ['printf("%zu ", sizeof(dd_seqq_pair));'] + ['printf("%%zu ", offsetof(dd_seqq_pair, %s));' % f for f in pair]
    lines += ['printf("%zu ", sizeof(dd_seqq_record));'] + ['printf("%%zu ", offsetof(dd_seqq_record, %s));' % f for f in rec]
    lines += ['printf("%d %d\\n", DD_SEQQ_MAX_PAIRS, DD_SEQQ_TILE);']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dd_hip.h"\nint main(void){ %s return 0; }\n' % " ".join(lines)
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    have = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    P, R = _lib.SequenceQualityPair, _lib.SequenceQualityRecord
    assert [name for name, _ in P._fields_] == list(pair) and [name for name, _ in R._fields_] == list(rec)
    assert have[:10] == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in pair] == [56, 0, 8, 16, 24, 32, 36, 40, 44, 48]
    assert have[10:20] == [ctypes.sizeof(R)] + [getattr(R, f).offset for f in rec] == [72] + [8 * k for k in range(9)]
    assert have[20:] == [_lib.SEQQ_MAX_PAIRS, _lib.SEQQ_TILE] and have[20] == 32


def test_symbols_are_declared_built_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "dd_hip.h")).read()
    for name in ("dd_sequence_quality", "dd_sequence_quality_scratch_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint dd_sequence_quality\(const dd_seqq_pair\* pairs, int n_pairs, int H, int W, const float\* motion, int motion_ld, float sx, float sy,", header)
    assert re.search(r"\blong dd_sequence_quality_scratch_bytes\(int n_pairs, int H, int W\);", header)
    comment = header[header.index("(csrc/dd_sequence_quality.hip)"):header.index("#define DD_SEQQ_MAX_PAIRS")]
    for word in ("offscreen takes precedence", "a tap with weight 0 still counts", "they add up to H * W", "Refused with a negative status", "No host sync"):
        assert word in comment, word
    from deepdenoiser_amd import build
    assert "dd_sequence_quality.hip" in build.SOURCES and "dd_frame_common.h" in build.HEADERS and "dd_motion.h" not in build.HEADERS
    assert build.NO_SCRATCH["dd_sequence_quality.hip"] == ("sequence_quality_kernel", "sequence_quality_finalize_kernel")
    source = open(os.path.join(build.CSRC, "dd_sequence_quality.hip")).read()
    assert '#include "dd_frame_common.h"' in source and "dd_motion_previous(" in source
    assert "asm" not in source.replace("assembly", "") and "atomic" not in source.replace("No atomics", "").replace("floating-point atomics", "")
    stabiliser = open(os.path.join(build.CSRC, "dd_temporal.hip")).read()                # the stabiliser compiles the same function: one rule
    assert '#include "dd_frame_common.h"' in stabiliser and "dd_motion_previous(" in stabiliser and "floorf(px)" not in stabiliser
    assert not os.path.exists(os.path.join(build.CSRC, "dd_motion.h"))
    T = _lib.SEQQ_TILE
    tiles = lambda n: (n + T - 1) // T                                              # noqa: E731
    assert lib.dd_sequence_quality_scratch_bytes(15, 1080, 1920) == 15 * tiles(1080) * tiles(1920) * 72
    assert lib.dd_sequence_quality_scratch_bytes(1, 1, 1) == 72
    for bad in ((0, 4, 4), (33, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert lib.dd_sequence_quality_scratch_bytes(*bad) < 0 and b"dd_sequence_quality_scratch_bytes" in lib.dd_last_error()


def test_host_side_refusals(lib):
    """every pointer is a fake address: a call that got as far as a launch, or read one of them, would not return a clean negative status"""
    fake = lambda k: k << 20                                                        # noqa: E731
    motion, thresholds, records, scratch = fake(1), fake(2), fake(3), fake(4)
    images = ("pred", "pred_previous", "target", "target_previous")

    def table(n=2):
        pairs = (_lib.SequenceQualityPair * max(n, 1))()
        for k, p in enumerate(pairs):
            p.pred, p.pred_previous, p.target, p.target_previous = (fake(10 + 4 * k + j) for j in range(4))
            p.pred_ld, p.pred_previous_ld, p.target_ld, p.target_previous_ld, p.nch = 3, 3, 5, 3, 3 if k % 2 == 0 else 1
        return pairs

    def call(pairs, n=2, H=20, W=30, mv=motion, motion_ld=3, sx=-1.0, sy=1.0, thr=thresholds, exposure=1.0, rec=records, scr=scratch):
        return lib.dd_sequence_quality(pairs, n, H, W, mv, motion_ld, sx, sy, thr, exposure, rec, scr, None)

    def refused(word, change=None, **k):
        pairs = table(max(k.get("n", 2), 2))
        if change:
            change(pairs)
        assert call(pairs, **k) < 0
        assert word in lib.dd_last_error(), lib.dd_last_error()

    def setter(index, field, value):
        def change(pairs):
            setattr(pairs[index], field, value)
        return change
    assert call(None) < 0 and b"null pair table" in lib.dd_last_error()
    for n in (0, -1, 33):
        refused(b"n_pairs = %d" % n, n=n)
    refused(b"bad shape", H=0)
    refused(b"bad shape", W=0)
    refused(b"bad shape", H=-3)
    refused(b"motion is null", mv=None)
    refused(b"motion is null or not 4-byte aligned", mv=fake(1) + 2)
    for ld in (1, 0, -2):
        refused(b"motion_ld = %d" % ld, motion_ld=ld)
    refused(b"motion scale is not finite", sx=float("nan"))
    refused(b"motion scale is not finite", sy=float("-inf"))
    refused(b"thresholds is null", thr=None)
    for exposure in (float("nan"), float("inf"), float("-inf")):
        refused(b"exposure is not finite", exposure=exposure)
    refused(b"records is null", rec=None)
    refused(b"records is null or not 8-byte aligned", rec=fake(3) + 4)
    refused(b"scratch is null", scr=None)
    refused(b"scratch is null or not 8-byte aligned", scr=fake(4) + 4)
    for field in images:
        refused(b"pair 1 has a null", setter(1, field, None))
        refused(b"pair 0 is not 4-byte aligned", setter(0, field, fake(50) + 1))
        refused(b"pair 31 is not 4-byte aligned", setter(31, field, fake(50) + 2), n=32)
    for nch in (0, 2, 4, -1):
        refused(b"pair 1 has %d channels" % nch, setter(1, "nch", nch))
    for field in images:
        refused(b"pair 0 has a pixel stride", setter(0, field + "_ld", 2))
        refused(b"pair 1 has a pixel stride", setter(1, field + "_ld", 0))


def test_predict_option_rules_around_target_sequence():
    from deepdenoiser_amd import predict
    parser = predict.parser()
    args = parser.parse_args(["a.json"])                                            # what existing tests parse: it must keep parsing
    assert (args.target_sequence, args.sequence_quality_json, args.input, args.input_sequence) == (None, None, None, None)
    rules = lambda extra: predict.check_option_rules(parser.parse_args(["a.json"] + extra))      # noqa: E731
    assert rules(["--input", "a", "--target_sequence", "t"]) == "--target_sequence needs --input_sequence"
    assert rules(["--input_sequence", "b", "--target", "t"]) == "--target needs --input (scoring sequences is out of scope)"
    assert rules(["--input_sequence", "b", "--target_sequence", "t"]) is None
    assert rules(["--input_sequence", "b", "--target_sequence", "t", "--motion_scale", "1", "-1"]) is None
    assert rules(["--input_sequence", "b", "--target_sequence", "t", "--temporal", "--motion_scale", "1", "-1", "--sequence_quality_json", "q.json"]) is None
    assert rules(["--input_sequence", "b", "--motion_scale", "1", "-1"]) == "--motion_scale needs --temporal"
    assert rules(["--input_sequence", "b", "--target_sequence", "t", "--temporal_alpha", "0.5"]) == "--temporal_alpha needs --temporal"
    assert rules(["--input", "a", "--motion_scale", "1", "1"]) == "--temporal and its options need --input_sequence"
    with pytest.raises(SystemExit) as e:
        predict.main(parser.parse_args(["does_not_exist.json", "--input", "a", "--target_sequence", "t"]))      # (the rules come before anything is opened)
    assert str(e.value) == "--target_sequence needs --input_sequence"
    for option in ("--target_sequence", "--sequence_quality_json"):
        assert option in parser.format_help()
