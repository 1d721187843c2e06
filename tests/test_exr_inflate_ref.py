"""The Python restatement of the device inflate (tests/exr_inflate_ref.py) against zlib, without a GPU: it is the yardstick of the statuses, so
it is itself held to zlib.decompress -- OK only where zlib agrees byte for byte, never laxer."""
import zlib

import pytest

import exr_inflate_ref as I
from deepdenoiser_amd import openexr

VALID = I.valid_streams()
MALFORMED = I.malformed_streams()


@pytest.mark.parametrize("name, stream, expected", VALID, ids=[v[0] for v in VALID])
def test_valid_stream_is_ok_and_equals_zlib(name, stream, expected):
    want = zlib.decompress(stream)
    assert I.inflate(stream, len(want)) == (I.OK, want)


@pytest.mark.parametrize("name, stream, expected", VALID, ids=[v[0] for v in VALID])
def test_valid_stream_is_what_its_name_says(name, stream, expected):
    I.check_walk(name, stream, expected)


def test_the_list_covers_what_it_must():
    walks = {name: I.walk(stream) for name, stream, _ in VALID if len(stream) < 100000}
    assert {kind for w in walks.values() for kind in w["blocks"]} == {0, 1, 2}
    assert max(w["longest_code"] for w in walks.values()) == 15
    assert max(w["max_distance"] for w in walks.values()) == 32768 and max(w["max_length"] for w in walks.values()) == 258
    assert {w["min_distance"] for w in walks.values() if w["overlapping"]} >= {1, 2, 3, 5, 63, 64, 65, 127, 257}
    sizes = [len(zlib.decompress(stream)) for _, stream, _ in VALID]
    assert min(sizes) == 1 and max(sizes) == 491520
    for name in ("hand_distance_32768", "hand_one_distance_code", "hand_no_distance_code"):      # zlib accepts the hand-assembled ones
        assert zlib.decompress(dict((n, s) for n, s, _ in VALID)[name])


@pytest.mark.parametrize("name, stream, dst_bytes, status", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_stream_has_its_status_and_zlib_refuses_it_too(name, stream, dst_bytes, status):
    assert status != I.OK and I.inflate(stream, dst_bytes)[0] == status
    try:
        size = len(zlib.decompress(stream))
    except zlib.error:
        return
    assert size != dst_bytes                     # zlib takes it: the size check of openexr._decode_chunk refuses it
    with pytest.raises(openexr.ExrError, match="chunk expands to"):
        openexr._decode_chunk(stream, openexr.ZIP_COMPRESSION, dst_bytes)


def test_malformed_list_covers_every_status_a_stream_can_have():
    assert {m[3] for m in MALFORMED} == set(range(1, 11))      # (RECORD is about the record, not the stream)


def test_mutations_terminate_and_ok_means_zlib_agrees():
    corpus = I.mutations()
    assert len(corpus) == 2000
    ok = 0
    for stream, dst_bytes in corpus:
        status, out = I.inflate(stream, dst_bytes)
        assert 0 <= status <= I.CHECK
        if status == I.OK:
            ok += 1
            assert zlib.decompress(stream) == out
    assert 0 < ok < len(corpus) // 2               # (a flipped bit in a stored length's padding, a byte inserted behind the Adler-32, ...)


def test_bytes_behind_the_adler_32_are_ignored_as_zlib_ignores_them():
    stream = VALID[0][1]
    assert zlib.decompress(stream + b"trailing") == b"abc"
    assert I.inflate(stream + b"trailing", 3) == (I.OK, b"abc")
