"""The PNG row coder (csrc/dd_png_core.h) and the segment framing of the deflate coder core (csrc/dd_deflate_core.h) on the CPU, under
AddressSanitizer and UndefinedBehaviorSanitizer, before they run on a GPU: tests/png_core_main.cpp -- a stand-alone program, not loaded into
Python -- filters the test images (tests/png_ref.py: images()) and codes their segments, and codes the enumerated inputs of the device deflate
(tests/exr_deflate_inputs.py) cut into 2 to 5 segments, every buffer exactly sized.  The filtered bytes must equal the reference's, the
bodies behind 78 01 and in front of the combined Adler-32 must inflate to the input, every body but the last must end on the marker of an
empty stored block, RAW is allowed only where nothing is to be won, a second run gives the same bytes, the sizes are gated against zlib
level 1 and the digests against tests/golden/png_segments.json (what the GPU test compares the device with).

DD_WRITE_GOLDEN=1 rewrites the golden file and profiles/png_deflate_ratio.txt from this build instead of comparing."""
import json
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import exr_deflate_inputs as D
import exr_inflate_ref as I
import png_ref as P
from deepdenoiser_amd import png

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "png_segments.json")
RATIO = os.path.join(ROOT, "profiles", "png_deflate_ratio.txt")
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]
MARKER = b"\x00\x00\xff\xff"
MARKER_BYTES = 5                              # three bits, the padding, LEN and NLEN: what a segment that is not the last carries behind its blocks


def image_jobs():
    """the test images as jobs of the program: RGB planes have a fourth channel and a permuted channel order for every second image"""
    jobs = []
    for k, (name, image, exposure, segment_rows) in enumerate(P.images()):
        n = image.shape[2]
        if k % 2 == 1 and n == 3:
            plane = np.full(image.shape[:2] + (4,), np.float32(7.0), dtype=np.float32)
            channels = (3, 0, 2)
            for c, s in enumerate(channels):
                plane[:, :, s] = image[:, :, c]
        else:
            plane, channels = image, tuple(range(n))
        jobs.append((plane, n, channels, exposure, segment_rows))
    return jobs


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("png_core") / "corpus.bin")
    P.write_corpus(path, image_jobs(), P.byte_jobs())
    return path


@pytest.fixture(scope="module", params=COMPILERS)
def results(request, corpus, tmp_path_factory):
    """the program built with one compiler and run twice -> (results of the first run, bytes of both result files)"""
    where = tmp_path_factory.mktemp("png_core_build")
    exe = str(where / "png_core_main")
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "png_core_main.cpp"), "-o", exe])
    files = []
    for k in range(2):
        result = str(where / ("result%d.bin" % k))
        run = subprocess.run([exe, corpus, result], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert run.returncode == 0 and run.stderr == b"", run.stderr.decode(errors="replace")[-4000:]
        files.append(open(result, "rb").read())
    return P.read_results(str(where / "result0.bin"), len(P.job_names())), files


def sources(have):
    """per job (name, [the source bytes of its segments], [its segment records])"""
    out = []
    n_images = len(P.images())
    for k, (name, (filtered, segments)) in enumerate(zip(P.job_names(), have)):
        if k < n_images:
            _, image, _, segment_rows = P.images()[k]
            lengths = P.image_segment_lengths(image, segment_rows)
            data = filtered
        else:
            data, lengths = P.byte_jobs()[k - n_images]
        pieces, at = [], 0
        for n in lengths:
            pieces.append(data[at:at + n])
            at += n
        assert at == len(data) and len(pieces) == len(segments), name
        out.append((name, pieces, segments))
    return out


def coded_blocks(body, last, t):
    """the number of Huffman-coded blocks of a segment's body, by the strict decoder's restatement; the body must give t back"""
    stream = b"\x78\x01" + bytes(body) + (b"" if last else b"\x01\x00\x00\xff\xff") + zlib.adler32(t).to_bytes(4, "big")
    out, seen = bytearray(len(t)), I._fresh()
    try:
        I._run(stream, len(t), out, seen)
    except I._Stop as stop:
        assert stop.status == I.OK, "the strict decoder says %d" % stop.status
    assert bytes(out) == t
    if not last:
        assert seen["blocks"][-2:] == [0, 0] and seen["block_bytes"][-2:] == [0, 0]
    return sum(1 for kind in seen["blocks"] if kind != 0)


def test_a_compiler_is_there():
    assert "g++" in COMPILERS


def test_second_run_gives_identical_bytes(results):
    _, files = results
    assert files[0] == files[1]


def test_filtered_bytes_equal_the_reference(results):
    have, _ = results
    for (name, image, exposure, _), (filtered, _) in zip(P.images(), have):
        want = P.filtered_rows(image, exposure)
        assert filtered == want.tobytes(), name
        assert png.filtered_rows(image, exposure).tobytes() == filtered, name


def test_streams_inflate_to_the_input_and_segments_end_on_the_marker(results):
    have, _ = results
    statuses = set()
    for name, pieces, segments in sources(have):
        bodies = []
        for k, (t, (status, size, adler, body)) in enumerate(zip(pieces, segments)):
            last = k == len(pieces) - 1
            assert status in (P.OK, P.RAW), name
            assert adler == zlib.adler32(t), "%s segment %d" % (name, k)
            statuses.add(status)
            if status == P.RAW:
                bodies.append(png.stored_blocks(t, last))
                continue
            assert size == len(body) and 1 <= size < len(t), "%s segment %d: %d bytes for %d" % (name, k, size, len(t))
            if not last:
                assert body[-4:] == MARKER, "%s segment %d" % (name, k)
            bodies.append(body)
        stream = P.stream_of(bodies, [s[2] for s in segments], [len(t) for t in pieces])
        assert zlib.decompress(stream) == b"".join(pieces), name
    assert statuses == {P.OK, P.RAW}


def test_raw_only_where_allowed_and_sizes_against_zlib_level_1(results):
    have, _ = results
    raw_of = {}
    for name, pieces, segments in sources(have):
        for k, (t, (status, size, _, body)) in enumerate(zip(pieces, segments)):
            level1 = len(zlib.compress(t, 1))
            if status == P.RAW:
                raw_of[name] = raw_of.get(name, 0) + 1
                assert level1 >= 0.98 * len(t), "%s segment %d (%d bytes) is RAW, zlib level 1 makes %d" % (name, k, len(t), level1)
                continue
            blocks = coded_blocks(body, k == len(pieces) - 1, t)
            gate = D.size_gate(t, blocks) + MARKER_BYTES
            print("%s segment %d: %d bytes -> %d, zlib level 1 %d, %d blocks, gate %d" % (name, k, len(t), size, level1, blocks, gate))
            assert size <= gate, "%s segment %d: %d bytes, the gate is %d (zlib level 1: %d, %d blocks)" % (name, k, size, gate, level1, blocks)
    assert raw_of.get("image noise_rgb_64x64", 0) >= 1            # (the encoder's RAW path is taken by the GPU test of this image)
    assert "image gradient_rgb_53x67" not in raw_of and "image smooth_rgb_96x128" not in raw_of


def test_digests_equal_the_golden_file(results):
    have, _ = results
    fresh = {name: P.digest(segments) for name, (_, segments) in zip(P.job_names(), have)}
    if os.environ.get("DD_WRITE_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(fresh, f, indent=1, sort_keys=True)
            f.write("\n")
        lines = ["# image | filtered bytes | segments | RAW segments | segmented stream | zlib level 1 of the whole | zlib level 6 of the whole"]
        for (name, pieces, segments), (filtered, _) in zip(sources(have)[:len(P.images())], have):
            total = 2 + 4 + sum(size if status == P.OK else len(png.stored_blocks(t, False)) for (status, size, _, _), t in zip(segments, pieces))
            lines.append("%s | %d | %d | %d | %d | %d | %d" % (name[len("image "):], len(filtered), len(segments), sum(1 for s in segments if s[0] == P.RAW), total,
                                                             len(zlib.compress(filtered, 1)), len(zlib.compress(filtered, 6))))
        open(RATIO, "w").write("\n".join(lines) + "\n")
    assert json.load(open(GOLDEN)) == fresh
