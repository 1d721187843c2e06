"""The coder core of the device deflate (csrc/dd_deflate_core.h) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, before it runs
on a GPU: tests/exr_deflate_core_main.cpp -- a stand-alone program, not loaded into Python -- runs the core, its 64 lanes as a loop, over the
enumerated inputs (tests/exr_deflate_inputs.py) and 500 seeded random ones, every stream into a heap buffer of exactly dst_capacity = n - 1
bytes and a workspace of exactly its size.  zlib and the strict decoder's restatement (tests/exr_inflate_ref.py) must give the input back,
RAW is allowed only where nothing is to be won, a second run gives the same bytes, the sizes are gated against zlib level 1 and the digests
against tests/golden/exr_deflate_streams.json (what the GPU test compares the device with).

DD_WRITE_GOLDEN=1 rewrites the golden file and profiles/exr_deflate_ratio.txt from this build instead of comparing."""
import json
import os
import shutil
import subprocess
import zlib

import pytest

import exr_deflate_inputs as D
import exr_inflate_ref as I

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "exr_deflate_streams.json")
RATIO = os.path.join(ROOT, "profiles", "exr_deflate_ratio.txt")
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    inputs = [t for _, t in D.enumerated()] + D.random_inputs()
    path = str(tmp_path_factory.mktemp("deflate_core") / "corpus.bin")
    D.write_corpus(path, inputs)
    return path, inputs


@pytest.fixture(scope="module", params=COMPILERS)
def results(request, corpus, tmp_path_factory):
    """the program built with one compiler and run twice -> (inputs, results of the first run, bytes of both result files)"""
    path, inputs = corpus
    where = tmp_path_factory.mktemp("deflate_core_build")
    exe = str(where / "core_main")
    subprocess.check_call([request.param, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "exr_deflate_core_main.cpp"), "-o", exe])
    files = []
    for k in range(2):
        result = str(where / ("result%d.bin" % k))
        run = subprocess.run([exe, path, result], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert run.returncode == 0 and run.stderr == b"", run.stderr.decode(errors="replace")[-4000:]
        files.append(open(result, "rb").read())
    return inputs, D.read_results(str(where / "result0.bin"), len(inputs)), files


def test_a_compiler_is_there():
    assert "g++" in COMPILERS


def test_the_named_inputs_may_not_be_raw_because_huffman_alone_shrinks_them():
    by_name = dict(D.enumerated())
    for name in D.MUST_OK:
        assert D.huffman_only(by_name[name]) < 0.9 * len(by_name[name]), name


def test_second_run_gives_identical_bytes(results):
    _, _, files = results
    assert files[0] == files[1]


def test_every_stream_inflates_to_its_input(results):
    inputs, have, _ = results
    n_enumerated = len(D.enumerated())
    assert len(have) == n_enumerated + 500
    for k, (t, (status, size, stream)) in enumerate(zip(inputs, have)):
        name = D.enumerated()[k][0] if k < n_enumerated else "random %d" % (k - n_enumerated)
        assert status in (D.OK, D.RAW), name
        if status == D.RAW:
            continue
        assert size == len(stream) and size < len(t), "%s: %d bytes for %d" % (name, size, len(t))
        assert zlib.decompress(stream) == t, name
        strict, out, _ = D.strict_inflate(stream, len(t))
        assert strict == I.OK and out == t, "%s: the strict decoder says %d" % (name, strict)


def test_raw_only_where_allowed(results):
    inputs, have, _ = results
    enumerated = D.enumerated()
    status_of = {name: have[k][0] for k, (name, _) in enumerate(enumerated)}
    for name in D.MUST_OK:
        assert status_of[name] == D.OK, name
    for name in D.MUST_RAW:
        assert status_of[name] == D.RAW, name
    for k in range(len(enumerated), len(inputs)):
        if have[k][0] == D.RAW:
            t = inputs[k]
            assert len(zlib.compress(t, 1)) >= 0.98 * len(t), "random %d (%d bytes) is RAW, zlib level 1 makes %d" % (k - len(enumerated), len(t),
                                                                                                                      len(zlib.compress(t, 1)))


def _table(have):
    lines = ["# input | raw bytes | device deflate | zlib level 1 | zlib level 6 | blocks | gate (level 1 + 10 % + 160 per block)"]
    rows = []
    for k, (name, t) in enumerate(D.enumerated()):
        if name in D.REALISTIC:
            status, size, stream = have[k]
            blocks = D.strict_inflate(stream, len(t))[2] if status == D.OK else 0
            rows.append((name, len(t), status, size, len(zlib.compress(t, 1)), len(zlib.compress(t, 6)), blocks, D.size_gate(t, blocks)))
            lines.append("%s | %d | %d | %d | %d | %d | %d" % (rows[-1][:2] + rows[-1][3:]))
    return rows, "\n".join(lines) + "\n"


def test_sizes_against_zlib_level_1(results):
    _, have, _ = results
    rows, text = _table(have)
    print(text)
    assert len(rows) == len(D.REALISTIC)
    if os.environ.get("DD_WRITE_GOLDEN") == "1":
        open(RATIO, "w").write(text)
    for name, n, status, size, level1, level6, blocks, gate in rows:
        assert status == D.OK and size <= gate, "%s: %d bytes, the gate is %d (zlib level 1: %d, %d blocks)" % (name, size, gate, level1, blocks)
    recorded = [line.split(" | ")[:3] for line in open(RATIO).read().splitlines()[1:]]      # (the zlib columns depend on the zlib at hand)
    assert recorded == [[name, str(n), str(size)] for name, n, _, size, _, _, _, _ in rows], "profiles/exr_deflate_ratio.txt is not this build's table"


def test_digests_equal_the_golden_file(results):
    _, have, _ = results
    fresh = {name: D.digest(*have[k]) for k, (name, _) in enumerate(D.enumerated())}
    if os.environ.get("DD_WRITE_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(fresh, f, indent=1, sort_keys=True)
            f.write("\n")
    assert json.load(open(GOLDEN)) == fresh
