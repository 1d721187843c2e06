"""The decoder core of the device inflate (csrc/dd_inflate_core.h) on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer, before it
runs on a GPU: tests/exr_inflate_core_main.cpp -- a stand-alone program, not loaded into Python -- drives the core with plain byte stores
into a buffer of exactly dst_bytes over the valid list, the malformed list and the 2 000 mutations; statuses and outputs must equal the
restatement's (tests/exr_inflate_ref.py) and the sanitizers must stay silent."""
import os
import shutil
import subprocess
import zlib

import pytest

import exr_inflate_ref as I

HERE = os.path.dirname(os.path.abspath(__file__))
COMPILERS = [c for c in ("g++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    entries = [(s, len(zlib.decompress(s))) for _, s, _ in I.valid_streams()] + [(s, n) for _, s, n, _ in I.malformed_streams()] + list(I.mutations())
    path = str(tmp_path_factory.mktemp("inflate_core") / "corpus.bin")
    I.write_corpus(path, entries)
    return path, entries, [I.inflate(s, n) for s, n in entries]


def test_a_compiler_is_there():
    assert "g++" in COMPILERS


@pytest.mark.parametrize("compiler", COMPILERS)
def test_core_equals_restatement_under_sanitizers(compiler, corpus, tmp_path):
    path, entries, want = corpus
    exe, result = str(tmp_path / "core_main"), str(tmp_path / "result.bin")
    subprocess.check_call([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "exr_inflate_core_main.cpp"), "-o", exe])
    run = subprocess.run([exe, path, result], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stderr == b"", run.stderr.decode(errors="replace")[-4000:]
    have = I.read_results(result, entries)
    assert len(have) == len(want) == len(I.valid_streams()) + len(I.malformed_streams()) + 2000
    for k, (h, w) in enumerate(zip(have, want)):
        assert h[0] == w[0], "entry %d: status %d, the restatement says %d" % (k, h[0], w[0])
        assert h[1] == w[1], "entry %d: output differs (status %d)" % (k, h[0])
