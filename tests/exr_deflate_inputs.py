"""The inputs of the device deflate's tests (TEST INFRASTRUCTURE ONLY): the enumerated list the CPU build of the coder core, the golden digests
and the GPU launch all walk, the 500 seeded random inputs of the CPU test, the corpus / result files of tests/exr_deflate_core_main.cpp, and
the size gate.

An input is what deflate sees: for the image rows the predictor output (openexr._interleave_and_predict) of a chunk's raw bytes.  `must_ok`
names the inputs the coder may not answer with RAW (zlib with Z_HUFFMAN_ONLY already brings each below 0.9 n: the test checks that);
`realistic` names the rows of the size table."""
import hashlib
import struct
import zlib

import numpy as np

from deepdenoiser_amd import openexr
from exr_device_ref import smooth

OK, RAW, RECORD = 0, 1, 2
BLOCK_TOKENS = 16384                      # DD_DEFLATE_BLOCK_TOKENS
HEADER_BYTES_PER_BLOCK = 160              # the flat code-length header: (286 + 30) * 4 bits and the fields in front


def _chunk(img, dtype):
    """the predictor output of one scan-line chunk holding all rows of img [rows, W, C]: per row, per channel, W samples"""
    a = np.asarray(img).astype(dtype)
    raw = b"".join(np.ascontiguousarray(a[r, :, c]).tobytes() for r in range(a.shape[0]) for c in range(a.shape[2]))
    return openexr._interleave_and_predict(raw)


def _text(n, seed=3):
    rng = np.random.default_rng(seed)
    words = ("the render pass of a frame is denoised tile by tile and every tile overlaps its neighbours by a border "
             "diffuse glossy transmission subsurface volume emission environment normal depth shadow ambient occlusion").split()
    out = []
    while sum(len(w) + 1 for w in out) < n:
        out.append(words[int(rng.integers(len(words)))])
    return " ".join(out).encode()[:n]


def _de_bruijn(k, order):
    """every `order`-gram over k symbols exactly once (cyclic): no substring of that length repeats"""
    a, seq = [0] * (k * order), []

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def _periodic(period, n, seed):
    block = np.random.default_rng(seed).integers(0, 16, size=period, dtype=np.uint8).tobytes()      # (16 values: Huffman alone halves it)
    return (block * (n // period + 1))[:n]


def _half_black():
    img = smooth(16, 300, 3, seed=13)
    img[:, :150] = 0.0
    return img


_CACHE = []


def enumerated():
    """[(name, bytes)] -- built once, never changed"""
    if _CACHE:
        return _CACHE
    out = []
    text = _text(20000)
    for n in (1, 2, 3, 4, 63, 64, 65, 127, 128, 129):
        out.append(("text_%d" % n, text[:n]))
    for n in (3, 258, 259, 260, 600, 70000):
        out.append(("run_%d" % n, b"\x37" * n))
    out.append(("period_2", b"ab" * 300))
    out.append(("period_7", b"abcdefg" * 100))
    out.append(("period_32768", _periodic(32768, 32768 * 2 + 300, seed=1)))
    out.append(("period_32769", _periodic(32769, 32769 * 2 + 300, seed=2)))
    out.append(("no_match", _de_bruijn(16, 3)))
    out.append(("random_64k", np.random.default_rng(4).integers(0, 256, size=1 << 16, dtype=np.uint8).tobytes()))
    out.append(("text", text))
    out.append(("smooth_half_16x37", _chunk(smooth(16, 37, 3, seed=5), np.float16)))
    out.append(("smooth_float_16x37", _chunk(smooth(16, 37, 3, seed=5), np.float32)))
    out.append(("flat_half_16x300", _chunk(np.full((16, 300, 3), 0.18, dtype=np.float32), np.float16)))
    out.append(("half_black_float_16x300", _chunk(_half_black(), np.float32)))
    out.append(("smooth_float_16x1920x4", _chunk(smooth(16, 1920, 4, seed=11), np.float32)))      # 491 520 bytes: the inflate tests' largest
    _CACHE.extend(out)
    return _CACHE


MUST_OK = ("run_258", "run_259", "run_260", "run_600", "run_70000", "period_2", "period_7", "period_32768", "period_32769", "text",
           "smooth_half_16x37", "flat_half_16x300", "half_black_float_16x300")      # (Huffman alone does not shrink the smooth FLOAT chunks: their
                                                                                     #  low mantissa bytes are noise; the size gate holds them)
MUST_RAW = ("random_64k",)
REALISTIC = ("smooth_half_16x37", "smooth_float_16x37", "flat_half_16x300", "smooth_float_16x1920x4", "text", "half_black_float_16x300")


def random_inputs(count=500, seed=17):
    """mixed run lengths and alphabets, 1 <= n <= 8192"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 8193))
        alphabet = int(rng.choice([1, 2, 3, 4, 16, 64, 256]))
        mean_run = float(rng.choice([1.0, 1.5, 4.0, 40.0, 400.0]))
        parts, have = [], 0
        while have < n:
            run = int(rng.geometric(1.0 / mean_run))
            if rng.random() < 0.15 and have > 8:                     # a copy of something earlier
                joined = b"".join(parts)
                start = int(rng.integers(0, have - 4))
                piece = joined[start:start + run + 3]
            else:
                piece = bytes([int(rng.integers(alphabet))]) * run
            parts.append(piece)
            have += len(piece)
        out.append(b"".join(parts)[:n])
    return out


def write_corpus(path, inputs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for t in inputs:
            f.write(struct.pack("<I", len(t)) + t)


def read_results(path, count):
    """-> [(status, size, stream bytes)]"""
    buf, at, out = open(path, "rb").read(), 0, []
    for _ in range(count):
        status, size = struct.unpack_from("<ii", buf, at)
        at += 8
        out.append((status, size, buf[at:at + size]))
        at += size
    assert at == len(buf)
    return out


def strict_inflate(stream, n):
    """the strict decoder's restatement (tests/exr_inflate_ref.py) -> (DD_INFLATE_* status, output bytes, number of blocks)"""
    import exr_inflate_ref as I
    out, seen = bytearray(n), I._fresh()
    try:
        I._run(bytes(stream), n, out, seen)
    except I._Stop as stop:
        return stop.status, bytes(out), len(seen["blocks"])
    return I.OK, bytes(out), len(seen["blocks"])


def size_gate(t, n_blocks):
    """zlib level 1 on the same bytes + 10 % + the flat code-length header of every block"""
    reference = len(zlib.compress(t, 1))
    return reference + reference // 10 + HEADER_BYTES_PER_BLOCK * n_blocks


def huffman_only(t):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(t) + c.flush())


def digest(status, size, stream):
    return {"status": int(status), "size": int(size), "sha256": hashlib.sha256(stream).hexdigest() if status == OK else ""}
