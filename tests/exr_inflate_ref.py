"""The device inflate restated in Python, a bit writer, a block walker and the stream lists its tests read (TEST INFRASTRUCTURE ONLY).

inflate() is csrc/dd_inflate_core.h decision by decision: the same checks in the same order give the same DD_INFLATE_* status and the same
bytes in a buffer of exactly dst_bytes (0xA5 where nothing was written).  The yardstick for a stream that is OK is always zlib.decompress.

BitWriter assembles stored, fixed and dynamic blocks from given symbols and code lengths: streams zlib cannot produce (a distance of 32768,
a one-code distance set, no distance code) and the malformed ones.  walk() reports what a stream really contains, so that every entry of
valid_streams() is asserted to be what its name says.  valid_streams(), malformed_streams() and mutations() are the fixed lists the CPU and
the GPU tests walk."""
import functools
import zlib

import numpy as np

from deepdenoiser_amd import _lib, openexr

import exr_device_ref as R

OK, HEADER, TRUNCATED, BLOCK_TYPE, STORED = _lib.INFLATE_OK, _lib.INFLATE_HEADER, _lib.INFLATE_TRUNCATED, _lib.INFLATE_BLOCK_TYPE, _lib.INFLATE_STORED
LENGTHS, SYMBOL, DISTANCE, OVERRUN = _lib.INFLATE_LENGTHS, _lib.INFLATE_SYMBOL, _lib.INFLATE_DISTANCE, _lib.INFLATE_OVERRUN
SHORT, CHECK, RECORD = _lib.INFLATE_SHORT, _lib.INFLATE_CHECK, _lib.INFLATE_RECORD
FILL = 0xA5
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CODE_CLEN, CODE_LIT, CODE_DIST = 0, 1, 2


def length_code(sym):
    """literal/length symbol 257 .. 285 -> (base length, extra bits)"""
    if sym == 285:
        return 258, 0
    i = sym - 257
    if i < 8:
        return 3 + i, 0
    extra = (i >> 2) - 1
    return 3 + ((4 + (i & 3)) << extra), extra


def distance_code(sym):
    """distance symbol 0 .. 29 -> (base distance, extra bits)"""
    if sym < 4:
        return 1 + sym, 0
    extra = (sym >> 1) - 1
    return 1 + ((2 + (sym & 1)) << extra), extra


def fixed_lengths():
    return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


def canonical(lens):
    """{symbol: (code, length)} of the canonical code"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, have in enumerate(lens):
            if have == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


# ---------------------------------------------------------------------------------------------------- the restatement
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data, pos):
        self.data, self.at, self.end = data, 8 * pos, 8 * len(data)

    def need(self, n):
        if self.at + n > self.end:
            raise _Stop(TRUNCATED)

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[(self.at + k) >> 3] >> ((self.at + k) & 7)) & 1) << k
        self.at += n
        return v

    def to_byte(self):
        self.at = (self.at + 7) & ~7
        return self.at >> 3


def _build(lens, kind):
    """-> {(1 << length) | code: symbol}; the completeness rules of zlib's inflate_table"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    if count[0] == len(lens):
        if kind != CODE_DIST:
            raise _Stop(LENGTHS)
        return {}
    left, longest = 1, 0
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            raise _Stop(LENGTHS)
        if count[l]:
            longest = l
    if left > 0 and (kind == CODE_CLEN or longest != 1):
        raise _Stop(LENGTHS)
    return {(1 << l) | code: s for s, (code, l) in canonical(lens).items()}


def _decode(bits, table):
    code = 0
    for l in range(1, 16):
        bits.need(1)
        code = (code << 1) | bits.take(1)
        s = table.get((1 << l) | code)
        if s is not None:
            return s, l
    raise _Stop(SYMBOL)


def _dynamic(bits, seen):
    bits.need(14)
    nlen, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if nlen > 286 or ndist > 30:
        raise _Stop(LENGTHS)
    clens = [0] * 19
    for i in range(ncode):
        bits.need(3)
        clens[CLEN_ORDER[i]] = bits.take(3)
    clen = _build(clens, CODE_CLEN)
    lens, total = [], nlen + ndist
    while len(lens) < total:
        s, _ = _decode(bits, clen)
        if s < 16:
            lens.append(s)
            continue
        value = 0
        if s == 16:
            if not lens:
                raise _Stop(LENGTHS)
            bits.need(2)
            value, repeat = lens[-1], 3 + bits.take(2)
        elif s == 17:
            bits.need(3)
            repeat = 3 + bits.take(3)
        else:
            bits.need(7)
            repeat = 11 + bits.take(7)
        if repeat > total - len(lens):
            raise _Stop(LENGTHS)
        lens += [value] * repeat
    if lens[256] == 0:
        raise _Stop(LENGTHS)
    seen["longest_code"] = max(seen["longest_code"], max(lens))
    return _build(lens[:nlen], CODE_LIT), _build(lens[nlen:], CODE_DIST)


def _run(data, dst_bytes, out, seen):
    if len(data) < 2:
        raise _Stop(TRUNCATED)
    cmf, flg = data[0], data[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 != 0 or flg & 32:
        raise _Stop(HEADER)
    bits, produced, last = _Bits(data, 2), 0, 0
    while not last:
        bits.need(3)
        last, kind = bits.take(1), bits.take(2)
        if kind == 3:
            raise _Stop(BLOCK_TYPE)
        seen["blocks"].append(kind)
        seen["block_bytes"].append(-produced)
        if kind == 0:
            pos = bits.to_byte()
            if pos > len(data) - 4:
                raise _Stop(TRUNCATED)
            n, inverse = data[pos] | data[pos + 1] << 8, data[pos + 2] | data[pos + 3] << 8
            if n ^ inverse != 0xFFFF:
                raise _Stop(STORED)
            pos += 4
            if n > len(data) - pos:
                raise _Stop(TRUNCATED)
            if n > dst_bytes - produced:
                raise _Stop(OVERRUN)
            out[produced:produced + n] = data[pos:pos + n]
            produced += n
            bits.at = 8 * (pos + n)
            seen["block_bytes"][-1] += produced
            continue
        if kind == 1:
            lit_lens, dist_lens = fixed_lengths()
            lit, dist = _build(lit_lens, CODE_LIT), _build(dist_lens, CODE_DIST)
        else:
            lit, dist = _dynamic(bits, seen)
        while True:
            s, _ = _decode(bits, lit)
            if s < 256:
                if produced >= dst_bytes:
                    raise _Stop(OVERRUN)
                out[produced] = s
                produced += 1
                continue
            if s == 256:
                seen["block_bytes"][-1] += produced
                break
            if s > 285:
                raise _Stop(SYMBOL)
            length, extra = length_code(s)
            bits.need(extra)
            length += bits.take(extra)
            d, _ = _decode(bits, dist)
            if d > 29:
                raise _Stop(SYMBOL)
            distance, extra = distance_code(d)
            bits.need(extra)
            distance += bits.take(extra)
            if distance > produced:
                raise _Stop(DISTANCE)
            if length > dst_bytes - produced:
                raise _Stop(OVERRUN)
            start = produced - distance
            if distance >= length:
                out[produced:produced + length] = out[start:start + length]
            else:
                unit = bytes(out[start:produced])
                out[produced:produced + length] = (unit * (length // distance + 1))[:length]
            produced += length
            seen["matches"] += 1
            seen["min_distance"] = min(seen["min_distance"], distance)
            seen["max_distance"] = max(seen["max_distance"], distance)
            seen["max_length"] = max(seen["max_length"], length)
            seen["overlapping"] += distance < length
    if produced != dst_bytes:
        raise _Stop(SHORT)
    pos = bits.to_byte()
    if pos > len(data) - 4:
        raise _Stop(TRUNCATED)
    if zlib.adler32(bytes(out)) != int.from_bytes(data[pos:pos + 4], "big"):
        raise _Stop(CHECK)


def _fresh():
    return {"blocks": [], "block_bytes": [], "matches": 0, "min_distance": 1 << 30, "max_distance": 0, "max_length": 0, "overlapping": 0, "longest_code": 0}


def inflate(data, dst_bytes):
    """-> (DD_INFLATE_* status, the dst_bytes output bytes: FILL where nothing was written)"""
    out = bytearray([FILL]) * dst_bytes
    try:
        _run(bytes(data), dst_bytes, out, _fresh())
    except _Stop as stop:
        return stop.status, bytes(out)
    return OK, bytes(out)


def walk(data):
    """What a valid stream contains: {"blocks": [types], "matches", "min_distance", "max_distance", "max_length", "overlapping",
    "longest_code" (of the dynamic blocks), "block_bytes": [bytes each block adds]}."""
    size = len(zlib.decompress(data))
    seen = _fresh()
    _run(bytes(data), size, bytearray(size), seen)
    return seen


# ---------------------------------------------------------------------------------------------------- the bit writer
class BitWriter:
    def __init__(self, cmf=0x78, flg=0x9C):
        self.bytes, self.acc, self.n = bytearray([cmf, flg]), 0, 0

    def put(self, value, nbits):
        """nbits of value, least significant first"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.bytes.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):
        """a Huffman code (code, length): most significant bit first"""
        code, length = pair
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def flush(self):
        if self.n:
            self.put(0, 8 - self.n)

    def block(self, last, kind):
        self.put(last, 1)
        self.put(kind, 2)

    def stored(self, payload, last=0, inverse=None):
        self.block(last, 0)
        self.flush()
        n = len(payload)
        self.bytes += n.to_bytes(2, "little") + ((n ^ 0xFFFF) if inverse is None else inverse).to_bytes(2, "little") + bytes(payload)

    def symbols(self, symbols, lit, dist):
        """symbols: ("lit", value) | ("match", length, distance) | ("raw", literal/length symbol) | ("rawdist", distance symbol, extra bits,
        extra value) | ("end",); lit / dist: {symbol: (code, length)}"""
        for s in symbols:
            if s[0] == "lit":
                self.code(lit[s[1]])
            elif s[0] == "end":
                self.code(lit[256])
            elif s[0] == "raw":
                self.code(lit[s[1]])
            elif s[0] == "rawdist":
                self.code(dist[s[1]])
                self.put(s[3], s[2])
            else:
                _, length, distance = s
                ls = max(k for k in range(257, 286) if length_code(k)[0] <= length and (k == 285 or length < 258))
                base, extra = length_code(ls)
                self.code(lit[ls])
                self.put(length - base, extra)
                ds = max(k for k in range(30) if distance_code(k)[0] <= distance)
                base, extra = distance_code(ds)
                self.code(dist[ds])
                self.put(distance - base, extra)

    def fixed(self, symbols, last=1):
        self.block(last, 1)
        lit_lens, dist_lens = fixed_lengths()
        self.symbols(symbols, canonical(lit_lens), canonical(dist_lens))

    def dynamic_header(self, hlit, hdist, clen_lens, clen_symbols, last=1):
        """The fields as given: hlit / hdist are the 5-bit fields; clen_lens the 19 code-length code lengths (all sent, HCLEN = 15);
        clen_symbols [(symbol, extra value)] with the extra bits of 16 / 17 / 18."""
        self.block(last, 2)
        self.put(hlit, 5)
        self.put(hdist, 5)
        self.put(15, 4)
        for s in CLEN_ORDER:
            self.put(clen_lens[s], 3)
        codes = canonical(clen_lens)
        for s, extra in clen_symbols:
            self.code(codes[s])
            if s >= 16:
                self.put(extra, {16: 2, 17: 3, 18: 7}[s])

    def dynamic(self, symbols, lit_lens, dist_lens, last=1):
        """A dynamic block whose header sends every length as it is (the code-length code gives 0 .. 15 four bits each)."""
        self.dynamic_header(len(lit_lens) - 257, len(dist_lens) - 1, [4] * 16 + [0] * 3, [(l, 0) for l in list(lit_lens) + list(dist_lens)], last)
        self.symbols(symbols, canonical(lit_lens), canonical(dist_lens))

    def finish(self, expected=None, adler=None):
        self.flush()
        if adler is None:
            adler = zlib.adler32(expected)
        return bytes(self.bytes) + adler.to_bytes(4, "big")


def _lens(n, **given):
    """n lengths, zero except given s<symbol>=length"""
    out = [0] * n
    for name, l in given.items():
        out[int(name[1:])] = l
    return out


# ---------------------------------------------------------------------------------------------------- the inputs
def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def chunk_bytes():
    """the predictor bytes of the 16 x 300 RGB `smooth` chunk of exr_device_ref (what deflate sees of the file zip_16x300)"""
    img = R.smooth(16, 300, 3, seed=316)
    raw = b"".join(np.ascontiguousarray(img[r, :, c]).tobytes() for r in range(16) for c in (2, 1, 0))
    return openexr._interleave_and_predict(raw)


@functools.lru_cache(maxsize=None)
def full_chunk_bytes():
    """16 lines x 1920 x RGBA FLOAT: 491 520 bytes"""
    img = R.smooth(16, 1920, 4, seed=77)
    raw = b"".join(np.ascontiguousarray(img[r, :, c]).tobytes() for r in range(16) for c in (3, 2, 1, 0))
    return openexr._interleave_and_predict(raw)


def _fibonacci_bytes():
    fib, data = [1, 1], []
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    for i, n in enumerate(fib):
        data += [i] * n
    return bytes(np.random.default_rng(3).permutation(np.array(data, dtype=np.uint8)))


def _runs():
    rng, out = np.random.default_rng(4), bytearray()
    while len(out) < 20000:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 701))
    return bytes(out)


def _periodic(period):
    unit = bytes(np.random.default_rng(100 + period).integers(0, 256, size=period, dtype=np.uint8))
    return (unit * (3000 // period + 1))[:3000]


def _flushed(final_after_full_flush=False):
    data = chunk_bytes()
    c = zlib.compressobj(6)
    if final_after_full_flush:
        return c.compress(data) + c.flush(zlib.Z_FULL_FLUSH) + c.flush()
    out = c.compress(data[:5000]) + c.flush(zlib.Z_FULL_FLUSH) + c.flush(zlib.Z_SYNC_FLUSH)
    out += c.compress(data[5000:20000]) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.compress(data[20000:]) + c.flush()


def _distance_32768():
    head = bytes(np.random.default_rng(5).integers(0, 256, size=32768, dtype=np.uint8))
    w = BitWriter()
    w.stored(head)
    w.fixed([("match", 258, 32768), ("end",)])
    return w.finish(head + head[:258])


def _one_distance_code():
    w = BitWriter()
    w.dynamic([("lit", 97), ("match", 3, 1), ("lit", 97), ("match", 3, 1), ("end",)], _lens(258, s97=1, s256=2, s257=2), [1])
    return w.finish(b"a" * 8)


def _no_distance_code():
    w = BitWriter()
    w.dynamic([("lit", 97)] * 4 + [("end",)], _lens(257, s97=1, s256=1), [0])
    return w.finish(b"aaaa")


@functools.lru_cache(maxsize=None)
def valid_streams():
    """[(name, stream, expected: what walk() must report: a dict of exact values, of (low, high) ranges, or of the set of values a list holds)]"""
    rng = np.random.default_rng(1)
    random_5000 = bytes(rng.integers(0, 256, size=5000, dtype=np.uint8))
    random_70000 = bytes(rng.integers(0, 256, size=70000, dtype=np.uint8))
    geometric = bytes(np.minimum(rng.geometric(0.2, size=40000), 255).astype(np.uint8))
    chunk = chunk_bytes()
    fixed_literal = BitWriter()
    fixed_literal.fixed([("lit", 0x41), ("end",)])
    out = [
        ("stored_3_bytes", _deflate(b"abc", 0), {"blocks": [0], "matches": 0}),
        ("stored_two_blocks", _deflate(random_70000, 0), {"blocks": [0, 0], "matches": 0}),
        ("stored_by_level_6", _deflate(random_5000, 6), {"blocks": [0], "matches": 0}),
        ("fixed_chunk", _deflate(chunk, 6, zlib.Z_FIXED), {"blocks": {1}, "matches": (1000, 3000), "max_distance": (16384, 32768)}),
        ("fixed_one_literal", fixed_literal.finish(b"A"), {"blocks": [1], "matches": 0}),
    ]
    for level in (1, 6, 9):
        out.append(("dynamic_chunk_level_%d" % level, _deflate(chunk, level), {"blocks": {2}, "matches": (100, 10000), "longest_code": (10, 15)}))
    out += [
        ("dynamic_huffman_only", _deflate(geometric, 6, zlib.Z_HUFFMAN_ONLY), {"blocks": [2, 2, 2], "matches": 0}),
        ("dynamic_code_lengths_15", _deflate(_fibonacci_bytes(), 6, zlib.Z_HUFFMAN_ONLY), {"matches": 0, "longest_code": 15}),
        ("overlap_rle_runs", _deflate(_runs(), 6, zlib.Z_RLE), {"min_distance": 1, "max_distance": 1, "max_length": 258}),
        ("overlap_zeros", _deflate(bytes(100000), 6), {"min_distance": 1, "max_distance": 1, "max_length": 258}),
    ]
    for period in (2, 3, 5, 63, 64, 65, 127, 257):
        out.append(("overlap_period_%d" % period, _deflate(_periodic(period), 6),
                    {"min_distance": period, "max_distance": period, "max_length": 258, "matches_overlap": True}))
    out += [
        ("blocks_flushed", _flushed(), {"blocks": {0, 2}, "empty_stored": (2, 3)}),
        ("blocks_empty_final", _flushed(True), {"last_block_bytes": 0}),
        ("hand_distance_32768", _distance_32768(), {"blocks": [0, 1], "matches": 1, "min_distance": 32768, "max_distance": 32768, "max_length": 258}),
        ("hand_one_distance_code", _one_distance_code(), {"blocks": [2], "matches": 2, "max_distance": 1}),
        ("hand_no_distance_code", _no_distance_code(), {"blocks": [2], "matches": 0}),
        ("full_size_chunk", _deflate(full_chunk_bytes(), 6), {"matches": (1000, 400000)}),
    ]
    return out


def check_walk(name, stream, expected):
    """assert that walk(stream) reports what `expected` says"""
    seen = walk(stream)
    for key, want in expected.items():
        if key == "matches_overlap":                             # (all but the last, which covers the shorter rest of the input)
            assert seen["matches"] >= 10 and seen["overlapping"] >= seen["matches"] - 1, (name, seen)
        elif key == "empty_stored":
            empty = sum(1 for kind, n in zip(seen["blocks"], seen["block_bytes"]) if kind == 0 and n == 0)
            assert want[0] <= empty <= want[1], (name, seen["blocks"], seen["block_bytes"])
        elif key == "last_block_bytes":
            assert len(seen["blocks"]) >= 2 and seen["block_bytes"][-1] == want, (name, seen["block_bytes"])
        elif isinstance(want, set):
            assert set(seen[key]) == want, (name, key, seen[key])
        elif isinstance(want, tuple):
            assert want[0] <= seen[key] <= want[1], (name, key, seen[key])
        else:
            assert seen[key] == want, (name, key, seen[key])


def _small_valid():
    return [(name, s) for name, s, _ in valid_streams() if len(s) <= 600]


@functools.lru_cache(maxsize=None)
def malformed_streams():
    """[(name, stream, dst_bytes, expected status)]: each a stated edit of a valid stream or assembled with the bit writer"""
    stored_3 = _deflate(b"abc", 0)
    stored_100 = _deflate(bytes(range(100)), 0)
    zeros_100 = _deflate(bytes(100), 6)
    text = _deflate(b"the quick brown fox jumps over the lazy dog, the quick brown fox" * 4, 6)
    pad = bytes(8)

    def with_header(cmf, flg=None):
        if flg is None:
            flg = (31 - (cmf << 8) % 31) % 31
        return bytes([cmf, flg]) + stored_3[2:]

    def writer(build, tail=pad):
        w = BitWriter()
        build(w)
        w.flush()
        return bytes(w.bytes) + tail

    clen_plain = [4] * 16 + [0] * 3
    clen_repeat = _lens(19, s0=2, s1=2, s16=2, s18=2)

    def header_of(lit_lens, dist_lens=(0,)):
        def build(w):
            w.dynamic_header(len(lit_lens) - 257, len(dist_lens) - 1, clen_plain, [(l, 0) for l in list(lit_lens) + list(dist_lens)])
        return build
    out = [
        ("input_0_bytes", b"", 3, TRUNCATED),
        ("input_1_byte", b"\x78", 3, TRUNCATED),
        ("header_method_7", with_header(0x77), 3, HEADER),
        ("header_window_bits_16", with_header(0x88), 3, HEADER),
        ("header_bad_check", with_header(0x78, 0x9D), 3, HEADER),
        ("header_fdict", with_header(0x78, 0x20 | ((31 - ((0x78 << 8) | 0x20) % 31) % 31)), 3, HEADER),
        ("block_type_3", writer(lambda w: w.block(1, 3)), 3, BLOCK_TYPE),
        ("stored_len_nlen_mismatch", stored_3[:5] + bytes([stored_3[5] ^ 1]) + stored_3[6:], 3, STORED),
        ("stored_longer_than_input", stored_100[:60], 100, TRUNCATED),
        ("stored_longer_than_dst", stored_100, 50, OVERRUN),
        ("match_overruns_dst", zeros_100, 50, OVERRUN),
        ("final_block_one_byte_short", stored_100, 101, SHORT),
        ("dynamic_hlit_30", writer(lambda w: w.dynamic_header(30, 0, clen_plain, [])), 3, LENGTHS),
        ("dynamic_hdist_31", writer(lambda w: w.dynamic_header(0, 31, clen_plain, [])), 3, LENGTHS),
        ("dynamic_clen_oversubscribed", writer(lambda w: w.dynamic_header(0, 0, _lens(19, s0=1, s1=1, s2=1), [])), 3, LENGTHS),
        ("dynamic_repeat_first", writer(lambda w: w.dynamic_header(0, 0, clen_repeat, [(16, 0)])), 3, LENGTHS),
        ("dynamic_repeat_past_end", writer(lambda w: w.dynamic_header(0, 0, clen_repeat, [(18, 127), (18, 127)])), 3, LENGTHS),
        ("dynamic_no_end_of_block", writer(header_of(_lens(257, s0=1, s1=1))), 3, LENGTHS),
        ("dynamic_lit_oversubscribed", writer(header_of(_lens(257, s0=1, s1=1, s2=1, s256=1))), 3, LENGTHS),
        ("dynamic_lit_incomplete", writer(header_of(_lens(257, s0=2, s256=2))), 3, LENGTHS),
    ]
    lit_fixed = canonical(fixed_lengths()[0])
    for s in (286, 287):
        out.append(("fixed_symbol_%d" % s, writer(lambda w, s=s: w.fixed([("lit", 65), ("raw", s), ("end",)])), 3, SYMBOL))
    for s in (30, 31):
        out.append(("fixed_distance_symbol_%d" % s, writer(lambda w, s=s: w.fixed([("lit", 65), ("raw", 257), ("rawdist", s, 0, 0), ("end",)])), 8, SYMBOL))
    out += [
        ("match_first_symbol", writer(lambda w: w.fixed([("match", 3, 1), ("end",)])), 3, DISTANCE),
        ("match_distance_produced_plus_1", writer(lambda w: w.fixed([("lit", 65)] * 3 + [("match", 3, 4), ("end",)])), 6, DISTANCE),
        # 3 + 8 bits, then 5 of the 8 bits of the next literal: the input ends inside the code
        ("cut_in_symbol", writer(lambda w: (w.fixed([("lit", 65)]), w.put(lit_fixed[66][0] >> 3, 5)), tail=b""), 2, TRUNCATED),
        # the code of distance symbol 29 wants 13 extra bits; fewer than 8 follow
        ("cut_in_extra_bits", writer(lambda w: w.fixed([("lit", 65), ("raw", 257), ("rawdist", 29, 0, 0)]), tail=b""), 4, TRUNCATED),
        ("cut_in_dynamic_header", text[:7], 256, TRUNCATED),
        ("cut_in_adler", text[:-2], 256, TRUNCATED),
        ("adler_byte_flipped", text[:-1] + bytes([text[-1] ^ 0x10]), 256, CHECK),
        ("stored_payload_byte_flipped", stored_100[:20] + bytes([stored_100[20] ^ 0x01]) + stored_100[21:], 100, CHECK),
    ]
    return out


@functools.lru_cache(maxsize=None)
def mutations(n=2000, seed=9):
    """[(stream, dst_bytes)]: a byte flipped, the stream cut, or a byte inserted, over the small valid streams"""
    rng, small, out = np.random.default_rng(seed), _small_valid(), []
    for k in range(n):
        name, s = small[k % len(small)]
        size = len(zlib.decompress(s))
        b, kind, at = bytearray(s), int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        if kind == 0:
            b[at] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            del b[at:]
        else:
            b.insert(at, int(rng.integers(0, 256)))
        out.append((bytes(b), size))
    return out


# ---------------------------------------------------------------------------------------------------- the corpus file of the core program
def write_corpus(path, entries):
    """entries: [(stream, dst_bytes)] -> a file of int32 count, then per entry int32 src_bytes, int32 dst_bytes, the stream"""
    with open(path, "wb") as f:
        f.write(len(entries).to_bytes(4, "little"))
        for s, size in entries:
            f.write(len(s).to_bytes(4, "little") + size.to_bytes(4, "little") + s)


def read_results(path, entries):
    """the program's answer: per entry int32 status, then dst_bytes output bytes -> [(status, bytes)]"""
    buf, at, out = open(path, "rb").read(), 0, []
    for _, size in entries:
        out.append((int.from_bytes(buf[at:at + 4], "little"), buf[at + 4:at + 4 + size]))
        at += 4 + size
    assert at == len(buf)
    return out
