// The inflate decoder core shared by the device kernel (dd_exr_inflate.hip) and a stand-alone host program (tests/exr_inflate_core_main.cpp):
// everything that decides an ADDRESS or a STATUS of dd_exr_inflate (include/dd_hip.h) lives here, as functions that compile for the host
// and for the device from the same text, so the same decisions run on the CPU under sanitizers before they run on a GPU.
//   - the zlib header (RFC 1950), the bounded bit reader, stored-block parsing,
//   - dynamic-header parsing and canonical code construction with zlib's completeness rules,
//   - symbol, length and distance decode; the loop that turns a stream into literal / stored / match / check calls of a Sink.
// The caller supplies where the tables live (a dd_inflate_tables; the kernel keeps one in LDS) and a Sink that says how bytes are stored,
// copied and summed:
//     void     literal(int at, unsigned value)                      out[at] = value
//     void     stored(int at, const unsigned char* from, int n)     out[at .. at + n) = from[0 .. n)
//     void     match(int at, int distance, int length)              out[at + i] = out[at - distance + i % distance], i < length
//     unsigned adler(int n)                                          Adler-32 of out[0 .. n)
// Guarantees towards the Sink: every `at + n` / `at + length` is <= dst_bytes, every `from` range lies inside the source, distance <= at.
// Every loop is bounded by bits consumed or bytes produced: a symbol takes at least one bit, a block at least three, and nothing is read
// past src_bytes, so no malformed stream can spin.  The decoder may be stricter than zlib, never laxer.
#ifndef DD_INFLATE_CORE_H
#define DD_INFLATE_CORE_H

#include "../../include/dd_hip.h"

#if defined(__HIPCC__)
#define DD_HD __host__ __device__ __forceinline__
#else
#define DD_HD inline
#endif

#define DD_INFLATE_LIT_BITS 9        // primary lookup of the literal/length code
#define DD_INFLATE_DIST_BITS 8       // ... of the distance code
#define DD_INFLATE_MAX_BITS 15
#define DD_INFLATE_LIT_SYMBOLS 288   // the fixed code has 288 literal/length symbols (286 and 287 never valid) and 32 distance symbols
#define DD_INFLATE_DIST_SYMBOLS 32
#define DD_INFLATE_CLEN_SYMBOLS 19

// One stream's code tables.  A primary table entry is (symbol << 4) | code length, 0 where no code of at most that many bits matches; codes
// longer than the primary index are found through the canonical count / symbol arrays.  Small dynamically indexed arrays all live here
// (LDS on the device), none in registers.
struct dd_inflate_tables {
  unsigned short lit_fast[1 << DD_INFLATE_LIT_BITS];
  unsigned short dist_fast[1 << DD_INFLATE_DIST_BITS];
  unsigned short lit_sym[DD_INFLATE_LIT_SYMBOLS];
  unsigned short dist_sym[DD_INFLATE_DIST_SYMBOLS];
  unsigned short clen_sym[DD_INFLATE_CLEN_SYMBOLS + 1];
  unsigned short lit_count[DD_INFLATE_MAX_BITS + 1];
  unsigned short dist_count[DD_INFLATE_MAX_BITS + 1];
  unsigned short clen_count[DD_INFLATE_MAX_BITS + 1];
  unsigned short offs[DD_INFLATE_MAX_BITS + 1];
  unsigned char lens[DD_INFLATE_LIT_SYMBOLS + DD_INFLATE_DIST_SYMBOLS];
};

// ---------------------------------------------------------------------------------------------------- the bit reader
// Bits are taken from the low end of `hold`; pos is the next unread source byte.  Every source read is checked against n.
struct dd_bits {
  const unsigned char* src;
  int n, pos, nbits;
  unsigned long long hold;
};

// One aligned word of the source.  On the device the source is read-only for the whole launch, so the word is loaded through the constant
// address space: a wave-uniform load from there is a scalar load, which waits neither for the wave's outstanding byte stores nor for a
// vector memory round trip (the compiler does not prove that by itself in a function with this many stores).
DD_HD unsigned dd_load_word(const unsigned char* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const unsigned __attribute__((address_space(4))) * constant_words;
  return *reinterpret_cast<constant_words>(reinterpret_cast<unsigned long long>(p));
#else
  unsigned w;
  __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);      // (little-endian hosts)
  return w;
#endif
}

// Fill `hold` as far as it goes: single bytes up to the next 4-byte aligned source address (and over the last three bytes of the source),
// whole aligned words in between (dd_load_word).  Afterwards at least 16 bits are there unless the source is exhausted.
DD_HD void dd_bits_refill(dd_bits& b) {
  while (b.nbits <= 56 && b.pos < b.n && (((unsigned long long)(b.src + b.pos) & 3ull) != 0ull || b.pos > b.n - 4)) {      // at most 8 rounds
    b.hold |= (unsigned long long)b.src[b.pos++] << b.nbits;
    b.nbits += 8;
  }
  if (b.nbits <= 32 && b.pos <= b.n - 4 && ((unsigned long long)(b.src + b.pos) & 3ull) == 0ull) {
    b.hold |= (unsigned long long)dd_load_word(b.src + b.pos) << b.nbits;
    b.pos += 4;
    b.nbits += 32;
  }
}

// true when n (<= 16) bits are there
DD_HD bool dd_bits_need(dd_bits& b, int n) {
  if (b.nbits < n) dd_bits_refill(b);
  return b.nbits >= n;
}

DD_HD unsigned dd_bits_take(dd_bits& b, int n) {
  const unsigned v = (unsigned)(b.hold & ((1ull << n) - 1ull));
  b.hold >>= n;
  b.nbits -= n;
  return v;
}

// drop the rest of the current byte and hand the whole bytes still held back to the source: pos is the next byte of the stream
DD_HD void dd_bits_to_byte(dd_bits& b) {
  b.nbits -= b.nbits & 7;
  b.pos -= b.nbits >> 3;
  b.nbits = 0;
  b.hold = 0ull;
}

// ---------------------------------------------------------------------------------------------------- the zlib header
DD_HD int dd_zlib_header(const unsigned char* src, int src_bytes) {
  if (src_bytes < 2) return DD_INFLATE_TRUNCATED;
  const unsigned cmf = src[0], flg = src[1];
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u) != 0u) return DD_INFLATE_HEADER;
  return DD_INFLATE_OK;
}

// ---------------------------------------------------------------------------------------------------- codes
struct dd_huff {
  unsigned short* count;      // [16]: codes per length
  unsigned short* sym;        // symbols in canonical order
  unsigned short* fast;       // primary table, or null
  int fast_bits;
};

enum { DD_CODE_CLEN = 0, DD_CODE_LIT = 1, DD_CODE_DIST = 2 };

// Canonical code of lens[0 .. n).  The rules are those of zlib's inflate_table: an over-subscribed set is refused; an incomplete one too,
// except a set whose only code has one bit (libdeflate writes such distance codes) -- never for the code-length code; a set with no code
// at all is accepted for distances only (a block of literals) and then decodes nothing.
DD_HD int dd_huff_build(const dd_huff& h, const unsigned char* lens, int n, unsigned short* offs, int kind) {
  for (int l = 0; l <= DD_INFLATE_MAX_BITS; ++l) h.count[l] = 0;
  for (int i = 0; i < n; ++i) h.count[lens[i]]++;
  if (h.fast)
    for (int j = 0; j < (1 << h.fast_bits); ++j) h.fast[j] = 0;
  if (h.count[0] == n) return kind == DD_CODE_DIST ? DD_INFLATE_OK : DD_INFLATE_LENGTHS;
  int left = 1, longest = 0;
  for (int l = 1; l <= DD_INFLATE_MAX_BITS; ++l) {
    left = (left << 1) - (int)h.count[l];
    if (left < 0) return DD_INFLATE_LENGTHS;
    if (h.count[l] != 0) longest = l;
  }
  if (left > 0 && (kind == DD_CODE_CLEN || longest != 1)) return DD_INFLATE_LENGTHS;
  offs[1] = 0;
  for (int l = 1; l < DD_INFLATE_MAX_BITS; ++l) offs[l + 1] = (unsigned short)(offs[l] + h.count[l]);
  for (int i = 0; i < n; ++i)
    if (lens[i] != 0) h.sym[offs[lens[i]]++] = (unsigned short)i;
  if (h.fast) {
    unsigned code = 0;
    int index = 0;
    for (int l = 1; l <= h.fast_bits; ++l) {
      for (int k = 0; k < (int)h.count[l]; ++k, ++code, ++index) {
        unsigned rev = 0;                          // the code's bits arrive most significant first
        for (int bit = 0; bit < l; ++bit) rev |= ((code >> bit) & 1u) << (l - 1 - bit);
        const unsigned short entry = (unsigned short)((h.sym[index] << 4) | l);
        for (unsigned j = rev; j < (1u << h.fast_bits); j += 1u << l) h.fast[j] = entry;
      }
      code <<= 1;
    }
  }
  return DD_INFLATE_OK;
}

// -> the symbol, or minus a status: TRUNCATED when the input ends inside the code, SYMBOL when the bits are no code of an incomplete set
DD_HD int dd_huff_decode(dd_bits& b, const dd_huff& h) {
  if (h.fast) {
    if (b.nbits < DD_INFLATE_MAX_BITS) dd_bits_refill(b);
    const unsigned entry = h.fast[b.hold & ((1u << h.fast_bits) - 1u)];      // (bits that are not there read as zero)
    if (entry != 0u) {
      const int l = (int)(entry & 15u);
      if (l > b.nbits) return -DD_INFLATE_TRUNCATED;      // a prefix code: no shorter code matches the bits that are there
      dd_bits_take(b, l);
      return (int)(entry >> 4);
    }
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= DD_INFLATE_MAX_BITS; ++l) {
    if (!dd_bits_need(b, 1)) return -DD_INFLATE_TRUNCATED;
    code |= (int)dd_bits_take(b, 1);
    const int count = h.count[l];
    if (code - count < first) return h.sym[index + (code - first)];
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -DD_INFLATE_SYMBOL;
}

DD_HD dd_huff dd_huff_lit(dd_inflate_tables* t) { return dd_huff{t->lit_count, t->lit_sym, t->lit_fast, DD_INFLATE_LIT_BITS}; }
DD_HD dd_huff dd_huff_dist(dd_inflate_tables* t) { return dd_huff{t->dist_count, t->dist_sym, t->dist_fast, DD_INFLATE_DIST_BITS}; }

// the fixed code of RFC 1951 3.2.6
DD_HD void dd_fixed_codes(dd_inflate_tables* t) {
  for (int i = 0; i < DD_INFLATE_LIT_SYMBOLS; ++i) t->lens[i] = (unsigned char)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
  for (int i = 0; i < DD_INFLATE_DIST_SYMBOLS; ++i) t->lens[DD_INFLATE_LIT_SYMBOLS + i] = 5;
  dd_huff_build(dd_huff_lit(t), t->lens, DD_INFLATE_LIT_SYMBOLS, t->offs, DD_CODE_LIT);
  dd_huff_build(dd_huff_dist(t), t->lens + DD_INFLATE_LIT_SYMBOLS, DD_INFLATE_DIST_SYMBOLS, t->offs, DD_CODE_DIST);
}

// the header of a dynamic block (RFC 1951 3.2.7) -> status
DD_HD int dd_dynamic_codes(dd_bits& b, dd_inflate_tables* t) {
  if (!dd_bits_need(b, 14)) return DD_INFLATE_TRUNCATED;
  const int nlen = (int)dd_bits_take(b, 5) + 257, ndist = (int)dd_bits_take(b, 5) + 1, ncode = (int)dd_bits_take(b, 4) + 4;
  if (nlen > 286 || ndist > 30) return DD_INFLATE_LENGTHS;
  // the order the code-length code's lengths are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
  const unsigned long long order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                                      5ull << 45 | 11ull << 50 | 4ull << 55;
  const unsigned long long order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  for (int i = 0; i < DD_INFLATE_CLEN_SYMBOLS; ++i) t->lens[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    if (!dd_bits_need(b, 3)) return DD_INFLATE_TRUNCATED;
    const int which = (int)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31ull);
    t->lens[which] = (unsigned char)dd_bits_take(b, 3);
  }
  const dd_huff clen = dd_huff{t->clen_count, t->clen_sym, nullptr, 0};
  if (dd_huff_build(clen, t->lens, DD_INFLATE_CLEN_SYMBOLS, t->offs, DD_CODE_CLEN) != DD_INFLATE_OK) return DD_INFLATE_LENGTHS;
  const int total = nlen + ndist;
  int at = 0;
  while (at < total) {                                      // every round takes at least one bit
    const int sym = dd_huff_decode(b, clen);
    if (sym < 0) return -sym;
    if (sym < 16) {
      t->lens[at++] = (unsigned char)sym;
      continue;
    }
    int value = 0, repeat;
    if (sym == 16) {
      if (at == 0) return DD_INFLATE_LENGTHS;               // nothing to repeat
      if (!dd_bits_need(b, 2)) return DD_INFLATE_TRUNCATED;
      value = t->lens[at - 1];
      repeat = 3 + (int)dd_bits_take(b, 2);
    } else if (sym == 17) {
      if (!dd_bits_need(b, 3)) return DD_INFLATE_TRUNCATED;
      repeat = 3 + (int)dd_bits_take(b, 3);
    } else {
      if (!dd_bits_need(b, 7)) return DD_INFLATE_TRUNCATED;
      repeat = 11 + (int)dd_bits_take(b, 7);
    }
    if (repeat > total - at) return DD_INFLATE_LENGTHS;
    for (int i = 0; i < repeat; ++i) t->lens[at++] = (unsigned char)value;
  }
  if (t->lens[256] == 0) return DD_INFLATE_LENGTHS;         // no end-of-block code
  // the distance lengths move behind the 288 literal/length slots first (at most 30 of them, from a lower index: walk down)
  for (int i = ndist - 1; i >= 0; --i) t->lens[DD_INFLATE_LIT_SYMBOLS + i] = t->lens[nlen + i];
  if (dd_huff_build(dd_huff_lit(t), t->lens, nlen, t->offs, DD_CODE_LIT) != DD_INFLATE_OK) return DD_INFLATE_LENGTHS;
  if (dd_huff_build(dd_huff_dist(t), t->lens + DD_INFLATE_LIT_SYMBOLS, ndist, t->offs, DD_CODE_DIST) != DD_INFLATE_OK) return DD_INFLATE_LENGTHS;
  return DD_INFLATE_OK;
}

// ---------------------------------------------------------------------------------------------------- one stream
// src[0 .. src_bytes) -> exactly dst_bytes bytes through the Sink -> status
template <class Sink>
DD_HD int dd_inflate_stream(const unsigned char* src, int src_bytes, int dst_bytes, dd_inflate_tables* t, Sink& sink) {
  const int head = dd_zlib_header(src, src_bytes);
  if (head != DD_INFLATE_OK) return head;
  dd_bits b{src, src_bytes, 2, 0, 0ull};
  int produced = 0;
  for (unsigned last = 0u; last == 0u;) {                  // every block takes at least three bits
    if (!dd_bits_need(b, 3)) return DD_INFLATE_TRUNCATED;
    last = dd_bits_take(b, 1);
    const unsigned type = dd_bits_take(b, 2);
    if (type == 3u) return DD_INFLATE_BLOCK_TYPE;
    if (type == 0u) {
      dd_bits_to_byte(b);
      if (b.pos > src_bytes - 4) return DD_INFLATE_TRUNCATED;
      const int len = src[b.pos] | (src[b.pos + 1] << 8), nlen = src[b.pos + 2] | (src[b.pos + 3] << 8);
      if ((len ^ nlen) != 0xffff) return DD_INFLATE_STORED;
      b.pos += 4;
      if (len > src_bytes - b.pos) return DD_INFLATE_TRUNCATED;
      if (len > dst_bytes - produced) return DD_INFLATE_OVERRUN;
      if (len > 0) sink.stored(produced, src + b.pos, len);
      b.pos += len;
      produced += len;
      continue;
    }
    if (type == 1u) {
      dd_fixed_codes(t);
    } else {
      const int status = dd_dynamic_codes(b, t);
      if (status != DD_INFLATE_OK) return status;
    }
    const dd_huff lit = dd_huff_lit(t), dist = dd_huff_dist(t);
    for (;;) {                                              // every symbol takes at least one bit
      // Runs of literals, the common case, in a loop of their own that holds nothing but the primary lookup.  It decides nothing: it
      // leaves at anything that is not a literal with a whole code in the primary table and room for its byte, with the reader where it
      // was, and the general path below decodes that symbol again.
      for (;;) {
        if (b.nbits < DD_INFLATE_MAX_BITS) dd_bits_refill(b);
        const unsigned entry = lit.fast[b.hold & ((1u << DD_INFLATE_LIT_BITS) - 1u)];
        const int l = (int)(entry & 15u);
        if (entry == 0u || entry >= (256u << 4) || l > b.nbits || produced >= dst_bytes) break;
        dd_bits_take(b, l);
        sink.literal(produced++, entry >> 4);
      }
      const int sym = dd_huff_decode(b, lit);
      if (sym < 0) return -sym;
      if (sym < 256) {
        if (produced >= dst_bytes) return DD_INFLATE_OVERRUN;
        sink.literal(produced++, (unsigned)sym);
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) return DD_INFLATE_SYMBOL;
      // lengths 3 .. 258: symbols 257 .. 264 one each, then four symbols per number of extra bits, 285 is 258
      int length = 258;
      if (sym < 285) {
        const int i = sym - 257, extra = i < 8 ? 0 : (i >> 2) - 1;
        length = i < 8 ? 3 + i : 3 + ((4 + (i & 3)) << extra);
        if (extra) {
          if (!dd_bits_need(b, extra)) return DD_INFLATE_TRUNCATED;
          length += (int)dd_bits_take(b, extra);
        }
      }
      const int dsym = dd_huff_decode(b, dist);
      if (dsym < 0) return -dsym;
      if (dsym > 29) return DD_INFLATE_SYMBOL;
      // distances 1 .. 32768: symbols 0 .. 3 one each, then two symbols per number of extra bits
      const int dextra = dsym < 4 ? 0 : (dsym >> 1) - 1;
      int distance = dsym < 4 ? 1 + dsym : 1 + ((2 + (dsym & 1)) << dextra);
      if (dextra) {
        if (!dd_bits_need(b, dextra)) return DD_INFLATE_TRUNCATED;
        distance += (int)dd_bits_take(b, dextra);
      }
      if (distance > produced) return DD_INFLATE_DISTANCE;
      if (length > dst_bytes - produced) return DD_INFLATE_OVERRUN;
      sink.match(produced, distance, length);
      produced += length;
    }
  }
  if (produced != dst_bytes) return DD_INFLATE_SHORT;
  dd_bits_to_byte(b);
  if (b.pos > src_bytes - 4) return DD_INFLATE_TRUNCATED;
  const unsigned want = ((unsigned)src[b.pos] << 24) | ((unsigned)src[b.pos + 1] << 16) | ((unsigned)src[b.pos + 2] << 8) | (unsigned)src[b.pos + 3];
  if (sink.adler(dst_bytes) != want) return DD_INFLATE_CHECK;
  return DD_INFLATE_OK;      // (bytes behind the Adler-32 are ignored, as zlib.decompress ignores them)
}

#endif  // DD_INFLATE_CORE_H
