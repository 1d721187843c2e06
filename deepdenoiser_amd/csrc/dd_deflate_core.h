// The deflate coder core shared by the device kernel (dd_exr_deflate.hip) and a stand-alone host program (tests/exr_deflate_core_main.cpp):
// everything that decides a BYTE, an ADDRESS or a STATUS of dd_exr_deflate (include/dd_hip.h) lives here, as functions that compile for the
// host and for the device from the same text, so bounds and undefined behaviour are found on the CPU under sanitizers before the code runs
// on a GPU, and the two builds give the same bytes.
//
// Lanes.  One wave codes one stream.  The text is written in phases: code outside DD_FOR_LANES is wave-uniform (every lane computes the same
// values from the same LDS words and writes the same values back); a DD_FOR_LANES body is the work of one lane.  On the device the body runs
// once, on the 64 lanes; on the CPU it is a loop over 64 lane numbers.  The two agree because, inside a phase, a lane reads only what earlier
// phases wrote (or its own slots) and what lanes write to a shared word goes through max / add / or, which do not depend on the order.
// DD_LANES_SYNC stands between phases (a workgroup fence on the device: LDS and the token buffer; nothing on the CPU).  State that lives across
// phases is in a dd_deflate_state (LDS on the device), never in a per-lane variable.
//
// The coder, per stream of n bytes (n <= 2^30):
//   match   : 64 consecutive positions per step.  Every lane hashes the four bytes at its position and reads its bucket (the latest earlier
//             position with that hash, + 1) FIRST; after the step all lanes put their positions in with a maximum, so the table does not depend
//             on lane order.  Beside the bucket a lane probes the distances 1 .. 4 (the start of runs and of short periods) and looks for the
//             nearest earlier lane of its own step with the same four bytes: the bucket of an earlier step sees neither.  Length 3 .. 258, distance <= 32768, a length-3 match farther than 4096 is dropped (its distance
//             bits cost more than three literals).  A uniform walk over the step picks greedily: a position a running match covers is skipped,
//             the match's end is carried into the next step, and a step a match covers entirely is skipped whole (no bucket reads or updates).
//   blocks  : tokens (a literal, or length and distance in one word) go to the stream's slice of the workspace and into the histograms; a block
//             ends at DD_DEFLATE_BLOCK_TOKENS tokens, at the border between the two halves ((n + 1) / 2: the even and the odd bytes of an EXR
//             chunk have different statistics; streams under DD_DEFLATE_SPLIT_BYTES, where a second header costs more than it wins, are
//             one block) and at the end.
//   codes   : per block a Huffman code from the histograms (rank sort by the lanes, the in-place Moffat-Katajainen length computation, lengths
//             limited to 15 by moving codes down until the Kraft sum is exact: the code is complete).  A distance code with fewer than two used
//             symbols gets two codes of one bit, so it is complete for every inflater.  The code lengths are sent with one of two FIXED codes, so
//             there is no third construction: flat, four bits for each length 0 .. 15 (at most (286 + 30) * 4 bits per block), or, where
//             that is smaller (few used symbols), zero runs as the symbols 17 / 18 in two bits and every other length in five.  The sizes
//             of the dynamic and of the fixed form follow exactly from the histograms; the smaller is written.
//   emit    : 64 items (tokens, or header fields) per step: bit lengths, a prefix sum, every lane ORs its bits (at most 48) into an LDS window,
//             whole words are stored in order.  Before every store the bytes still to come (at least the framing's trailer: the four of the
//             Adler-32, or of a segment's marker, see Framings) are checked against dst_capacity: running out is DD_DEFLATE_RAW, never a
//             write past the slot.
//   adler   : sums of the SOURCE bytes by the lanes, 16 bytes per lane and step, kept in 64 bits (dd_exr_inflate.hip has the same form).
//
// Framings.  DD_DEFLATE_FRAME_ZLIB (dd_deflate_stream, the EXR chunks): the two header bytes 78 01, the blocks (the last one final), padding to
// the byte border, the Adler-32.  DD_DEFLATE_FRAME_SEGMENT / _LAST_SEGMENT (dd_deflate_segment, the pieces of a PNG's one IDAT stream,
// dd_png_encode.hip): a raw-deflate body without header; the Adler-32 of the source goes back to the caller, who combines the pieces'.  A
// segment that is not the last has no final block and ends with an EMPTY STORED block -- three zero bits, padding to the byte border, 00 00 FF FF
// (what zlib's Z_SYNC_FLUSH writes) -- so it ends on a byte border and the next body follows it directly; the last segment's last block is
// final and padded to the byte border.  A segment is one block until the token buffer is full (no border between two halves: filtered image
// rows have none).  The emitter's reserve (below) is the four marker bytes for a segment that is not the last and nothing for the last one.
#ifndef DD_DEFLATE_CORE_H
#define DD_DEFLATE_CORE_H

#include "../../include/dd_hip.h"

#if defined(__HIPCC__)
#define DD_DHD __host__ __device__ __forceinline__
#else
#define DD_DHD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define DD_FOR_LANES(lane) for (int lane = (int)threadIdx.x, dd_once_ = 1; dd_once_; dd_once_ = 0)
#define DD_LANES_SYNC()                                     \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); \
    __builtin_amdgcn_wave_barrier();                        \
  } while (0)
#else
#define DD_FOR_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define DD_LANES_SYNC() \
  do {                  \
  } while (0)
#endif

#define DD_DEFLATE_LANES 64
#define DD_DEFLATE_HASH_BITS 13
#define DD_DEFLATE_BLOCK_TOKENS 16384      // per stream: the workspace slice holds this many 32-bit tokens
#define DD_DEFLATE_MAX_BYTES (1 << 30)
#define DD_DEFLATE_SPLIT_BYTES 1024         // from this size on a block ends at the border between the two halves
#define DD_DEFLATE_LIT 288                 // literal/length lengths and codes at [0, 288), distances at [288, 320)
#define DD_DEFLATE_DIST 32
#define DD_DEFLATE_MAX_BITS 15
#define DD_DEFLATE_WINDOW_WORDS 104        // 31 bits left over + 64 items of at most 48 bits, and the two words a shifted item may reach into

struct dd_deflate_state {
  unsigned hash[1 << DD_DEFLATE_HASH_BITS];      // position + 1 of the latest quadruple with this hash, 0: none
  unsigned long long item[DD_DEFLATE_LANES];     // emit: a lane's bits
  unsigned long long sums[3 * DD_DEFLATE_LANES]; // adler: a lane's partial sums
  unsigned scan[DD_DEFLATE_LANES];
  unsigned mlen[DD_DEFLATE_LANES], mdist[DD_DEFLATE_LANES], sel[DD_DEFLATE_LANES], quad[DD_DEFLATE_LANES];
  unsigned hist[DD_DEFLATE_LIT + DD_DEFLATE_DIST];
  unsigned work[DD_DEFLATE_LIT];                 // code construction: the sorted frequencies, then parents, then depths
  unsigned window[DD_DEFLATE_WINDOW_WORDS];
  unsigned cost[2];                              // bits of the block's tokens under the dynamic and the fixed code
  unsigned short order[DD_DEFLATE_LIT];          // the used symbols by ascending frequency
  unsigned short code[DD_DEFLATE_LIT + DD_DEFLATE_DIST];      // bit-reversed: ready to be ORed in
  unsigned short header[DD_DEFLATE_LIT + DD_DEFLATE_DIST];    // the run form of the code lengths: bits | number of bits << 12
  unsigned short bl_count[DD_DEFLATE_MAX_BITS + 1], next_code[DD_DEFLATE_MAX_BITS + 1];
  unsigned char lens[DD_DEFLATE_LIT + DD_DEFLATE_DIST];
};

// ---------------------------------------------------------------------------------------------------- words shared by the lanes
DD_DHD void dd_lanes_max(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (*p < v) *p = v;
#endif
}

DD_DHD void dd_lanes_add(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}

DD_DHD void dd_lanes_or(unsigned* p, unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}

// a[0 .. 64) becomes its inclusive prefix sum (a[lane] was written by the lane itself)
DD_DHD void dd_lanes_scan(unsigned* a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int lane = (int)threadIdx.x;
  unsigned v = a[lane];
  for (int delta = 1; delta < DD_DEFLATE_LANES; delta <<= 1) {
    const unsigned up = __shfl_up(v, delta);
    if (lane >= delta) v += up;
  }
  a[lane] = v;
#else
  for (int i = 1; i < DD_DEFLATE_LANES; ++i) a[i] += a[i - 1];
#endif
}

DD_DHD unsigned dd_load4(const unsigned char* p) {      // four bytes, little-endian, any alignment
  unsigned w;
  __builtin_memcpy(&w, p, 4);
  return w;
}

DD_DHD unsigned dd_deflate_hash(unsigned w) { return (w * 2654435761u) >> (32 - DD_DEFLATE_HASH_BITS); }

// ---------------------------------------------------------------------------------------------------- symbols
// length 3 .. 258 -> symbol 257 .. 285, its number of extra bits and their value (RFC 1951 3.2.5)
DD_DHD void dd_length_symbol(int length, int& sym, int& extra, unsigned& value) {
  const int l = length - 3;
  if (length == 258) { sym = 285; extra = 0; value = 0u; return; }
  if (l < 8) { sym = 257 + l; extra = 0; value = 0u; return; }
  extra = (31 - __builtin_clz((unsigned)l)) - 2;
  sym = 257 + (((extra + 1) << 2) | ((l >> extra) & 3));
  value = (unsigned)l & ((1u << extra) - 1u);
}

// distance 1 .. 32768 -> symbol 0 .. 29
DD_DHD void dd_distance_symbol(int distance, int& sym, int& extra, unsigned& value) {
  const int d = distance - 1;
  if (d < 4) { sym = d; extra = 0; value = 0u; return; }
  extra = (31 - __builtin_clz((unsigned)d)) - 1;
  sym = ((extra + 1) << 1) | ((d >> extra) & 1);
  value = (unsigned)d & ((1u << extra) - 1u);
}

DD_DHD int dd_symbol_extra(int s) {      // extra bits of symbol s of the joint table (distances behind DD_DEFLATE_LIT)
  if (s < DD_DEFLATE_LIT) return (s < 265 || s >= 285) ? 0 : ((s - 257) >> 2) - 1;
  const int d = s - DD_DEFLATE_LIT;
  return d < 4 ? 0 : (d >> 1) - 1;
}

DD_DHD int dd_fixed_length(int s) {
  if (s >= DD_DEFLATE_LIT) return 5;
  return s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
}

#define DD_TOKEN_MATCH 0x80000000u      // | (length - 3) << 16 | (distance - 1); a literal is its byte

// ---------------------------------------------------------------------------------------------------- codes
// Code lengths (at most 15, a complete code) of hist[0 .. nsym) into lens[0 .. nsym).  A set with fewer than two used symbols gets two codes of
// one bit: the used symbol (or symbol 0) and its neighbour.
DD_DHD void dd_deflate_lengths(dd_deflate_state* ws, const unsigned* hist, int nsym, unsigned char* lens) {
  DD_LANES_SYNC();
  DD_FOR_LANES(lane) {
    for (int s = lane; s < nsym; s += DD_DEFLATE_LANES) {
      const unsigned f = hist[s];
      lens[s] = 0;
      if (f == 0u) continue;
      int rank = 0;
      for (int j = 0; j < nsym; ++j) {
        const unsigned g = hist[j];
        rank += (g != 0u && (g < f || (g == f && j < s))) ? 1 : 0;
      }
      ws->work[rank] = f;
      ws->order[rank] = (unsigned short)s;
    }
  }
  DD_LANES_SYNC();
  int used = 0;
  for (int j = 0; j < nsym; ++j) used += hist[j] != 0u ? 1 : 0;
  if (used < 2) {
    const int s = used ? (int)ws->order[0] : 0;
    lens[s] = 1;
    lens[s == 0 ? 1 : s - 1] = 1;
    DD_LANES_SYNC();
    return;
  }
  unsigned* a = ws->work;      // (Moffat, Katajainen: in-place calculation of minimum-redundancy codes)
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < used - 1; ++next) {
    if (leaf >= used || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (unsigned)next; } else { a[next] = a[leaf++]; }
    if (leaf >= used || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (unsigned)next; } else { a[next] += a[leaf++]; }
  }
  a[used - 2] = 0u;
  for (int next = used - 3; next >= 0; --next) a[next] = a[a[next]] + 1u;
  {
    int avail = 1, inner = 0, next = used - 1;
    unsigned depth = 0u;
    root = used - 2;
    while (avail > 0) {
      while (root >= 0 && a[root] == depth) { ++inner; --root; }
      while (avail > inner) { a[next--] = depth; --avail; }
      avail = 2 * inner;
      ++depth;
      inner = 0;
    }
  }
  // a[i]: the depth of the i-th symbol by ascending frequency.  Limit to 15 bits: clamp, then repair the Kraft sum one unit at a time.
  for (int l = 0; l <= DD_DEFLATE_MAX_BITS; ++l) ws->bl_count[l] = 0;
  for (int i = 0; i < used; ++i) {
    const unsigned d = a[i] > (unsigned)DD_DEFLATE_MAX_BITS ? (unsigned)DD_DEFLATE_MAX_BITS : a[i];
    ws->bl_count[d]++;
  }
  unsigned total = 0u;
  for (int l = DD_DEFLATE_MAX_BITS; l >= 1; --l) total += (unsigned)ws->bl_count[l] << (DD_DEFLATE_MAX_BITS - l);
  while (total > (1u << DD_DEFLATE_MAX_BITS)) {      // (every round takes one unit off: it ends)
    ws->bl_count[DD_DEFLATE_MAX_BITS]--;
    for (int l = DD_DEFLATE_MAX_BITS - 1; l >= 1; --l)
      if (ws->bl_count[l] != 0) {
        ws->bl_count[l]--;
        ws->bl_count[l + 1] += 2;
        break;
      }
    --total;
  }
  int i = used - 1;
  for (int l = 1; l <= DD_DEFLATE_MAX_BITS; ++l)
    for (int k = (int)ws->bl_count[l]; k > 0 && i >= 0; --k) lens[ws->order[i--]] = (unsigned char)l;
  DD_LANES_SYNC();
}

// the canonical codes of lens[0 .. nsym), bit-reversed
DD_DHD void dd_deflate_codes(dd_deflate_state* ws, const unsigned char* lens, int nsym, unsigned short* code) {
  for (int l = 0; l <= DD_DEFLATE_MAX_BITS; ++l) ws->bl_count[l] = 0;
  for (int s = 0; s < nsym; ++s) ws->bl_count[lens[s]]++;
  ws->bl_count[0] = 0;
  unsigned c = 0u;
  for (int l = 1; l <= DD_DEFLATE_MAX_BITS; ++l) {
    c = (c + ws->bl_count[l - 1]) << 1;
    ws->next_code[l] = (unsigned short)c;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = lens[s];
    if (l == 0) { code[s] = 0; continue; }
    const unsigned v = ws->next_code[l]++;
    unsigned rev = 0u;
    for (int bit = 0; bit < l; ++bit) rev |= ((v >> bit) & 1u) << (l - 1 - bit);
    code[s] = (unsigned short)rev;
  }
  DD_LANES_SYNC();
}

// ---------------------------------------------------------------------------------------------------- the bit writer
// Out:  void word(int at, unsigned v)  four bytes at byte `at` of the stream (at % 4 == 0), little-endian;  void byte(int at, unsigned v)
struct dd_deflate_emitter {
  int fill;         // bits of window[0] that are taken (<= 32)
  int written;      // bytes stored
  int capacity;
  int reserve;      // bytes that are certain to follow the call at hand (the Adler-32, the marker of a segment): a store is made only where they still fit
};

// The lanes have set ws->item[lane] (bits, low end first) and ws->scan[lane] (how many, <= 48).  `last`: nothing follows (the bits end on a
// byte): the tail bytes are stored too.  -> false when the stream does not fit.
template <class Out>
DD_DHD bool dd_deflate_emit(dd_deflate_state* ws, dd_deflate_emitter& em, Out& out, bool last) {
  DD_LANES_SYNC();
  dd_lanes_scan(ws->scan);
  DD_LANES_SYNC();
  DD_FOR_LANES(lane) {
    const unsigned incl = ws->scan[lane], nb = incl - (lane ? ws->scan[lane - 1] : 0u);
    if (nb != 0u) {
      const unsigned at = (unsigned)em.fill + incl - nb, w = at >> 5, s = at & 31u;
      const unsigned long long bits = ws->item[lane], lo = bits << s;
      dd_lanes_or(ws->window + w, (unsigned)lo);
      if ((unsigned)(lo >> 32) != 0u) dd_lanes_or(ws->window + w + 1, (unsigned)(lo >> 32));
      if (s != 0u && (unsigned)(bits >> (64u - s)) != 0u) dd_lanes_or(ws->window + w + 2, (unsigned)(bits >> (64u - s)));
    }
  }
  const int total = em.fill + (int)ws->scan[DD_DEFLATE_LANES - 1], full = total >> 5;
  DD_LANES_SYNC();
  // what is still to come: the rest of this word and, unless this is the last call, at least the framing's trailer (em.reserve)
  const int tail = last ? ((total & 31) + 7) >> 3 : em.reserve;
  if (em.written > em.capacity - 4 * full - tail) return false;
  DD_FOR_LANES(lane) {
    for (int w = lane; w < full; w += DD_DEFLATE_LANES) out.word(em.written + 4 * w, ws->window[w]);
    if (last && lane < tail) out.byte(em.written + 4 * full + lane, (ws->window[full] >> (8 * lane)) & 0xffu);
  }
  const unsigned left = ws->window[full];
  DD_LANES_SYNC();
  DD_FOR_LANES(lane) {
    for (int w = lane; w <= full; w += DD_DEFLATE_LANES) ws->window[w] = 0u;
  }
  DD_LANES_SYNC();
  ws->window[0] = left;
  em.fill = total & 31;
  em.written += 4 * full + (last ? tail : 0);
  DD_LANES_SYNC();
  return true;
}

// One block: codes from the histograms, the smaller of the dynamic and the fixed form, header, tokens, end of block.
template <class Out>
DD_DHD bool dd_deflate_block(dd_deflate_state* ws, const unsigned* tokens, int ntok, bool final_block, dd_deflate_emitter& em, Out& out) {
  dd_deflate_lengths(ws, ws->hist, 286, ws->lens);
  dd_deflate_lengths(ws, ws->hist + DD_DEFLATE_LIT, 30, ws->lens + DD_DEFLATE_LIT);
  ws->lens[286] = ws->lens[287] = 0;      // (the symbols only the fixed code has)
  ws->lens[DD_DEFLATE_LIT + 30] = ws->lens[DD_DEFLATE_LIT + 31] = 0;
  int hlit = 257, hdist = 1;
  for (int s = 257; s < 286; ++s)
    if (ws->lens[s] != 0) hlit = s + 1;
  for (int s = 1; s < 30; ++s)
    if (ws->lens[DD_DEFLATE_LIT + s] != 0) hdist = s + 1;
  ws->cost[0] = 0u;
  ws->cost[1] = 0u;
  DD_LANES_SYNC();
  DD_FOR_LANES(lane) {
    unsigned dynamic = 0u, fixed = 0u;
    for (int s = lane; s < DD_DEFLATE_LIT + DD_DEFLATE_DIST; s += DD_DEFLATE_LANES) {
      const unsigned f = ws->hist[s];
      if (f == 0u) continue;
      const unsigned extra = (unsigned)dd_symbol_extra(s);
      dynamic += f * ((unsigned)ws->lens[s] + extra);
      fixed += f * ((unsigned)dd_fixed_length(s) + extra);
    }
    dd_lanes_add(ws->cost + 0, dynamic);
    dd_lanes_add(ws->cost + 1, fixed);
  }
  DD_LANES_SYNC();
  // The code lengths in their second form: zero runs as the symbols 17 (3 .. 10) and 18 (11 .. 138) of a code that is fixed as well (two bits
  // for 17 and 18, five for a length 0 .. 15, none for 16; Kraft: 2/4 + 16/32).  Items: bits | number of bits << 12.
  const int nlens = hlit + hdist;
  int nitems = 0;
  unsigned run_bits = 0u;
  for (int k = 0; k < nlens;) {
    const unsigned v = ws->lens[k < hlit ? k : DD_DEFLATE_LIT + (k - hlit)];
    int r = 1;
    if (v == 0u)
      while (k + r < nlens && r < 138 && ws->lens[k + r < hlit ? k + r : DD_DEFLATE_LIT + (k + r - hlit)] == 0) ++r;
    unsigned item;
    if (r >= 11) {
      item = 2u | (unsigned)(r - 11) << 2 | 9u << 12;                       // 18 is "01", sent from its high bit
    } else if (r >= 3) {
      item = 0u | (unsigned)(r - 3) << 2 | 5u << 12;                        // 17 is "00"
    } else {
      r = 1;                                                                // the length v is "1vvvv"
      item = (1u | ((v >> 3) & 1u) << 1 | ((v >> 2) & 1u) << 2 | ((v >> 1) & 1u) << 3 | (v & 1u) << 4) | 5u << 12;
    }
    ws->header[nitems++] = (unsigned short)item;
    run_bits += item >> 12;
    k += r;
  }
  const bool use_runs = run_bits < 4u * (unsigned)nlens;
  const unsigned dynamic_bits = 3u + 14u + 19u * 3u + (use_runs ? run_bits : 4u * (unsigned)nlens) + ws->cost[0], fixed_bits = 3u + ws->cost[1];
  const bool use_fixed = fixed_bits <= dynamic_bits;
  DD_LANES_SYNC();
  if (use_fixed) {
    DD_FOR_LANES(lane) {
      for (int s = lane; s < DD_DEFLATE_LIT + DD_DEFLATE_DIST; s += DD_DEFLATE_LANES) ws->lens[s] = (unsigned char)dd_fixed_length(s);
    }
    DD_LANES_SYNC();
  }
  dd_deflate_codes(ws, ws->lens, DD_DEFLATE_LIT, ws->code);
  dd_deflate_codes(ws, ws->lens + DD_DEFLATE_LIT, DD_DEFLATE_DIST, ws->code + DD_DEFLATE_LIT);
  // ---- the block header
  DD_FOR_LANES(lane) {
    unsigned long long bits = 0ull;
    unsigned nb = 0u;
    if (lane == 0) {
      bits = (final_block ? 1ull : 0ull) | (use_fixed ? 1ull : 2ull) << 1;
      nb = 3u;
      if (!use_fixed) {
        bits |= (unsigned long long)(hlit - 257) << 3 | (unsigned long long)(hdist - 1) << 8 | 15ull << 13;      // HCLEN: all 19
        nb = 17u;
      }
    } else if (!use_fixed && lane == 1) {
      // the code-length code, three bits each in the order 16 17 18 0 8 7 ...: flat (16, 17, 18 unused, the lengths 0 .. 15 four bits each)
      // or the run form
      for (int k = 3; k < 19; ++k) bits |= (use_runs ? 5ull : 4ull) << (3 * k);
      if (use_runs) bits |= 2ull << 3 | 2ull << 6;
      nb = 57u;
    }
    ws->item[lane] = bits;
    ws->scan[lane] = nb;
  }
  if (!dd_deflate_emit(ws, em, out, false)) return false;
  if (!use_fixed && use_runs) {
    for (int g = 0; g < nitems; g += DD_DEFLATE_LANES) {
      DD_FOR_LANES(lane) {
        const int k = g + lane;
        const unsigned item = k < nitems ? ws->header[k] : 0u;
        ws->item[lane] = item & 0xfffu;
        ws->scan[lane] = item >> 12;
      }
      if (!dd_deflate_emit(ws, em, out, false)) return false;
    }
  } else if (!use_fixed) {
    for (int g = 0; g < nlens; g += DD_DEFLATE_LANES) {
      DD_FOR_LANES(lane) {
        const int k = g + lane;
        unsigned long long bits = 0ull;
        unsigned nb = 0u;
        if (k < nlens) {
          const unsigned v = ws->lens[k < hlit ? k : DD_DEFLATE_LIT + (k - hlit)];      // the flat code of v is v, sent from its high bit
          bits = ((v >> 3) & 1u) | ((v >> 2) & 1u) << 1 | ((v >> 1) & 1u) << 2 | (v & 1u) << 3;
          nb = 4u;
        }
        ws->item[lane] = bits;
        ws->scan[lane] = nb;
      }
      if (!dd_deflate_emit(ws, em, out, false)) return false;
    }
  }
  // ---- the tokens and the end-of-block code
  for (int g = 0; g <= ntok; g += DD_DEFLATE_LANES) {
    DD_FOR_LANES(lane) {
      const int k = g + lane;
      unsigned long long bits = 0ull;
      unsigned nb = 0u;
      if (k < ntok) {
        const unsigned t = tokens[k];
        if ((t & DD_TOKEN_MATCH) == 0u) {
          bits = ws->code[t & 255u];
          nb = ws->lens[t & 255u];
        } else {
          int sym, extra;
          unsigned value;
          dd_length_symbol((int)((t >> 16) & 255u) + 3, sym, extra, value);
          bits = ws->code[sym];
          nb = ws->lens[sym];
          bits |= (unsigned long long)value << nb;
          nb += (unsigned)extra;
          dd_distance_symbol((int)(t & 0x7fffu) + 1, sym, extra, value);
          bits |= (unsigned long long)ws->code[DD_DEFLATE_LIT + sym] << nb;
          nb += ws->lens[DD_DEFLATE_LIT + sym];
          bits |= (unsigned long long)value << nb;
          nb += (unsigned)extra;
        }
      } else if (k == ntok) {
        bits = ws->code[256];
        nb = ws->lens[256];
      }
      ws->item[lane] = bits;
      ws->scan[lane] = nb;
    }
    if (!dd_deflate_emit(ws, em, out, false)) return false;
  }
  return true;
}

// Adler-32 of src[0 .. n), n <= 2^30
DD_DHD unsigned dd_deflate_adler(dd_deflate_state* ws, const unsigned char* src, int n) {
  const int groups = n >> 4;
  DD_LANES_SYNC();
  DD_FOR_LANES(lane) {
    unsigned long long a = 0ull, b = 0ull, t = 0ull;      // sum d, sum (n - group start) * (group's sum), sum (index in group) * d
    for (int g = lane; g < groups; g += DD_DEFLATE_LANES) {
      const unsigned char* p = src + ((long)g << 4);
      unsigned s = 0u, weighted = 0u;
      for (int k = 0; k < 4; ++k) {
        const unsigned w = dd_load4(p + 4 * k);
        const unsigned b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
        const unsigned sum = b0 + b1 + b2 + b3;
        weighted += 4u * (unsigned)k * sum + b1 + 2u * b2 + 3u * b3;
        s += sum;
      }
      a += s;
      b += (unsigned long long)(n - (g << 4)) * s;
      t += weighted;
    }
    if (lane == 0)
      for (int i = groups << 4; i < n; ++i) {
        const unsigned d = src[i];
        a += d;
        b += (unsigned long long)(n - i) * d;
      }
    ws->sums[3 * lane] = a;
    ws->sums[3 * lane + 1] = b;
    ws->sums[3 * lane + 2] = t;
  }
  DD_LANES_SYNC();
  unsigned long long a = 0ull, b = 0ull, t = 0ull;
  for (int l = 0; l < DD_DEFLATE_LANES; ++l) {
    a += ws->sums[3 * l];
    b += ws->sums[3 * l + 1];
    t += ws->sums[3 * l + 2];
  }
  DD_LANES_SYNC();
  const unsigned long long m = 65521ull;
  const unsigned lo = (unsigned)((1ull + a) % m);
  const unsigned hi = (unsigned)(((unsigned long long)n % m + b % m + m - t % m) % m);
  return (hi << 16) | lo;
}

// how far src[c ..] and src[p ..] agree, at most `limit` bytes (c < p, p + limit <= n)
DD_DHD int dd_match_length(const unsigned char* src, int c, int p, int limit) {
  int l = 0;
  while (l + 4 <= limit) {
    const unsigned x = dd_load4(src + c + l) ^ dd_load4(src + p + l);
    if (x != 0u) return l + (__builtin_ctz(x) >> 3);
    l += 4;
  }
  while (l < limit && src[c + l] == src[p + l]) ++l;
  return l;
}

// ---------------------------------------------------------------------------------------------------- one stream
#define DD_DEFLATE_FRAME_ZLIB 0
#define DD_DEFLATE_FRAME_SEGMENT 1
#define DD_DEFLATE_FRAME_LAST_SEGMENT 2

// src[0 .. n) -> a stream in `framing` of at most `capacity` bytes through `out`; tokens: DD_DEFLATE_BLOCK_TOKENS words of workspace.
// -> DD_DEFLATE_OK and *size, or DD_DEFLATE_RAW (then anything may stand in out[0 .. capacity), nothing behind it).  *adler: the Adler-32 of
// the source, for the segment framings whatever the status (the ZLIB framing writes it into the stream and sets it only with OK).
template <class Out>
DD_DHD int dd_deflate_framed(const int framing, const unsigned char* src, int n, int capacity, unsigned* tokens, dd_deflate_state* ws, Out& out, int* size,
                             unsigned* adler_out) {
  const bool zlib = framing == DD_DEFLATE_FRAME_ZLIB, final_stream = framing != DD_DEFLATE_FRAME_SEGMENT;
  *size = 0;
  if (!zlib) *adler_out = dd_deflate_adler(ws, src, n);
  // (ZLIB: two header bytes, at least a 10-bit block, the Adler-32; a segment: the block, and the three bits and four bytes of its marker)
  if (capacity < (zlib ? 8 : (final_stream ? 2 : 6))) return DD_DEFLATE_RAW;
  DD_FOR_LANES(lane) {
    for (int i = lane; i < (1 << DD_DEFLATE_HASH_BITS); i += DD_DEFLATE_LANES) ws->hash[i] = 0u;
    for (int i = lane; i < DD_DEFLATE_WINDOW_WORDS; i += DD_DEFLATE_LANES) ws->window[i] = 0u;
    for (int i = lane; i < DD_DEFLATE_LIT + DD_DEFLATE_DIST; i += DD_DEFLATE_LANES) ws->hist[i] = i == 256 ? 1u : 0u;
  }
  DD_LANES_SYNC();
  if (zlib) ws->window[0] = 0x0178u;      // CMF 0x78 (deflate, 32 KiB window), FLG 0x01 (fastest; 0x7801 % 31 == 0)
  dd_deflate_emitter em{zlib ? 16 : 0, 0, capacity, framing == DD_DEFLATE_FRAME_LAST_SEGMENT ? 0 : 4};
  DD_LANES_SYNC();
  const int half = (zlib && n >= DD_DEFLATE_SPLIT_BYTES) ? (n + 1) >> 1 : n;      // (a short stream is one block: a second header costs more than it wins)
  int pos = 0, carry = 0, ntok = 0, block_start = 0;
  while (pos < n) {
    int end = pos + DD_DEFLATE_LANES < n ? pos + DD_DEFLATE_LANES : n;
    if (pos < half && end > half) end = half;
    const int count = end - pos;
    if (carry < end) {
      // ---- every lane's best match, from the table as the earlier steps left it
      DD_FOR_LANES(lane) {
        const int p = pos + lane;
        ws->quad[lane] = (lane < count && n - p >= 4) ? dd_load4(src + p) : 0u;
      }
      DD_LANES_SYNC();
      DD_FOR_LANES(lane) {
        const int p = pos + lane;
        int best = 0, best_distance = 0;
        if (lane < count) {
          const int limit = n - p < 258 ? n - p : 258;
          if (limit >= 3) {
            for (int d = 1; d <= 4 && d <= p; ++d) {      // (of equally long matches the nearest: fewer distance bits)
              const int l = dd_match_length(src, p - d, p, limit);
              if (l >= 3 && l > best) { best = l; best_distance = d; }
            }
            if (limit >= 4 && best < limit) {      // the nearest earlier position of this step with the same four bytes
              const unsigned w = ws->quad[lane];
              int j = lane - 5;
              while (j >= 0 && ws->quad[j] != w) --j;
              if (j >= 0) {
                const int l = dd_match_length(src, pos + j, p, limit);
                if (l > best) { best = l; best_distance = lane - j; }
              }
            }
            if (limit >= 4 && best < limit) {
              const unsigned c1 = ws->hash[dd_deflate_hash(dd_load4(src + p))];
              if (c1 != 0u && p - (int)(c1 - 1u) <= 32768) {
                const int c = (int)(c1 - 1u), l = dd_match_length(src, c, p, limit);
                if (l > best && (l >= 4 || p - c <= 4096)) { best = l; best_distance = p - c; }
              }
            }
          }
        }
        ws->mlen[lane] = (unsigned)best;
        ws->mdist[lane] = (unsigned)best_distance;
        ws->sel[lane] = 0u;
      }
      DD_LANES_SYNC();
      // ---- greedy choice, in order
      int i = (carry > pos ? carry : pos) - pos;
      while (i < count) {
        const int l = (int)ws->mlen[i];
        ws->sel[i] = 1u;
        i += l >= 3 ? l : 1;
      }
      carry = pos + i;
      DD_LANES_SYNC();
      // ---- the table takes the step's positions; the chosen tokens are numbered
      DD_FOR_LANES(lane) {
        const int p = pos + lane;
        if (lane < count && n - p >= 4) dd_lanes_max(ws->hash + dd_deflate_hash(dd_load4(src + p)), (unsigned)p + 1u);
        ws->scan[lane] = ws->sel[lane];
      }
      DD_LANES_SYNC();
      dd_lanes_scan(ws->scan);
      DD_LANES_SYNC();
      DD_FOR_LANES(lane) {
        if (ws->sel[lane] != 0u) {
          const int k = ntok + (int)ws->scan[lane] - 1, l = (int)ws->mlen[lane];
          if (l >= 3) {
            int sym, extra;
            unsigned value;
            tokens[k] = DD_TOKEN_MATCH | (unsigned)(l - 3) << 16 | (ws->mdist[lane] - 1u);
            dd_length_symbol(l, sym, extra, value);
            dd_lanes_add(ws->hist + sym, 1u);
            dd_distance_symbol((int)ws->mdist[lane], sym, extra, value);
            dd_lanes_add(ws->hist + DD_DEFLATE_LIT + sym, 1u);
          } else {
            const unsigned v = src[pos + lane];
            tokens[k] = v;
            dd_lanes_add(ws->hist + v, 1u);
          }
        }
      }
      ntok += (int)ws->scan[DD_DEFLATE_LANES - 1];
      DD_LANES_SYNC();
    }
    pos = carry > end ? carry : end;
    const bool more = pos < n;
    if (!more || ntok + DD_DEFLATE_LANES > DD_DEFLATE_BLOCK_TOKENS || (block_start < half && pos >= half)) {
      if (!dd_deflate_block(ws, tokens, ntok, !more && final_stream, em, out)) return DD_DEFLATE_RAW;
      DD_FOR_LANES(lane) {
        for (int s = lane; s < DD_DEFLATE_LIT + DD_DEFLATE_DIST; s += DD_DEFLATE_LANES) ws->hist[s] = s == 256 ? 1u : 0u;
      }
      DD_LANES_SYNC();
      ntok = 0;
      block_start = pos;
    }
  }
  if (zlib) {
    // ---- up to the byte border, then the Adler-32 of the source, high byte first
    const unsigned adler = dd_deflate_adler(ws, src, n);
    em.fill = (em.fill + 7) & ~7;
    DD_FOR_LANES(lane) {
      ws->item[lane] = lane == 0 ? (unsigned long long)((adler >> 24) | ((adler >> 8) & 0xff00u) | ((adler << 8) & 0xff0000u) | (adler << 24)) : 0ull;
      ws->scan[lane] = lane == 0 ? 32u : 0u;
    }
    if (!dd_deflate_emit(ws, em, out, true)) return DD_DEFLATE_RAW;
    *adler_out = adler;
  } else if (final_stream) {
    // ---- the final block is behind: up to the byte border, nothing more
    em.fill = (em.fill + 7) & ~7;
    DD_FOR_LANES(lane) {
      ws->item[lane] = 0ull;
      ws->scan[lane] = 0u;
    }
    if (!dd_deflate_emit(ws, em, out, true)) return DD_DEFLATE_RAW;
  } else {
    // ---- an empty stored block that is not final: BFINAL 0 and BTYPE 00, zero bits up to the byte border, LEN 0000 and NLEN FFFF
    const unsigned zeros = 3u + ((0u - ((unsigned)em.fill + 3u)) & 7u);
    DD_FOR_LANES(lane) {
      ws->item[lane] = lane == 1 ? 0xffff0000ull : 0ull;
      ws->scan[lane] = lane == 0 ? zeros : (lane == 1 ? 32u : 0u);
    }
    if (!dd_deflate_emit(ws, em, out, true)) return DD_DEFLATE_RAW;
  }
  *size = em.written;
  return DD_DEFLATE_OK;
}

// a zlib stream (RFC 1950): what dd_exr_deflate writes per chunk
template <class Out>
DD_DHD int dd_deflate_stream(const unsigned char* src, int n, int capacity, unsigned* tokens, dd_deflate_state* ws, Out& out, int* size) {
  unsigned adler;
  return dd_deflate_framed(DD_DEFLATE_FRAME_ZLIB, src, n, capacity, tokens, ws, out, size, &adler);
}

// one segment of a zlib stream that the caller puts together (dd_png_deflate): a raw-deflate body and the segment's Adler-32
template <class Out>
DD_DHD int dd_deflate_segment(const unsigned char* src, int n, int capacity, bool last, unsigned* tokens, dd_deflate_state* ws, Out& out, int* size,
                              unsigned* adler) {
  return dd_deflate_framed(last ? DD_DEFLATE_FRAME_LAST_SEGMENT : DD_DEFLATE_FRAME_SEGMENT, src, n, capacity, tokens, ws, out, size, adler);
}

#endif  // DD_DEFLATE_CORE_H
