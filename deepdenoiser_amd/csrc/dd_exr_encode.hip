// OpenEXR scan-line chunks packed on the device (include/dd_hip.h, dd_exr_pack): the inverse of exr_reconstruct_kernel (dd_exr_decode.hip).  ONE
// launch turns the fp32 planes of a whole frame's passes into the bytes of every scan-line chunk, at the chunk's place in one staged buffer:
// HALF or FLOAT samples, per row and per channel in name order, and for a coded chunk the even / odd byte split and the delta predictor, so
// that dd_exr_deflate (dd_exr_deflate.hip, the next launch on the same stream) finds what zlib would be given
// (deepdenoiser_amd/openexr/codec.py: _interleave_and_predict; openexr/encode.py: DeviceEncoder).
//
// Shape.  One workgroup of 256 threads per chunk (1 or 16 scan lines), all files of a batch in one grid.  A chunk holds n = rows * row_bytes
// bytes at a 16-byte aligned offset and owns the bytes up to the next multiple of 16.  A thread builds 16 consecutive OUTPUT bytes and stores
// them with one 16-byte store (the padding behind n as zero).  Output byte i of a coded chunk is d[i] = t[i] - t[i-1] + 128 (d[0] = t[0]) with
// t[i] the raw byte 2 i for i < half = (n + 1) / 2 and the raw byte 2 (i - half) + 1 behind: the thread fetches t[i0 - 1] too, across the
// borders of lanes, rows and the two halves alike.  Consecutive t are the same byte of consecutive samples (HALF) or two bytes of each
// (FLOAT), so a thread reads along a row of one channel; the sample a byte belongs to is kept until the walk leaves it.  The raw byte q lies in
// row q / row_bytes, in the channel whose span of the row holds the rest, at sample (rest - channel offset) / sample size.
// fp32 -> HALF in integer arithmetic: round to nearest even, overflow to +-inf, subnormals; a NaN keeps its sign and the top payload bits and
// stays a NaN.  Both tables live in device memory, so the kernel trusts no record: a chunk whose file index, rows, offset or size do not fit
// writes nothing (the test is uniform over the workgroup).  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kMaxPlaneChannels = 32;
constexpr long kMaxChunkBytes = 1l << 30;

// IEEE float bits -> half bits, round to nearest even
__host__ __device__ __forceinline__ unsigned float_bits_to_half_bits(unsigned x) {
  const unsigned sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7e00u | ((a >> 13) & 0x3ffu);      // NaN: quiet, never the infinity pattern
  const unsigned e = a >> 23;
  if (e >= 143u) return sign | 0x7c00u;                                   // 65536 and above, and infinity
  if (e >= 113u) {                                                        // normal: the carry of the rounding runs into the exponent (65520 -> inf)
    unsigned h = ((e - 112u) << 10) | ((a >> 13) & 0x3ffu);
    const unsigned rest = a & 0x1fffu;
    h += (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ? 1u : 0u;
    return sign | h;
  }
  if (e < 101u) return sign;                                              // below 2^-26: zero (2^-25 itself ties to even: zero, below)
  const unsigned m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;       // 14 .. 25: subnormal, value = m * 2^(e - 150) = (m >> shift) * 2^-24
  unsigned h = m >> shift;
  const unsigned rest = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
  h += (rest > halfway || (rest == halfway && (h & 1u))) ? 1u : 0u;
  return sign | h;
}

struct Walker {      // the sample the last byte came from
  int start, size;
  unsigned bits;
};

__global__ __launch_bounds__(kThreads) void exr_pack_kernel(const dd_exr_chunk* __restrict__ chunks, const dd_exr_source* __restrict__ sources, int n_sources,
                                                            unsigned char* __restrict__ staged, long staged_bytes) {
  __shared__ int channel_at[DD_EXR_MAX_CHANNELS + 1];      // the byte offset of a file channel in a row
  __shared__ int channel_wide[DD_EXR_MAX_CHANNELS];
  __shared__ int channel_source[DD_EXR_MAX_CHANNELS];
  const int tid = threadIdx.x;
  const dd_exr_chunk ck = chunks[blockIdx.x];
  // ---- the records are checked before anything is read or written through them (uniform: the whole workgroup leaves together)
  if (ck.file < 0 || ck.file >= n_sources) return;
  const dd_exr_source* f = sources + ck.file;
  const int H = f->H, W = f->W, C = f->C, nch = f->n_channels;
  if (H < 1 || W < 1 || C < 1 || C > kMaxPlaneChannels || nch < 1 || nch > DD_EXR_MAX_CHANNELS || f->src == nullptr) return;
  if (ck.rows < 1 || ck.rows > 16 || ck.row0 < 0 || ck.row0 > H - ck.rows) return;
  long row_bytes_long = 0;
  bool good = true;
  for (int c = 0; c < nch; ++c) {
    const int t = f->type[c], s = f->src_channel[c];
    good = good && (t == 1 || t == 2) && s >= 0 && s < C;
    row_bytes_long += (long)W * (t == 1 ? 2 : 4);
  }
  const long n_long = row_bytes_long * ck.rows;
  if (!good || n_long > kMaxChunkBytes || (long)H * W * C > (1l << 40)) return;
  const int n = (int)n_long, n16 = (n + 15) & ~15, row_bytes = (int)row_bytes_long;
  if (ck.offset < 0 || (ck.offset & 15) != 0 || ck.offset > staged_bytes - n16) return;
  if (tid == 0) {
    int at = 0;
    for (int c = 0; c < nch; ++c) {
      channel_at[c] = at;
      channel_wide[c] = f->type[c] == 2;
      channel_source[c] = f->src_channel[c];
      at += W * (f->type[c] == 1 ? 2 : 4);
    }
    channel_at[nch] = at;
  }
  __syncthreads();
  const float* __restrict__ src = f->src;
  unsigned char* out = staged + ck.offset;
  const bool coded = ck.coded != 0;
  const int half = (n + 1) >> 1;
  Walker w{-8, 0, 0u};

  auto raw_byte = [&](int q) -> unsigned {      // byte q < n of the chunk as the file stores it
    if ((unsigned)(q - w.start) >= (unsigned)w.size) {
      const int r = q / row_bytes, rest = q - r * row_bytes;
      int k = 0;
      while (k + 1 < nch && rest >= channel_at[k + 1]) ++k;
      const int wide = channel_wide[k], inside = rest - channel_at[k], x = inside >> (wide ? 2 : 1);
      const unsigned bits = __float_as_uint(src[((long)(ck.row0 + r) * W + x) * C + channel_source[k]]);
      w.size = wide ? 4 : 2;
      w.start = q - (inside & (w.size - 1));
      w.bits = wide ? bits : float_bits_to_half_bits(bits);
    }
    return (w.bits >> (8 * (q - w.start))) & 0xffu;
  };
  auto chunk_byte = [&](int i) -> unsigned { return raw_byte(!coded ? i : (i < half ? 2 * i : 2 * (i - half) + 1)); };

  for (int i0 = tid * 16; i0 < n16; i0 += kThreads * 16) {
    unsigned before = (coded && i0 > 0) ? chunk_byte(i0 - 1) : 0u;
    unsigned words[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = i0 + j;
      unsigned d = 0u;
      if (i < n) {
        const unsigned t = chunk_byte(i);
        d = (coded && i > 0) ? (t - before + 128u) & 0xffu : t;
        before = t;
      }
      words[j >> 2] |= d << (8 * (j & 3));
    }
    *reinterpret_cast<uint4*>(out + i0) = make_uint4(words[0], words[1], words[2], words[3]);
  }
}

}  // namespace

extern "C" int dd_exr_pack(const dd_exr_chunk* chunks_host, const dd_exr_chunk* chunks, int n_chunks, const dd_exr_source* sources_host,
                           const dd_exr_source* sources, int n_sources, void* staged, long staged_bytes, dd_stream stream) {
  DD_REQUIRE(n_chunks >= 0, "dd_exr_pack: n_chunks=%d", n_chunks);
  if (n_chunks == 0) return DD_OK;
  DD_REQUIRE(chunks_host && chunks && sources_host && sources, "dd_exr_pack: null chunk or source table");
  DD_REQUIRE(staged, "dd_exr_pack: null staged buffer");
  DD_REQUIRE((reinterpret_cast<unsigned long long>(staged) & 15ull) == 0ull, "dd_exr_pack: the staged buffer is not 16-byte aligned");
  DD_REQUIRE(n_sources >= 1, "dd_exr_pack: n_sources=%d", n_sources);
  DD_REQUIRE(staged_bytes >= 16, "dd_exr_pack: staged_bytes=%ld", staged_bytes);
  for (int k = 0; k < n_sources; ++k) {
    const dd_exr_source& f = sources_host[k];
    DD_REQUIRE(f.src, "dd_exr_pack: source %d has a null plane", k);
    DD_REQUIRE(f.H >= 1 && f.W >= 1, "dd_exr_pack: source %d: H=%d W=%d", k, f.H, f.W);
    DD_REQUIRE(f.C >= 1 && f.C <= kMaxPlaneChannels, "dd_exr_pack: source %d: C=%d (a plane has 1 .. %d channels)", k, f.C, kMaxPlaneChannels);
    DD_REQUIRE((long)f.H * f.W * f.C <= (1l << 40), "dd_exr_pack: source %d: %d x %d x %d samples", k, f.H, f.W, f.C);
    DD_REQUIRE(f.n_channels >= 1 && f.n_channels <= DD_EXR_MAX_CHANNELS, "dd_exr_pack: source %d: n_channels=%d (1 .. %d fit the record)", k, f.n_channels,
               DD_EXR_MAX_CHANNELS);
    for (int c = 0; c < f.n_channels; ++c) {
      DD_REQUIRE(f.type[c] == 1 || f.type[c] == 2, "dd_exr_pack: source %d channel %d: pixel type=%d (1 HALF, 2 FLOAT; the planes are fp32)", k, c, f.type[c]);
      DD_REQUIRE(f.src_channel[c] >= 0 && f.src_channel[c] < f.C, "dd_exr_pack: source %d channel %d: src_channel=%d outside the C=%d of the plane", k, c,
                 f.src_channel[c], f.C);
    }
  }
  for (int k = 0; k < n_chunks; ++k) {
    const dd_exr_chunk& ck = chunks_host[k];
    DD_REQUIRE(ck.rows >= 1 && ck.rows <= 16, "dd_exr_pack: chunk %d: rows=%d (1 .. 16)", k, ck.rows);
    DD_REQUIRE(ck.file >= 0 && ck.file < n_sources, "dd_exr_pack: chunk %d: file=%d of %d", k, ck.file, n_sources);
    const dd_exr_source& f = sources_host[ck.file];
    DD_REQUIRE(ck.row0 >= 0 && ck.row0 <= f.H - ck.rows, "dd_exr_pack: chunk %d: row0=%d rows=%d outside the %d rows of source %d", k, ck.row0, ck.rows, f.H,
               ck.file);
    long row_bytes = 0;
    for (int c = 0; c < f.n_channels; ++c) row_bytes += (long)f.W * (f.type[c] == 1 ? 2 : 4);
    const long n = row_bytes * ck.rows;
    DD_REQUIRE(n <= kMaxChunkBytes, "dd_exr_pack: chunk %d holds %ld bytes (at most %ld)", k, n, kMaxChunkBytes);
    DD_REQUIRE(ck.offset >= 0 && (ck.offset & 15) == 0 && ck.offset <= staged_bytes - ((n + 15) & ~15l),
               "dd_exr_pack: chunk %d: offset=%lld (%ld bytes) is not 16-byte aligned or leaves the %ld staged bytes", k, (long long)ck.offset, n, staged_bytes);
  }
  hipLaunchKernelGGL(exr_pack_kernel, dim3(n_chunks), dim3(kThreads), 0, S(stream), chunks, sources, n_sources, reinterpret_cast<unsigned char*>(staged),
                     staged_bytes);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
