// OpenEXR scan-line chunks rebuilt on the device (include/dd_hip.h, dd_exr_reconstruct): the host parses the header and inflates (or run-length
// decodes) every chunk of a batch of files into ONE staged buffer; ONE launch then undoes the byte predictor and the even / odd byte split of
// every coded chunk, splits rows and channels, converts UINT / HALF / FLOAT samples to fp32, writes the [H, W, C] planes the frame bank keeps
// and counts the non-finite samples per file (deepdenoiser_amd/openexr.py: plan_file, DeviceDecoder).  The planes are bit-identical to what
// openexr.read_image gives.
//
// Shape.  One workgroup of 256 threads per chunk (1 or 16 scan lines), all files of a batch in one grid.  A chunk holds n = rows * row_bytes
// bytes t[0 .. n) at a 16-byte aligned offset of the staged buffer and owns the bytes up to the next multiple of 16; it is NOT assumed to fit
// LDS (16 lines of a 1920-wide RGBA float file are 491 KB): the prefix sum runs in place in the staged buffer.
//   1. s[i] = (t[0] + sum_{j=1..i} (t[j] - 128)) & 0xFF = (sum_{j<=i} t[j] + 128 (i & 1)) & 0xFF.  A thread owns a contiguous span (a multiple of
//      16 bytes): it adds its span's bytes (16-byte loads), the 256 span sums are scanned (wave scan, then the four wave totals through LDS),
//      and the thread rewrites its span with the running sum.  A raw chunk (NO_COMPRESSION, or stored raw because coding did not shrink it)
//      skips this step.
//   2. After a workgroup barrier the original byte p of a coded chunk is s[p >> 1] for even p and s[half + (p >> 1)] for odd p,
//      half = (n + 1) / 2; of a raw chunk it is t[p].  Threads walk the chunk's destination floats row by row with the destination channel
//      fastest (stores run along the plane's rows); the sample of row r, file channel c, column x starts at r * row_bytes + channel_offset[c] +
//      size[c] * x, an even byte.  FLOAT: the bits are moved.  HALF: widened exactly in integer arithmetic (subnormals normalised, the payload
//      of a NaN shifted up, as numpy does).  UINT: (float)u, rounded to nearest even.
//   3. A destination sample with all exponent bits set counts; the counts are reduced over the workgroup, then ONE integer atomic add on the
//      file's 64-bit counter (integer sums do not depend on the order of the adds).
// Both tables live in device memory, so the kernel trusts no record: a chunk whose file index, rows, offset or size do not fit is skipped whole
// (the test is uniform over the workgroup and stands in front of the first barrier), so nothing is read outside the staged buffer and nothing is
// written outside a plane.  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPlaneChannels = 32;            // a destination set is a 32-bit mask
constexpr long kMaxChunkBytes = 1l << 30;        // n and rows * W * C stay far inside 32 bits

__host__ __device__ __forceinline__ int sample_bytes(int type) { return type == 1 ? 2 : 4; }

// the sum of the four bytes of w (at most 1020: no lane of the 16-bit pair sum overflows)
__device__ __forceinline__ unsigned byte_sum(unsigned w) {
  const unsigned pairs = (w & 0x00ff00ffu) + ((w >> 8) & 0x00ff00ffu);
  return (pairs + (pairs >> 16)) & 0xffffu;
}

// the four running sums run + b0, run + b0 + b1, ... of w's bytes, each modulo 256, with 128 added at the odd positions (a word starts at a
// multiple of 4, so those are bytes 1 and 3); run becomes the last sum
__device__ __forceinline__ unsigned byte_scan(unsigned w, unsigned& run) {
  const unsigned r0 = run + (w & 0xffu), r1 = r0 + ((w >> 8) & 0xffu), r2 = r1 + ((w >> 16) & 0xffu), r3 = r2 + (w >> 24);
  run = r3;
  return ((r0 & 0xffu) | ((r1 & 0xffu) << 8) | ((r2 & 0xffu) << 16) | (r3 << 24)) ^ 0x80008000u;
}

// IEEE half -> float bits, exact
__device__ __forceinline__ unsigned half_bits_to_float_bits(unsigned h) {
  const unsigned sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return sign | 0x7f800000u | (m << 13);
  if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
  if (m == 0u) return sign;
  const unsigned shift = (unsigned)__clz((int)m) - 21u;      // 1 .. 10: moves the leading bit of m to bit 10
  return sign | ((113u - shift) << 23) | (((m << shift) & 0x3ffu) << 13);
}

__global__ __launch_bounds__(kThreads) void exr_reconstruct_kernel(const dd_exr_chunk* __restrict__ chunks, const dd_exr_file* __restrict__ files,
                                                                   int n_files, unsigned char* staged, long staged_bytes,
                                                                   unsigned long long* __restrict__ counts) {
  __shared__ unsigned wave_total[kWaves];
  __shared__ unsigned wave_count[kWaves];
  __shared__ int dst_offset[kMaxPlaneChannels];      // per destination channel: the byte offset of its file channel in a row, -1: not written
  __shared__ int dst_type[kMaxPlaneChannels];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const dd_exr_chunk ck = chunks[blockIdx.x];
  // ---- the records are checked before anything is read or written through them (uniform: the whole workgroup leaves together)
  if (ck.file < 0 || ck.file >= n_files) return;
  const dd_exr_file* f = files + ck.file;
  const int H = f->H, W = f->W, C = f->C, nch = f->n_channels;
  if (H < 1 || W < 1 || C < 1 || C > kMaxPlaneChannels || nch < 1 || nch > DD_EXR_MAX_CHANNELS || f->dst == nullptr) return;
  if (ck.rows < 1 || ck.rows > 16 || ck.row0 < 0 || ck.row0 > H - ck.rows) return;
  long row_bytes = 0;
  bool good = true;
  for (int c = 0; c < nch; ++c) {
    const int t = f->type[c];
    good = good && t >= 0 && t <= 2 && (f->dst_mask[c] >> (C - 1) >> 1) == 0u;
    row_bytes += (long)W * sample_bytes(t);
  }
  const long n_long = row_bytes * ck.rows, cells = (long)ck.rows * W * C;
  if (!good || n_long > kMaxChunkBytes || cells > kMaxChunkBytes) return;
  const int n = (int)n_long, n16 = (n + 15) & ~15;
  if (ck.offset < 0 || (ck.offset & 15) != 0 || ck.offset > staged_bytes - n16) return;
  unsigned char* s = staged + ck.offset;

  if (tid < C) {
    int off = 0, found = -1, type = 0;
    for (int c = 0; c < nch; ++c) {
      const int t = f->type[c];
      if (found < 0 && ((f->dst_mask[c] >> tid) & 1u)) { found = off; type = t; }
      off += W * sample_bytes(t);
    }
    dst_offset[tid] = found;
    dst_type[tid] = type;
  }

  const bool coded = ck.coded != 0;
  if (coded) {
    // ---- 1. the byte prefix sum, in place
    const int span = ((n16 / 16 + kThreads - 1) / kThreads) * 16;
    const int begin = min(tid * span, n16), end = min(begin + span, n16);
    unsigned sum = 0;
    for (int i = begin; i < end; i += 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(s + i);
      sum += byte_sum(v.x) + byte_sum(v.y) + byte_sum(v.z) + byte_sum(v.w);
    }
    unsigned incl = sum;
    for (int delta = 1; delta < 64; delta <<= 1) {
      const unsigned up = __shfl_up(incl, delta);
      if (lane >= delta) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    for (int i = begin; i < end; i += 16) {
      uint4 v = *reinterpret_cast<const uint4*>(s + i);
      v.x = byte_scan(v.x, run); v.y = byte_scan(v.y, run); v.z = byte_scan(v.z, run); v.w = byte_scan(v.w, run);
      *reinterpret_cast<uint4*>(s + i) = v;
    }
  }
  __syncthreads();      // (the rewritten spans, and the channel table, are visible to the workgroup)

  // ---- 2. rows and channels apart, to fp32
  const int half = (n + 1) >> 1, row_cells = W * C;
  float* __restrict__ dst = f->dst;
  unsigned bad = 0;
  for (int r = 0; r < ck.rows; ++r) {
    const int row_at = r * (int)row_bytes;
    float* __restrict__ out = dst + (long)(ck.row0 + r) * row_cells;
    for (int i = tid; i < row_cells; i += kThreads) {
      const int x = C == 3 ? i / 3 : (C == 1 ? i : i / C), d = i - x * C;
      const int at = dst_offset[d], type = dst_type[d];
      if (at < 0) continue;
      const int wide = type != 1;
      const int p = row_at + at + (x << (wide ? 2 : 1));      // even
      unsigned b0, b1, b2 = 0, b3 = 0;
      if (coded) {
        const int q = p >> 1;
        b0 = s[q]; b1 = s[half + q];
        if (wide) { b2 = s[q + 1]; b3 = s[half + q + 1]; }
      } else {
        b0 = s[p]; b1 = s[p + 1];
        if (wide) { b2 = s[p + 2]; b3 = s[p + 3]; }
      }
      const unsigned u = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      const unsigned bits = type == 2 ? u : (type == 1 ? half_bits_to_float_bits(u) : __float_as_uint((float)u));
      bad += (bits & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
      out[i] = __uint_as_float(bits);
    }
  }

  // ---- 3. the file's non-finite count: the waves' trees, then one atomic per workgroup
  for (int delta = 32; delta >= 1; delta >>= 1) bad += __shfl_down(bad, delta);
  if (lane == 0) wave_count[wave] = bad;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
    for (int w = 0; w < kWaves; ++w) total += wave_count[w];
    if (total != 0ull) atomicAdd(counts + ck.file, total);
  }
}

}  // namespace

extern "C" int dd_exr_reconstruct(const dd_exr_chunk* chunks_host, const dd_exr_chunk* chunks, int n_chunks, const dd_exr_file* files_host,
                                  const dd_exr_file* files, int n_files, void* staged, long staged_bytes, unsigned long long* counts,
                                  dd_stream stream) {
  DD_REQUIRE(n_chunks >= 0, "dd_exr_reconstruct: n_chunks=%d", n_chunks);
  if (n_chunks == 0) return DD_OK;
  DD_REQUIRE(chunks_host && chunks && files_host && files, "dd_exr_reconstruct: null chunk or file table");
  DD_REQUIRE(staged && counts, "dd_exr_reconstruct: null staged buffer or count array");
  DD_REQUIRE(n_files >= 1, "dd_exr_reconstruct: n_files=%d", n_files);
  DD_REQUIRE(staged_bytes >= 16, "dd_exr_reconstruct: staged_bytes=%ld", staged_bytes);
  for (int k = 0; k < n_files; ++k) {
    const dd_exr_file& f = files_host[k];
    DD_REQUIRE(f.dst, "dd_exr_reconstruct: file %d has a null plane", k);
    DD_REQUIRE(f.H >= 1 && f.W >= 1, "dd_exr_reconstruct: file %d: H=%d W=%d", k, f.H, f.W);
    DD_REQUIRE(f.C >= 1 && f.C <= kMaxPlaneChannels, "dd_exr_reconstruct: file %d: C=%d (a plane has 1 .. %d channels)", k, f.C, kMaxPlaneChannels);
    DD_REQUIRE(f.n_channels >= 1 && f.n_channels <= DD_EXR_MAX_CHANNELS, "dd_exr_reconstruct: file %d: n_channels=%d (1 .. %d fit the record)", k,
               f.n_channels, DD_EXR_MAX_CHANNELS);
    for (int c = 0; c < f.n_channels; ++c) {
      DD_REQUIRE(f.type[c] >= 0 && f.type[c] <= 2, "dd_exr_reconstruct: file %d channel %d: pixel type=%d (0 UINT, 1 HALF, 2 FLOAT)", k, c, f.type[c]);
      DD_REQUIRE((f.dst_mask[c] >> (f.C - 1) >> 1) == 0u, "dd_exr_reconstruct: file %d channel %d: destination mask 0x%x names a channel >= C=%d", k, c,
                 f.dst_mask[c], f.C);
    }
  }
  for (int k = 0; k < n_chunks; ++k) {
    const dd_exr_chunk& ck = chunks_host[k];
    DD_REQUIRE(ck.rows >= 1 && ck.rows <= 16, "dd_exr_reconstruct: chunk %d: rows=%d (1 .. 16)", k, ck.rows);
    DD_REQUIRE(ck.file >= 0 && ck.file < n_files, "dd_exr_reconstruct: chunk %d: file=%d of %d", k, ck.file, n_files);
    const dd_exr_file& f = files_host[ck.file];
    DD_REQUIRE(ck.row0 >= 0 && ck.row0 <= f.H - ck.rows, "dd_exr_reconstruct: chunk %d: row0=%d rows=%d outside the %d rows of file %d", k, ck.row0,
               ck.rows, f.H, ck.file);
    long row_bytes = 0;
    for (int c = 0; c < f.n_channels; ++c) row_bytes += (long)f.W * sample_bytes(f.type[c]);
    const long n = row_bytes * ck.rows;
    DD_REQUIRE(n <= kMaxChunkBytes && (long)ck.rows * f.W * f.C <= kMaxChunkBytes, "dd_exr_reconstruct: chunk %d holds %ld bytes (at most %ld)", k, n,
               kMaxChunkBytes);
    DD_REQUIRE(ck.offset >= 0 && (ck.offset & 15) == 0 && ck.offset <= staged_bytes - ((n + 15) & ~15l),
               "dd_exr_reconstruct: chunk %d: offset=%lld (%ld bytes) is not 16-byte aligned or leaves the %ld staged bytes", k, (long long)ck.offset, n,
               staged_bytes);
  }
  hipLaunchKernelGGL(exr_reconstruct_kernel, dim3(n_chunks), dim3(kThreads), 0, S(stream), chunks, files, n_files,
                     reinterpret_cast<unsigned char*>(staged), staged_bytes, counts);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
