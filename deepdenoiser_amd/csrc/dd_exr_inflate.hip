// The zlib streams of OpenEXR ZIP / ZIPS chunks inflated on the device (include/dd_hip.h, dd_exr_inflate): the host only reads the files; ONE
// launch inflates every stream of a batch into the staged buffer, at the place where dd_exr_reconstruct (dd_exr_decode.hip, the next launch
// on the same stream) expects the chunk's post-inflate bytes (deepdenoiser_amd/openexr.py: DeviceDecoder(inflate="device")).
//
// Shape.  Inflate is serial inside a stream and independent across streams (a 1080p frame with all passes has about 1 800 of them), so ONE
// WAVE decodes ONE stream: a workgroup is a single wave.  Every decision -- header, bit reader, code construction, symbol decode, every
// bound -- is the shared core (dd_inflate_core.h), executed wave-uniformly: all 64 lanes run the same scalar program on the same values (the
// source bytes come from the same addresses, the tables from the same LDS words, every lane writes the same table entries), so control flow
// never diverges.  This file supplies only where the tables live (LDS, 2.6 KB per wave) and how bytes are stored, copied and summed:
//   literal : lane 0 stores the byte.
//   stored  : the 64 lanes copy source bytes.
//   match   : the 64 lanes copy out[at + i] = out[at - distance + i % distance]; the window is READ BACK from the staged buffer (a 16-line
//             chunk of a 1920-wide RGBA float file is 491 KB; the last 32 KiB of it stay in the caches), every source byte lies before `at`.
//   adler   : a wave reduction over the finished output, 16 bytes per lane and step: with d_i the bytes and n their number,
//             a = 1 + sum d_i, b = n + sum (n - i) d_i, both modulo 65521; the sums are kept in 64 bits (n <= 2^30: no overflow).
// Ordering.  With read-back a lane loads bytes that ANOTHER lane of the same wave stored (lane 0 a literal, any lane a byte of an earlier
// match).  The compiler orders a thread's own accesses only, so a fence stands between the stores and the next loads of the window (in
// front of every match copy and of the checksum); the hardware performs one wave's vector memory operations in order.
// Source.  The source bytes are only read and never overlap the staged buffer (refused on the host), so the kernel takes them as
// `const __restrict__`: the bit reader's aligned word loads become scalar loads, off the vector memory counter the byte stores are on.
// The record table lives in device memory, so the kernel trusts no record: one that does not fit the buffers gets DD_INFLATE_RECORD and
// nothing is read or written through it.  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"
#include "dd_inflate_core.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kLanes = 64;
constexpr int kMaxStreamBytes = 1 << 30;

// a lane's earlier stores to the staged buffer are ordered before the wave's later loads from it (see Ordering above)
__device__ __forceinline__ void window_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

struct WaveSink {
  unsigned char* out;
  int lane;

  __device__ __forceinline__ void literal(int at, unsigned value) {
    if (lane == 0) out[at] = (unsigned char)value;
  }

  __device__ __forceinline__ void stored(int at, const unsigned char* from, int n) {
    for (int i = lane; i < n; i += kLanes) out[at + i] = from[i];
  }

  __device__ __forceinline__ void match(int at, int distance, int length) {
    window_fence();
    const unsigned char* from = out + (at - distance);
    if (distance >= length) {
      for (int i = lane; i < length; i += kLanes) out[at + i] = from[i];
    } else {                                                 // the match runs into itself: the `distance` bytes repeat
      for (int i = lane; i < length; i += kLanes) out[at + i] = from[i % distance];
    }
  }

  __device__ __forceinline__ unsigned adler(int n) {
    window_fence();
    unsigned long long a = 0ull, b = 0ull, t = 0ull;         // sum d, sum (n - group start) * (group's sum), sum (index in group) * d
    const int groups = n >> 4;
    for (int g = lane; g < groups; g += kLanes) {
      const uint4 v = *reinterpret_cast<const uint4*>(out + ((long)g << 4));
      unsigned s = 0u, weighted = 0u;
      const unsigned words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned w = words[k];
        const unsigned b0 = w & 0xffu, b1 = (w >> 8) & 0xffu, b2 = (w >> 16) & 0xffu, b3 = w >> 24;
        const unsigned sum = b0 + b1 + b2 + b3;
        weighted += 4u * k * sum + b1 + 2u * b2 + 3u * b3;
        s += sum;
      }
      a += s;
      b += (unsigned long long)(n - (g << 4)) * s;
      t += weighted;
    }
    if (lane == 0)
      for (int i = groups << 4; i < n; ++i) {                // (the bytes behind n up to the next multiple of 16 are not the stream's)
        const unsigned d = out[i];
        a += d;
        b += (unsigned long long)(n - i) * d;
      }
    for (int delta = 32; delta >= 1; delta >>= 1) {
      a += __shfl_down(a, delta);
      b += __shfl_down(b, delta);
      t += __shfl_down(t, delta);
    }
    a = __shfl(a, 0);
    b = __shfl(b, 0);
    t = __shfl(t, 0);
    const unsigned long long m = 65521ull;
    const unsigned lo = (unsigned)((1ull + a) % m);
    const unsigned hi = (unsigned)(((unsigned long long)n % m + b % m + m - t % m) % m);
    return (hi << 16) | lo;
  }
};

__global__ __launch_bounds__(kLanes) void exr_inflate_kernel(const dd_exr_stream* __restrict__ streams, const unsigned char* __restrict__ src, long src_total,
                                                             unsigned char* staged, long staged_bytes, int* __restrict__ status) {
  __shared__ dd_inflate_tables tables;
  const int lane = threadIdx.x;
  const dd_exr_stream r = streams[blockIdx.x];
  // ---- the record is checked before anything is read or written through it (uniform: the wave leaves together)
  const bool source_fits = r.src_bytes >= 1 && r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes;
  const bool size_fits = r.dst_bytes >= 1 && r.dst_bytes <= kMaxStreamBytes;
  const bool place_fits = r.dst_offset >= 0 && (r.dst_offset & 15) == 0 && size_fits && r.dst_offset <= staged_bytes - (((long)r.dst_bytes + 15) & ~15l);
  if (!(source_fits && size_fits && place_fits)) {
    if (lane == 0) status[blockIdx.x] = DD_INFLATE_RECORD;
    return;
  }
  WaveSink sink{staged + r.dst_offset, lane};
  const int result = dd_inflate_stream(src + r.src_offset, r.src_bytes, r.dst_bytes, &tables, sink);
  if (lane == 0) status[blockIdx.x] = result;
}

}  // namespace

extern "C" int dd_exr_inflate(const dd_exr_stream* streams_host, const dd_exr_stream* streams, int n_streams, const void* src, long src_total,
                              void* staged, long staged_bytes, int* status, dd_stream stream) {
  DD_REQUIRE(n_streams >= 0, "dd_exr_inflate: n_streams=%d", n_streams);
  if (n_streams == 0) return DD_OK;
  DD_REQUIRE(streams_host && streams, "dd_exr_inflate: null stream table");
  DD_REQUIRE(src && staged && status, "dd_exr_inflate: null source, staged buffer or status array");
  {
    const char* s0 = static_cast<const char*>(src);
    const char* d0 = static_cast<const char*>(staged);
    DD_REQUIRE(src_total < 0 || staged_bytes < 0 || s0 + src_total <= d0 || d0 + staged_bytes <= s0,
               "dd_exr_inflate: the source (%ld bytes) and the staged buffer (%ld bytes) overlap", src_total, staged_bytes);
  }
  for (int k = 0; k < n_streams; ++k) {
    const dd_exr_stream& r = streams_host[k];
    DD_REQUIRE(r.src_bytes >= 1, "dd_exr_inflate: stream %d: src_bytes=%d", k, r.src_bytes);
    DD_REQUIRE(r.dst_bytes >= 1 && r.dst_bytes <= kMaxStreamBytes, "dd_exr_inflate: stream %d: dst_bytes=%d (1 .. %d)", k, r.dst_bytes, kMaxStreamBytes);
    DD_REQUIRE(r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes, "dd_exr_inflate: stream %d: src_offset=%lld (%d bytes) leaves the %ld source bytes",
               k, r.src_offset, r.src_bytes, src_total);
    DD_REQUIRE(r.dst_offset >= 0 && (r.dst_offset & 15) == 0, "dd_exr_inflate: stream %d: dst_offset=%lld is negative or not 16-byte aligned", k, r.dst_offset);
    DD_REQUIRE(r.dst_offset <= staged_bytes - (((long)r.dst_bytes + 15) & ~15l), "dd_exr_inflate: stream %d: dst_offset=%lld (%d bytes) leaves the %ld staged bytes", k,
               r.dst_offset, r.dst_bytes, staged_bytes);
  }
  hipLaunchKernelGGL(exr_inflate_kernel, dim3(n_streams), dim3(kLanes), 0, S(stream), streams, reinterpret_cast<const unsigned char*>(src), src_total,
                     reinterpret_cast<unsigned char*>(staged), staged_bytes, status);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
