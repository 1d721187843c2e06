// The packed chunks of OpenEXR ZIP / ZIPS files deflated on the device (include/dd_hip.h, dd_exr_deflate): ONE launch turns every chunk of a
// batch (dd_exr_pack's output, dd_exr_encode.hip, the launch before on the same stream) into a zlib stream; the host downloads the streams and
// writes headers and offset tables (deepdenoiser_amd/openexr.py: DeviceEncoder).
//
// Shape.  Streams are independent (a 1080p frame with all passes has about a thousand of them), so ONE WAVE codes ONE stream: a workgroup is a
// single wave and there is no barrier.  Unlike inflate, deflate has parallel phases inside a stream -- 64 positions are matched per step, 64
// tokens are emitted per step -- and the whole coder, with every bound and every status, is the shared core (dd_deflate_core.h): its
// DD_FOR_LANES bodies run on the 64 lanes here and as a loop in the CPU build, with identical bytes.  This file supplies where the state lives
// (LDS, about 41 KB per wave: the hash table is 32 KB of it), where the tokens go (the stream's slice of the workspace in device memory) and
// how words are stored.  The LDS atomics (max on the hash table, add on the histograms, or on the bit window) are ordinary vector LDS
// operations.  The record table lives in device memory, so the kernel trusts no record: one that does not fit the buffers gets
// DD_DEFLATE_RECORD and nothing is read or written through it.  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"
#include "dd_deflate_core.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kLanes = DD_DEFLATE_LANES;
constexpr long kSliceBytes = (long)DD_DEFLATE_BLOCK_TOKENS * 4;

struct WaveOut {
  unsigned char* at0;      // 16-byte aligned
  __device__ __forceinline__ void word(int at, unsigned v) { *reinterpret_cast<unsigned*>(at0 + at) = v; }
  __device__ __forceinline__ void byte(int at, unsigned v) { at0[at] = (unsigned char)v; }
};

__global__ __launch_bounds__(kLanes) void exr_deflate_kernel(const dd_exr_deflate_stream* __restrict__ streams, const unsigned char* __restrict__ src,
                                                             long src_total, unsigned char* out, long out_bytes, unsigned* workspace,
                                                             int* __restrict__ status, int* __restrict__ sizes) {
  __shared__ dd_deflate_state state;
  const int lane = threadIdx.x;
  const dd_exr_deflate_stream r = streams[blockIdx.x];
  // ---- the record is checked before anything is read or written through it (uniform: the wave leaves together)
  const bool source_fits = r.src_bytes >= 1 && r.src_bytes <= DD_DEFLATE_MAX_BYTES && r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes;
  const bool capacity_fits = r.dst_capacity >= 0 && r.dst_capacity <= DD_DEFLATE_MAX_BYTES;
  const bool place_fits = capacity_fits && r.dst_offset >= 0 && (r.dst_offset & 15) == 0 && r.dst_offset <= out_bytes - (((long)r.dst_capacity + 15) & ~15l);
  if (!(source_fits && place_fits)) {
    if (lane == 0) {
      status[blockIdx.x] = DD_DEFLATE_RECORD;
      sizes[blockIdx.x] = 0;
    }
    return;
  }
  WaveOut sink{out + r.dst_offset};
  int size = 0;
  const int result = dd_deflate_stream(src + r.src_offset, r.src_bytes, r.dst_capacity, workspace + (long)blockIdx.x * DD_DEFLATE_BLOCK_TOKENS, &state, sink, &size);
  if (lane == 0) {
    status[blockIdx.x] = result;
    sizes[blockIdx.x] = result == DD_DEFLATE_OK ? size : 0;
  }
}

}  // namespace

extern "C" long dd_exr_deflate_workspace(int n_streams) { return n_streams > 0 ? (long)n_streams * kSliceBytes : 0l; }

extern "C" int dd_exr_deflate(const dd_exr_deflate_stream* streams_host, const dd_exr_deflate_stream* streams, int n_streams, const void* src, long src_total,
                              void* out, long out_bytes, void* workspace, long workspace_bytes, int* status, int* sizes, dd_stream stream) {
  DD_REQUIRE(n_streams >= 0, "dd_exr_deflate: n_streams=%d", n_streams);
  if (n_streams == 0) return DD_OK;
  DD_REQUIRE(streams_host && streams, "dd_exr_deflate: null stream table");
  DD_REQUIRE(src && out && workspace && status && sizes, "dd_exr_deflate: null source, output, workspace, status or size array");
  DD_REQUIRE((reinterpret_cast<unsigned long long>(out) & 15ull) == 0ull && (reinterpret_cast<unsigned long long>(workspace) & 3ull) == 0ull,
             "dd_exr_deflate: the output is not 16-byte aligned or the workspace not 4-byte aligned");
  DD_REQUIRE(workspace_bytes >= dd_exr_deflate_workspace(n_streams), "dd_exr_deflate: workspace_bytes=%ld, %d streams need %ld", workspace_bytes, n_streams,
             dd_exr_deflate_workspace(n_streams));
  {
    const char* s0 = static_cast<const char*>(src);
    const char* d0 = static_cast<const char*>(out);
    DD_REQUIRE(src_total < 0 || out_bytes < 0 || s0 + src_total <= d0 || d0 + out_bytes <= s0,
               "dd_exr_deflate: the source (%ld bytes) and the output (%ld bytes) overlap", src_total, out_bytes);
  }
  for (int k = 0; k < n_streams; ++k) {
    const dd_exr_deflate_stream& r = streams_host[k];
    DD_REQUIRE(r.src_bytes >= 1 && r.src_bytes <= DD_DEFLATE_MAX_BYTES, "dd_exr_deflate: stream %d: src_bytes=%d (1 .. %d)", k, r.src_bytes, DD_DEFLATE_MAX_BYTES);
    DD_REQUIRE(r.dst_capacity >= 0 && r.dst_capacity <= DD_DEFLATE_MAX_BYTES, "dd_exr_deflate: stream %d: dst_capacity=%d", k, r.dst_capacity);
    DD_REQUIRE(r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes, "dd_exr_deflate: stream %d: src_offset=%lld (%d bytes) leaves the %ld source bytes",
               k, r.src_offset, r.src_bytes, src_total);
    DD_REQUIRE(r.dst_offset >= 0 && (r.dst_offset & 15) == 0, "dd_exr_deflate: stream %d: dst_offset=%lld is negative or not 16-byte aligned", k, r.dst_offset);
    DD_REQUIRE(r.dst_offset <= out_bytes - (((long)r.dst_capacity + 15) & ~15l), "dd_exr_deflate: stream %d: dst_offset=%lld (capacity %d) leaves the %ld output bytes",
               k, r.dst_offset, r.dst_capacity, out_bytes);
  }
  hipLaunchKernelGGL(exr_deflate_kernel, dim3(n_streams), dim3(kLanes), 0, S(stream), streams, reinterpret_cast<const unsigned char*>(src), src_total,
                     reinterpret_cast<unsigned char*>(out), out_bytes, reinterpret_cast<unsigned*>(workspace), status, sizes);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
