// The packed chunks of OpenEXR ZIP / ZIPS files deflated on the device (include/dd_hip.h, dd_exr_deflate): ONE launch turns every chunk of a
// batch (dd_exr_pack's output, dd_exr_encode.hip, the launch before on the same stream) into a zlib stream; the host downloads the streams and
// writes headers and offset tables (deepdenoiser_amd/openexr/encode.py: DeviceEncoder).
//
// Shape.  Streams are independent (a 1080p frame with all passes has about a thousand of them), so ONE WAVE codes ONE stream: a workgroup is a
// single wave and there is no barrier.  Unlike inflate, deflate has parallel phases inside a stream -- 64 positions are matched per step, 64
// tokens are emitted per step -- and the whole coder, with every bound and every status, is the shared core (dd_deflate_core.h): its
// DD_FOR_LANES bodies run on the 64 lanes here and as a loop in the CPU build, with identical bytes.  This file supplies where the state lives
// (LDS, about 41 KB per wave: the hash table is 32 KB of it), where the tokens go (the stream's slice of the workspace in device memory) and
// how words are stored.  The LDS atomics (max on the hash table, add on the histograms, or on the bit window) are ordinary vector LDS
// operations.  The record table lives in device memory, so the kernel trusts no record: one that does not fit the buffers gets
// DD_DEFLATE_RECORD and nothing is read or written through it.  The sink, the workspace slices, that record test and the entry point's
// argument checks are dd_deflate_launch.h, shared with png_deflate_kernel.  Plain C++: no inline assembly, no scratch.
#include "dd_deflate_launch.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

__global__ __launch_bounds__(kLanes) void exr_deflate_kernel(const dd_exr_deflate_stream* __restrict__ streams, const unsigned char* __restrict__ src,
                                                             long src_total, unsigned char* out, long out_bytes, unsigned* workspace,
                                                             int* __restrict__ status, int* __restrict__ sizes) {
  __shared__ dd_deflate_state state;
  const int lane = threadIdx.x;
  const dd_exr_deflate_stream r = streams[blockIdx.x];
  // ---- the record is checked before anything is read or written through it (uniform: the wave leaves together)
  if (!deflate_record_fits(r, src_total, out_bytes)) {
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

extern "C" long dd_exr_deflate_workspace(int n_streams) { return deflate_workspace_bytes(n_streams); }

extern "C" int dd_exr_deflate(const dd_exr_deflate_stream* streams_host, const dd_exr_deflate_stream* streams, int n_streams, const void* src, long src_total,
                              void* out, long out_bytes, void* workspace, long workspace_bytes, int* status, int* sizes, dd_stream stream) {
  const int rc = deflate_check("dd_exr_deflate", streams_host, streams, n_streams, src, src_total, out, out_bytes, workspace, workspace_bytes, status && sizes,
                               "status or size array", [](int, const dd_exr_deflate_stream&) { return DD_OK; });
  if (rc != DD_OK || n_streams == 0) return rc;
  hipLaunchKernelGGL(exr_deflate_kernel, dim3(n_streams), dim3(kLanes), 0, S(stream), streams, reinterpret_cast<const unsigned char*>(src), src_total,
                     reinterpret_cast<unsigned char*>(out), out_bytes, reinterpret_cast<unsigned*>(workspace), status, sizes);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
