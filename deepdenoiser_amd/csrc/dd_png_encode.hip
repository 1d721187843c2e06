// Denoised passes written as 8-bit sRGB PNGs, encoded on the device (include/dd_hip.h: dd_png_pack, dd_png_deflate).  Prediction.py:483-510
// stores .npy only and its own PNG line is commented out; here TWO launches turn the fp32 planes of all passes of a frame into the pieces of
// every file's IDAT stream, and the host (deepdenoiser_amd/png.py: DevicePngEncoder) adds the chunk framing, the combined Adler-32 and the CRC.
//
// png_pack_kernel.  The filtered rows of an image are cut into segments of whole rows; ONE workgroup of 256 threads builds one segment in LDS
// and stores it.  Per row: the threads quantise the row's samples (sample * exposure against the host's threshold table, kept in LDS; the
// binary search of dd_preview.hip) into a row buffer, add the five filters' sums of absolute values with LDS atomics (integers: the order does
// not matter), every thread picks the same type from the five sums, and the threads write the type byte and the filtered bytes behind the rows
// before it in the staging buffer; the row buffer of the row above is kept, so every fp32 sample is read once per segment -- plus the one row
// above the segment, which is quantised again and not stored.  Rows are 1 + W * n bytes long, so no row starts on an aligned address: the
// segment is therefore staged whole in LDS (16-byte aligned there) and leaves as aligned 16-byte words, the padding up to the next multiple
// of 16 as zero.  All byte decisions are dd_png_core.h, shared with the CPU build (tests/png_core_main.cpp).
// LDS: the table 1 KB, two row buffers of DD_PNG_MAX_ROW_BYTES, the staging buffer of DD_PNG_STAGE_BYTES: 61 KB, two workgroups per CU.
//
// png_deflate_kernel.  The shape of exr_deflate_kernel (dd_exr_deflate.hip; what the two share is dd_deflate_launch.h): one wave per segment,
// all segments of all passes in one launch, the coder core dd_deflate_core.h in its segment framing: a raw-deflate body that ends on a
// byte border with an empty stored block, or, for a file's last segment, with the final block; the segment's Adler-32 goes to the host.
//
// Both tables of either launch live in device memory, so the kernels trust no record: one that does not fit its image or the buffers writes
// nothing (pack) or gets DD_DEFLATE_RECORD (deflate); the tests are uniform over the workgroup.  Plain C++: no inline assembly, no scratch.
#include "dd_deflate_launch.h"
#include "dd_png_core.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kMaxPlaneChannels = 32;

// what both the host check and the kernel ask of an image record and of a segment of it -> the segment's bytes, or 0
__host__ __device__ __forceinline__ bool image_fits(const dd_png_image& f) {
  if (f.src == nullptr || f.H < 1 || f.W < 1 || f.C < 1 || f.C > kMaxPlaneChannels || (f.n_channels != 1 && f.n_channels != 3)) return false;
  if ((long)f.H * f.W * f.C > (1l << 40) || (long)f.W * f.n_channels > DD_PNG_MAX_ROW_BYTES) return false;
  const int c0 = f.src_channel[0], c1 = f.n_channels == 3 ? f.src_channel[1] : c0, c2 = f.n_channels == 3 ? f.src_channel[2] : c0;      // (no indexed loop)
  return c0 >= 0 && c0 < f.C && c1 >= 0 && c1 < f.C && c2 >= 0 && c2 < f.C;
}

__host__ __device__ __forceinline__ long segment_bytes(const dd_png_image& f, const dd_png_segment& g) {
  if (g.rows < 1 || g.y0 < 0 || g.y0 > f.H - g.rows) return 0;
  const long n = (long)g.rows * (1 + f.W * f.n_channels);
  return n <= DD_PNG_STAGE_BYTES ? n : 0;
}

__global__ __launch_bounds__(kThreads) void png_pack_kernel(const dd_png_segment* __restrict__ segments, const dd_png_image* __restrict__ images, int n_images,
                                                            const float* __restrict__ thresholds, unsigned char* __restrict__ staged, long staged_bytes) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[DD_PNG_STAGE_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char rows[2][DD_PNG_MAX_ROW_BYTES];
  __shared__ float thr[DD_PNG_THRESHOLDS + 1];
  __shared__ unsigned cost[DD_PNG_FILTERS];
  const int tid = threadIdx.x;
  const dd_png_segment g = segments[blockIdx.x];
  // ---- the records are checked before anything is read or written through them (uniform: the whole workgroup leaves together)
  if (g.image < 0 || g.image >= n_images) return;
  const dd_png_image f = images[g.image];
  if (!image_fits(f)) return;
  const int n = (int)segment_bytes(f, g), n16 = (n + 15) & ~15;
  if (n == 0 || g.offset < 0 || (g.offset & 15) != 0 || g.offset > staged_bytes - n16) return;
  const int bpp = f.n_channels, nbytes = f.W * bpp;
  const int channel[3] = {f.src_channel[0], f.src_channel[bpp == 3 ? 1 : 0], f.src_channel[bpp == 3 ? 2 : 0]};
  if (tid < DD_PNG_THRESHOLDS) thr[tid] = thresholds[tid];
  __syncthreads();
  if (g.y0 > 0)      // the row above the segment: quantised again, not stored (the first row's sync stands before its first reader)
    dd_png_quantise_row(thr, f.src + (long)(g.y0 - 1) * f.W * f.C, f.W, f.C, bpp, channel, f.exposure, tid, kThreads, rows[0]);
  for (int r = 0; r < g.rows; ++r) {
    unsigned char* cur = rows[(r + 1) & 1];
    const unsigned char* up = (g.y0 + r > 0) ? rows[r & 1] : nullptr;
    dd_png_quantise_row(thr, f.src + (long)(g.y0 + r) * f.W * f.C, f.W, f.C, bpp, channel, f.exposure, tid, kThreads, cur);
    if (tid < DD_PNG_FILTERS) cost[tid] = 0u;
    __syncthreads();
    unsigned mine[DD_PNG_FILTERS] = {0u, 0u, 0u, 0u, 0u};
    dd_png_row_costs(cur, up, nbytes, bpp, tid, kThreads, mine);
#pragma unroll
    for (int t = 0; t < DD_PNG_FILTERS; ++t)
      if (mine[t] != 0u) atomicAdd(cost + t, mine[t]);
    __syncthreads();
    dd_png_write_row(dd_png_pick(cost), cur, up, nbytes, bpp, tid, kThreads, stage + (long)r * (1 + nbytes));
    __syncthreads();      // (the next row overwrites the buffer of the row above, and the sums)
  }
  if (tid < n16 - n) stage[n + tid] = 0;
  __syncthreads();
  unsigned char* out = staged + g.offset;
  for (int i0 = tid * 16; i0 < n16; i0 += kThreads * 16) *reinterpret_cast<uint4*>(out + i0) = *reinterpret_cast<const uint4*>(stage + i0);
}

__global__ __launch_bounds__(kLanes) void png_deflate_kernel(const dd_png_stream* __restrict__ streams, const unsigned char* __restrict__ src, long src_total,
                                                             unsigned char* out, long out_bytes, unsigned* workspace, int* __restrict__ status,
                                                             int* __restrict__ sizes, unsigned* __restrict__ adler) {
  __shared__ dd_deflate_state state;
  const int lane = threadIdx.x;
  const dd_png_stream r = streams[blockIdx.x];
  // ---- the record is checked before anything is read or written through it (uniform: the wave leaves together)
  if (!(deflate_record_fits(r, src_total, out_bytes) && (r.last == 0 || r.last == 1))) {
    if (lane == 0) {
      status[blockIdx.x] = DD_DEFLATE_RECORD;
      sizes[blockIdx.x] = 0;
      adler[blockIdx.x] = 0u;
    }
    return;
  }
  WaveOut sink{out + r.dst_offset};
  int size = 0;
  unsigned check = 0u;
  const int result = dd_deflate_segment(src + r.src_offset, r.src_bytes, r.dst_capacity, r.last != 0, workspace + (long)blockIdx.x * DD_DEFLATE_BLOCK_TOKENS, &state,
                                        sink, &size, &check);
  if (lane == 0) {
    status[blockIdx.x] = result;
    sizes[blockIdx.x] = result == DD_DEFLATE_OK ? size : 0;
    adler[blockIdx.x] = check;
  }
}

}  // namespace

extern "C" int dd_png_pack(const dd_png_segment* segments_host, const dd_png_segment* segments, int n_segments, const dd_png_image* images_host,
                           const dd_png_image* images, int n_images, const float* thresholds, void* staged, long staged_bytes, dd_stream stream) {
  DD_REQUIRE(n_segments >= 0, "dd_png_pack: n_segments=%d", n_segments);
  if (n_segments == 0) return DD_OK;
  DD_REQUIRE(segments_host && segments && images_host && images, "dd_png_pack: null segment or image table");
  DD_REQUIRE(thresholds, "dd_png_pack: no threshold table (thresholds is null)");
  DD_REQUIRE((reinterpret_cast<unsigned long long>(thresholds) & 3ull) == 0ull, "dd_png_pack: thresholds must be 4-byte aligned");
  DD_REQUIRE(staged, "dd_png_pack: null staged buffer");
  DD_REQUIRE((reinterpret_cast<unsigned long long>(staged) & 15ull) == 0ull, "dd_png_pack: the staged buffer is not 16-byte aligned");
  DD_REQUIRE(n_images >= 1, "dd_png_pack: n_images=%d", n_images);
  DD_REQUIRE(staged_bytes >= 16, "dd_png_pack: staged_bytes=%ld", staged_bytes);
  for (int k = 0; k < n_images; ++k) {
    const dd_png_image& f = images_host[k];
    DD_REQUIRE(f.src, "dd_png_pack: image %d has a null plane", k);
    DD_REQUIRE(f.H >= 1 && f.W >= 1, "dd_png_pack: image %d: H=%d W=%d", k, f.H, f.W);
    DD_REQUIRE(f.C >= 1 && f.C <= kMaxPlaneChannels, "dd_png_pack: image %d: C=%d (a plane has 1 .. %d channels)", k, f.C, kMaxPlaneChannels);
    DD_REQUIRE((long)f.H * f.W * f.C <= (1l << 40), "dd_png_pack: image %d: %d x %d x %d samples", k, f.H, f.W, f.C);
    DD_REQUIRE(f.n_channels == 1 || f.n_channels == 3, "dd_png_pack: image %d: n_channels=%d (1 gray, 3 RGB)", k, f.n_channels);
    for (int c = 0; c < f.n_channels; ++c)
      DD_REQUIRE(f.src_channel[c] >= 0 && f.src_channel[c] < f.C, "dd_png_pack: image %d channel %d: src_channel=%d outside the C=%d of the plane", k, c,
                 f.src_channel[c], f.C);
    DD_REQUIRE((long)f.W * f.n_channels <= DD_PNG_MAX_ROW_BYTES, "dd_png_pack: image %d: a row of %ld bytes (the pack kernel's LDS holds %d)", k,
               (long)f.W * f.n_channels, DD_PNG_MAX_ROW_BYTES);
    const char* s0 = reinterpret_cast<const char*>(f.src);
    const char* d0 = static_cast<const char*>(staged);
    const long plane_bytes = (long)f.H * f.W * f.C * 4;
    DD_REQUIRE(s0 + plane_bytes <= d0 || d0 + staged_bytes <= s0, "dd_png_pack: image %d: the plane (%ld bytes) and the staged buffer (%ld bytes) overlap", k,
               plane_bytes, staged_bytes);
  }
  for (int k = 0; k < n_segments; ++k) {
    const dd_png_segment& g = segments_host[k];
    DD_REQUIRE(g.image >= 0 && g.image < n_images, "dd_png_pack: segment %d: image=%d of %d", k, g.image, n_images);
    const dd_png_image& f = images_host[g.image];
    DD_REQUIRE(g.rows >= 1, "dd_png_pack: segment %d: rows=%d", k, g.rows);
    DD_REQUIRE(g.y0 >= 0 && g.y0 <= f.H - g.rows, "dd_png_pack: segment %d: y0=%d rows=%d outside the %d rows of image %d", k, g.y0, g.rows, f.H, g.image);
    const long n = segment_bytes(f, g);
    DD_REQUIRE(n != 0, "dd_png_pack: segment %d: rows=%d of %d bytes (the pack kernel stages %d bytes)", k, g.rows, 1 + f.W * f.n_channels, DD_PNG_STAGE_BYTES);
    DD_REQUIRE(g.offset >= 0 && (g.offset & 15) == 0 && g.offset <= staged_bytes - ((n + 15) & ~15l),
               "dd_png_pack: segment %d: offset=%lld (%ld bytes) is not 16-byte aligned or leaves the %ld staged bytes", k, (long long)g.offset, n, staged_bytes);
  }
  hipLaunchKernelGGL(png_pack_kernel, dim3(n_segments), dim3(kThreads), 0, S(stream), segments, images, n_images, thresholds,
                     reinterpret_cast<unsigned char*>(staged), staged_bytes);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" long dd_png_deflate_workspace(int n_streams) { return deflate_workspace_bytes(n_streams); }

extern "C" int dd_png_deflate(const dd_png_stream* streams_host, const dd_png_stream* streams, int n_streams, const void* src, long src_total, void* out,
                              long out_bytes, void* workspace, long workspace_bytes, int* status, int* sizes, unsigned* adler, dd_stream stream) {
  const int rc = deflate_check("dd_png_deflate", streams_host, streams, n_streams, src, src_total, out, out_bytes, workspace, workspace_bytes,
                               status && sizes && adler, "status, size or adler array", [](int k, const dd_png_stream& r) {
                                 DD_REQUIRE(r.last == 0 || r.last == 1, "dd_png_deflate: stream %d: last=%d (0 or 1)", k, r.last);
                                 return DD_OK;
                               });
  if (rc != DD_OK || n_streams == 0) return rc;
  hipLaunchKernelGGL(png_deflate_kernel, dim3(n_streams), dim3(kLanes), 0, S(stream), streams, reinterpret_cast<const unsigned char*>(src), src_total,
                     reinterpret_cast<unsigned char*>(out), out_bytes, reinterpret_cast<unsigned*>(workspace), status, sizes, adler);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
