// NaN / Inf samples of render passes (include/dd_hip.h, dd_nonfinite_desc): find them, say where they are, and fill them in from their
// finite neighbours, all in device memory in front of the forward graph:
//   dd_nonfinite_scan    one streaming read of every plane of the table -> one mask byte per pixel (bit c: channel c is inf / NaN) and exact
//                        integer counts per plane
//   dd_nonfinite_repair  in place: a masked value becomes the mean of the unmasked values of its channel in the (2 radius + 1)^2 window;
//                        a workgroup of a plane whose count is zero returns at its first branch
// Both take the whole table in ONE launch (the plane in blockIdx.y).  Plain HBM-streaming kernels of the csrc/dd_pointwise.hip family: no LDS,
// no inline assembly.
#include "dd_frame_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 1024;      // per plane; the rest is taken grid-stride

// inf or NaN <=> all eight exponent bits set: the test of csrc/dd_loss_scale.hip (on the bits, nothing a fast-math build may fold away)
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// the mask byte of one pixel read value by value (any ld, any alignment)
__device__ __forceinline__ unsigned pixel_mask(const float* __restrict__ px, int C) {
  unsigned m = nonfinite_bits(__float_as_uint(px[0]));
  if (C == 3) m |= (nonfinite_bits(__float_as_uint(px[1])) << 1) | (nonfinite_bits(__float_as_uint(px[2])) << 2);
  return m;
}

// Dense planes (ld == C, 16-byte aligned data, 4-byte aligned mask): a thread takes FOUR pixels -- one (C = 1) or three (C = 3) 16-byte loads --
// and writes their four mask bytes as one 32-bit word, so no two threads share a mask word.  Everything else, and the last npix % 4 pixels of a
// dense plane, goes pixel by pixel.  Every lane reaches the wave reduction; a wave that saw nothing -- every wave of a clean frame -- issues
// no atomic.
__global__ __launch_bounds__(kThreads) void nonfinite_scan_kernel(const dd_nonfinite_desc d, long npix, unsigned long long* __restrict__ counts) {
  const int plane = blockIdx.y;
  const float* __restrict__ data = d.plane[plane].data;
  unsigned char* __restrict__ mask = d.plane[plane].mask;
  const int C = d.plane[plane].C, ld = d.plane[plane].ld;
  const bool dense = ld == C && (reinterpret_cast<uintptr_t>(data) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const long tid = blockIdx.x * (long)kThreads + threadIdx.x, stride = (long)gridDim.x * kThreads;
  unsigned values = 0u, pixels = 0u;
  long first_single = 0;      // pixels from here on are taken one by one
  if (dense) {
    const long ngroups = npix >> 2;
    const uint4* __restrict__ dv = reinterpret_cast<const uint4*>(data);
    unsigned* __restrict__ mv = reinterpret_cast<unsigned*>(mask);
    for (long g = tid; g < ngroups; g += stride) {
      unsigned m0, m1, m2, m3;
      if (C == 3) {
        const uint4 a = dv[3 * g], b = dv[3 * g + 1], c = dv[3 * g + 2];      // pixels (a.x a.y a.z) (a.w b.x b.y) (b.z b.w c.x) (c.y c.z c.w)
        m0 = nonfinite_bits(a.x) | (nonfinite_bits(a.y) << 1) | (nonfinite_bits(a.z) << 2);
        m1 = nonfinite_bits(a.w) | (nonfinite_bits(b.x) << 1) | (nonfinite_bits(b.y) << 2);
        m2 = nonfinite_bits(b.z) | (nonfinite_bits(b.w) << 1) | (nonfinite_bits(c.x) << 2);
        m3 = nonfinite_bits(c.y) | (nonfinite_bits(c.z) << 1) | (nonfinite_bits(c.w) << 2);
      } else {
        const uint4 a = dv[g];
        m0 = nonfinite_bits(a.x); m1 = nonfinite_bits(a.y); m2 = nonfinite_bits(a.z); m3 = nonfinite_bits(a.w);
      }
      const unsigned word = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
      mv[g] = word;
      if (word != 0u) {
        values += __popc(word);
        pixels += (m0 != 0u) + (m1 != 0u) + (m2 != 0u) + (m3 != 0u);
      }
    }
    first_single = ngroups << 2;
  }
  for (long p = first_single + tid; p < npix; p += stride) {
    const unsigned m = pixel_mask(data + p * ld, C);
    mask[p] = (unsigned char)m;
    values += __popc(m);
    pixels += m != 0u;
  }
  // (every lane of the wave is back here)
  const unsigned wv = wave_sum(values), wp = wave_sum(pixels);
  if ((threadIdx.x & 63) == 0 && wp != 0u) {
    atomicAdd(&counts[2 * plane], (unsigned long long)wv);
    atomicAdd(&counts[2 * plane + 1], (unsigned long long)wp);
  }
}

// The mean of the usable neighbours of pixel (n, y, x), channel c.  Usable is decided from the MASK alone, never from the live values: the
// kernel writes only masked positions and reads only unmasked ones, so the update in place has no race and does not depend on scheduling.
// Row-major window order, fp32 adds, one division.
__device__ __forceinline__ float window_mean(const float* __restrict__ data, const unsigned char* __restrict__ mask, int ld, int c, long image0,
                                             int y, int x, int H, int W, int radius) {
  const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
  float sum = 0.f;
  int n = 0;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const long q = image0 + (long)yy * W + xx;
      if (((mask[q] >> c) & 1u) == 0u) {
        sum = __fadd_rn(sum, data[q * ld + c]);
        ++n;
      }
    }
  return n > 0 ? __fdiv_rn(sum, (float)n) : 0.f;
}

// A thread reads the mask bytes of four consecutive pixels (one 32-bit load where the mask plane is 4-byte aligned) and goes on at once when
// they are all zero: on a frame with a handful of bad samples the launch is one read of the mask planes.
__global__ __launch_bounds__(kThreads) void nonfinite_repair_kernel(const dd_nonfinite_desc d, int H, int W, long npix, int radius,
                                                                    const unsigned long long* __restrict__ counts) {
  const int plane = blockIdx.y;
  if (counts[2 * plane + 1] == 0ull) return;      // uniform over the plane's workgroups: a clean plane costs this one load
  float* __restrict__ data = d.plane[plane].data;
  const unsigned char* __restrict__ mask = d.plane[plane].mask;
  const int C = d.plane[plane].C, ld = d.plane[plane].ld;
  const bool words = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const long hw = (long)H * W, ngroups = (npix + 3) >> 2;
  for (long g = blockIdx.x * (long)kThreads + threadIdx.x; g < ngroups; g += (long)gridDim.x * kThreads) {
    const long p0 = g << 2;
    unsigned word = 0u;
    if (words && p0 + 4 <= npix) {
      word = *reinterpret_cast<const unsigned*>(mask + p0);
    } else {
      for (int j = 0; j < 4 && p0 + j < npix; ++j) word |= (unsigned)mask[p0 + j] << (8 * j);
    }
    if (word == 0u) continue;
    for (int j = 0; j < 4; ++j) {
      const unsigned m = (word >> (8 * j)) & 0xffu;
      if (m == 0u) continue;
      const long p = p0 + j, image0 = p / hw * hw;      // (the window never reaches into image n +- 1)
      const int rem = (int)(p - image0), y = rem / W, x = rem - y * W;
      for (int c = 0; c < C; ++c)
        if ((m >> c) & 1u) data[p * ld + c] = window_mean(data, mask, ld, c, image0, y, x, H, W, radius);
    }
  }
}

int check_table(const char* who, const dd_nonfinite_desc* desc, int N, int H, int W, const void* counts) {
  DD_REQUIRE(desc != nullptr, "%s: null plane table", who);
  DD_REQUIRE(counts != nullptr, "%s: null counts", who);
  DD_REQUIRE(desc->n_planes >= 1 && desc->n_planes <= DD_NONFINITE_MAX_PLANES, "%s: %d planes (1 .. %d)", who, desc->n_planes, DD_NONFINITE_MAX_PLANES);
  DD_REQUIRE(N > 0 && H > 0 && W > 0, "%s: N, H, W must be positive (%d, %d, %d)", who, N, H, W);
  DD_REQUIRE((long)N * H * W <= 0x7fffffffL, "%s: %d x %d x %d pixels exceed the 32-bit pixel index", who, N, H, W);
  for (int i = 0; i < desc->n_planes; ++i) {
    const dd_nonfinite_plane& p = desc->plane[i];
    DD_REQUIRE(p.data != nullptr && p.mask != nullptr, "%s: plane %d has a null data or mask pointer", who, i);
    DD_REQUIRE(p.C == 1 || p.C == 3, "%s: plane %d has %d channels (1 or 3)", who, i, p.C);
    DD_REQUIRE(p.ld >= p.C, "%s: plane %d has ld %d < C %d", who, i, p.ld, p.C);
  }
  return DD_OK;
}

unsigned blocks_for(long work_items) {
  const long want = (work_items + kThreads - 1) / kThreads;
  return (unsigned)(want < 1 ? 1 : (want < kMaxBlocksX ? want : kMaxBlocksX));
}

}  // namespace

extern "C" int dd_nonfinite_scan(const dd_nonfinite_desc* desc, int N, int H, int W, uint64_t* counts, dd_stream stream) {
  if (int rc = check_table("dd_nonfinite_scan", desc, N, H, W, counts)) return rc;
  const long npix = (long)N * H * W;
  hipLaunchKernelGGL(nonfinite_scan_kernel, dim3(blocks_for((npix + 3) >> 2), (unsigned)desc->n_planes), dim3(kThreads), 0, S(stream), *desc, npix,
                     reinterpret_cast<unsigned long long*>(counts));
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" int dd_nonfinite_repair(const dd_nonfinite_desc* desc, int N, int H, int W, int radius, const uint64_t* counts, dd_stream stream) {
  if (int rc = check_table("dd_nonfinite_repair", desc, N, H, W, counts)) return rc;
  DD_REQUIRE(radius >= 1 && radius <= 4, "dd_nonfinite_repair: radius %d (1 .. 4)", radius);
  const long npix = (long)N * H * W;
  hipLaunchKernelGGL(nonfinite_repair_kernel, dim3(blocks_for((npix + 3) >> 2), (unsigned)desc->n_planes), dim3(kThreads), 0, S(stream), *desc, H, W,
                     npix, radius, reinterpret_cast<const unsigned long long*>(counts));
  DD_LAUNCH_CHECK();
  return DD_OK;
}
