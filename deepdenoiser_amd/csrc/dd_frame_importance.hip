// Importance scores of frames that stay in device memory (include/dd_hip.h, dd_importance_desc): ONE launch reduces every G x G cell of a
// table to one double -- the SMAPE of the loss (LossDifference.py:30-34) between each noisy source rendering and the target rendering, summed
// over the cell's pixels, the three channels, the sources and every colour pass that is both a source and a target.  The host turns the cells
// into the density `--frames_crops importance` draws its training windows from (deepdenoiser_amd/frame_importance.py).
//
// Shape.  One WAVE per cell, kWaves cells per workgroup: the host writes the table row-major, so the cells of a workgroup are horizontal
// neighbours and their rows share cache lines.  A lane owns PIXELS l, l + 64, ... of the cell in row-major order; the target pixel of a pass is
// loaded once and compared with every source, so every sample of the colour passes is read exactly once.  No LDS, no barrier.
//
// Arithmetic.  A term is |s - t| / ((|s| + |t|) + epsilon) in fp32 in exactly that order, the division rounded to nearest (no product: nothing
// contracts); the terms are added in double.  Order of the sum (fixed, no atomics: two launches give the same bytes): a lane adds its pixels
// in ascending order, per pixel the passes in order, per pass the sources in order, channels 0 .. 2; the 64 lanes are combined by the
// shift-down tree of dd_frame_statistics.hip (lane i += lane i + 32, 16, 8, 4, 2, 1).  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void frame_importance_kernel(const dd_importance_desc desc, const dd_importance_cell* __restrict__ cells,
                                                                    int n_cells, int G, double* __restrict__ out) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = blockIdx.x * kWaves + wave;
  if (n >= n_cells) return;                               // (uniform over the wave; the kernel has no barrier)
  const dd_importance_cell r = cells[n];
  // a cell cannot be checked on the host (the table lives in device memory): planes and origins are clamped, so no read leaves a plane
  const int last = desc.n_planes - 1, nsrc = desc.n_sources;
  const int tp = min(max(r.target_plane, 0), last);
  const int sp0 = min(max(r.source_plane0, 0), max(desc.n_planes - nsrc, 0));
  const int th = desc.plane_hw[2 * tp], tw = desc.plane_hw[2 * tp + 1];
  bool fits = th >= G && tw >= G;
  for (int k = 0; k < nsrc && fits; ++k) {
    const int sp = (int)min((long)sp0 + k, (long)last);
    fits = desc.plane_hw[2 * sp] >= G && desc.plane_hw[2 * sp + 1] >= G;
  }
  if (!fits) {                                            // a plane smaller than a cell: the cell scores nothing
    if (lane == 0) out[n] = 0.0;
    return;
  }
  const int ty0 = min(max(r.y0, 0), th - G), tx0 = min(max(r.x0, 0), tw - G);
  const float eps = desc.epsilon;
  const int pixels = G * G;
  double sum = 0.0;
  for (int i = lane; i < pixels; i += 64) {
    const int y = i / G, x = i - y * G;
    const long toff = ((long)(ty0 + y) * tw + (tx0 + x)) * 3;
    for (int p = 0; p < desc.n_passes; ++p) {
      const float* const* planes = desc.pass[p].planes;
      const float* __restrict__ tframe = planes[tp];
      if (tframe == nullptr) continue;
      const float t0 = tframe[toff], t1 = tframe[toff + 1], t2 = tframe[toff + 2];
      const float a0 = fabsf(t0), a1 = fabsf(t1), a2 = fabsf(t2);
      for (int k = 0; k < nsrc; ++k) {
        const int sp = (int)min((long)sp0 + k, (long)last);
        const float* __restrict__ sframe = planes[sp];
        if (sframe == nullptr) continue;
        const int sh = desc.plane_hw[2 * sp], sw = desc.plane_hw[2 * sp + 1];      // (the origin is clamped by THAT plane's size)
        const int sy0 = min(max(r.y0, 0), sh - G), sx0 = min(max(r.x0, 0), sw - G);
        const float* q = sframe + ((long)(sy0 + y) * sw + (sx0 + x)) * 3;
        const float s0 = q[0], s1 = q[1], s2 = q[2];
        sum += (double)__fdiv_rn(fabsf(s0 - t0), (fabsf(s0) + a0) + eps);
        sum += (double)__fdiv_rn(fabsf(s1 - t1), (fabsf(s1) + a1) + eps);
        sum += (double)__fdiv_rn(fabsf(s2 - t2), (fabsf(s2) + a2) + eps);
      }
    }
  }
  // the wave's tree: after the step with delta, lanes 0 .. delta-1 hold the sums of lanes i, i + delta, ...
  for (int delta = 32; delta >= 1; delta >>= 1) sum += __shfl_down(sum, delta);
  if (lane == 0) out[n] = sum;
}

}  // namespace

extern "C" int dd_importance_cells(const dd_importance_desc* desc, const dd_importance_cell* cells, int n_cells, int G, double* out, dd_stream stream) {
  DD_REQUIRE(desc && cells && out, "dd_importance_cells: null descriptor, cell table or output");
  DD_REQUIRE(desc->n_passes >= 1 && desc->n_passes <= DD_IMPORTANCE_MAX_PASSES, "dd_importance_cells: n_passes=%d (1 .. %d passes fit the descriptor)",
             desc->n_passes, DD_IMPORTANCE_MAX_PASSES);
  DD_REQUIRE(desc->plane_hw && desc->n_planes >= 1, "dd_importance_cells: null plane size table or n_planes=%d", desc->n_planes);
  DD_REQUIRE(desc->n_sources >= 1, "dd_importance_cells: n_sources=%d", desc->n_sources);
  DD_REQUIRE(G >= 1 && G <= 64, "dd_importance_cells: G=%d (1 .. 64)", G);
  DD_REQUIRE(n_cells >= 1, "dd_importance_cells: n_cells=%d", n_cells);
  DD_REQUIRE(desc->epsilon > 0.f && desc->epsilon <= 3.402823466e38f, "dd_importance_cells: epsilon=%g (positive and finite)", (double)desc->epsilon);
  for (int i = 0; i < desc->n_passes; ++i)
    DD_REQUIRE(desc->pass[i].planes, "dd_importance_cells: pass %d has a null plane array", i);
  hipLaunchKernelGGL(frame_importance_kernel, dim3(dd_ceil_div(n_cells, kWaves)), dim3(kThreads), 0, S(stream), *desc, cells, n_cells, G, out);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
