// Importance scores refreshed from the running model's error (include/dd_hip.h, dd_importance_update_desc): ONE launch between the forward
// and the backward of a training step scores the mini-batch that was just forwarded -- per G x G cell of the FRAME that lies wholly inside
// an example's window, the SMAPE of the loss (LossDifference.py:30-34) between the prediction and the target of the colour passes -- and adds
// it to two flat integer tables over all cells of all scenes.  The host folds the tables into the density `--frames_crops importance` draws
// from (deepdenoiser_amd/frame_importance.py, ImportanceScorer / ImportanceMap.fold).
//
// Shape.  One WAVE per (example, cell slot), kWaves slots per workgroup, grid = (ceil((T / G)^2 / kWaves), B).  A window whose origin is no
// multiple of G on an axis holds T / G - 1 whole cells there; a slot past the last whole cell returns before doing anything (uniform over the
// wave: the kernel has no barrier).  No LDS.
//
// Geometry.  A lane owns PIXELS l, l + 64, ... of the cell in the FRAME's row-major order.  The frame pixel (fy, fx) of the un-augmented
// window is shown by exactly one pixel of the tile: the inverse of source_pixel (csrc/dd_tile_sampler.hip) for the record's rotate & 3 and
// flip under the two usage switches; prediction and target are read there.  The RGB permutation and the normal rotation do not matter:
// prediction and target carry the same permutation and a term is summed over the three channels.
//
// Arithmetic, as frame_importance_kernel (csrc/dd_frame_importance.hip).  A term is |p - t| / ((|p| + |t|) + epsilon) in fp32 in exactly
// that order, the division rounded to nearest; the terms are added in double: a lane adds its pixels in ascending order, per pixel the
// passes in order, channels 0 .. 2; the 64 lanes are combined by the same shift-down tree.  With the prediction replaced by the sampled source
// tile the sum is the one dd_importance_cells forms.  Lane 0 forms mean = sum / (G G 3 n_passes) and, when it is finite, adds
// llrint(mean 2^32) to acc_sum[cell] and 1 to acc_count[cell] with INTEGER atomics: the tables do not depend on the order of the adds, two runs
// over the same predictions leave the same bytes and data-parallel ranks can add their tables exactly.  Plain C++: no inline assembly, no
// scratch (build.NO_SCRATCH).
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// the pixel (y, x) of the tile that shows pixel (fy, fx) of the un-augmented T x T window: the inverse of source_pixel
__device__ __forceinline__ void tile_pixel(int fy, int fx, int T, int k, bool flip, int& y, int& x) {
  if (flip) fx = T - 1 - fx;
  y = fy; x = fx;
  if (k == 1) { y = T - 1 - fx; x = fy; }
  else if (k == 2) { y = T - 1 - fy; x = T - 1 - fx; }
  else if (k == 3) { y = fx; x = T - 1 - fy; }
}

__global__ __launch_bounds__(kThreads) void importance_update_kernel(const dd_importance_update_desc desc, const dd_tile_record* __restrict__ records,
                                                                     int T, int G, int use_flip, int use_rotate,
                                                                     unsigned long long* __restrict__ acc_sum, unsigned int* __restrict__ acc_count) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int m = T / G;
  const int slot = blockIdx.x * kWaves + wave;
  if (slot >= m * m) return;                              // (uniform over the wave; the kernel has no barrier)
  const int b = blockIdx.y;
  const dd_tile_record& r = records[b];
  // a record cannot be checked on the host (it lives in device memory): plane and origin are clamped as dd_sample_tiles clamps them
  const int plane = min(max(r.target_plane, 0), desc.n_planes - 1);
  const int h = desc.plane_hw[2 * plane], w = desc.plane_hw[2 * plane + 1];
  const int base = desc.cell_base[plane];
  if (h < T || w < T || base < 0) return;                 // a plane smaller than a tile, or one that is no target plane: nothing is added
  const int y0 = min(max(r.y0, 0), h - T), x0 = min(max(r.x0, 0), w - T);
  // the whole cells of the window: cy0 .. cy0 + ny - 1 by cx0 .. cx0 + nx - 1
  const int cy0 = (y0 + G - 1) / G, cx0 = (x0 + G - 1) / G;
  const int ny = (y0 + T) / G - cy0, nx = (x0 + T) / G - cx0;
  const int sy = slot / m, sx = slot - sy * m;
  if (sy >= ny || sx >= nx) return;                       // a slot past the last whole cell
  const int cy = cy0 + sy, cx = cx0 + sx;
  const int wy0 = cy * G - y0, wx0 = cx * G - x0;         // the cell's origin in the un-augmented window, 0 .. T - G
  const int k = use_rotate ? (r.draw.rotate & 3) : 0;
  const bool flip = use_flip && r.draw.flip > 0;
  const float eps = desc.epsilon;
  const int pixels = G * G;
  const long image = (long)b * T * T;
  double sum = 0.0;
  for (int i = lane; i < pixels; i += 64) {
    const int yy = i / G, xx = i - yy * G;
    int y, x;
    tile_pixel(wy0 + yy, wx0 + xx, T, k, flip, y, x);
    const long pix = image + (long)y * T + x;
    for (int p = 0; p < desc.n_passes; ++p) {
      const float* __restrict__ q = desc.pass[p].pred + pix * desc.pass[p].pred_ld;
      const float* __restrict__ t = desc.pass[p].target + pix * desc.pass[p].target_ld;
      const float p0 = q[0], p1 = q[1], p2 = q[2];
      const float t0 = t[0], t1 = t[1], t2 = t[2];
      sum += (double)__fdiv_rn(fabsf(p0 - t0), (fabsf(p0) + fabsf(t0)) + eps);
      sum += (double)__fdiv_rn(fabsf(p1 - t1), (fabsf(p1) + fabsf(t1)) + eps);
      sum += (double)__fdiv_rn(fabsf(p2 - t2), (fabsf(p2) + fabsf(t2)) + eps);
    }
  }
  // the wave's tree: after the step with delta, lanes 0 .. delta-1 hold the sums of lanes i, i + delta, ...
  for (int delta = 32; delta >= 1; delta >>= 1) sum += __shfl_down(sum, delta);
  if (lane == 0) {
    const double mean = sum / ((double)pixels * 3.0 * (double)desc.n_passes);
    if (isfinite(mean)) {                                 // an fp16 overflow or a NaN in a prediction: the cell is not scored
      const long cell = (long)base + (long)cy * (w / G) + cx;
      atomicAdd(acc_sum + cell, (unsigned long long)llrint(mean * 4294967296.0));
      atomicAdd(acc_count + cell, 1u);
    }
  }
}

}  // namespace

extern "C" int dd_importance_update(const dd_importance_update_desc* desc, const dd_tile_record* records, int B, int T, int G, int use_flip,
                                    int use_rotate, unsigned long long* acc_sum, unsigned int* acc_count, dd_stream stream) {
  DD_REQUIRE(desc && records && acc_sum && acc_count, "dd_importance_update: null descriptor, records or accumulators");
  DD_REQUIRE(desc->n_passes >= 1 && desc->n_passes <= DD_IMPORTANCE_MAX_PASSES, "dd_importance_update: n_passes=%d (1 .. %d passes fit the descriptor)",
             desc->n_passes, DD_IMPORTANCE_MAX_PASSES);
  DD_REQUIRE(desc->plane_hw && desc->cell_base && desc->n_planes >= 1, "dd_importance_update: null plane size table or cell_base, or n_planes=%d",
             desc->n_planes);
  DD_REQUIRE(T >= 1 && T <= 32768, "dd_importance_update: T=%d (1 .. 32768)", T);
  DD_REQUIRE(B >= 1 && B <= 65535, "dd_importance_update: B=%d (1 .. 65535)", B);
  DD_REQUIRE(G >= 1 && G <= 64 && T % G == 0, "dd_importance_update: G=%d (1 .. 64, a divisor of T=%d)", G, T);
  DD_REQUIRE(desc->epsilon > 0.f && desc->epsilon <= 3.402823466e38f, "dd_importance_update: epsilon=%g (positive and finite)", (double)desc->epsilon);
  for (int i = 0; i < desc->n_passes; ++i) {
    const dd_importance_update_pass& p = desc->pass[i];
    DD_REQUIRE(p.pred && p.target, "dd_importance_update: pass %d has a null pointer", i);
    DD_REQUIRE(p.pred_ld >= 3, "dd_importance_update: pass %d has pred_ld=%d < 3", i, p.pred_ld);
    DD_REQUIRE(p.target_ld >= 3, "dd_importance_update: pass %d has target_ld=%d < 3", i, p.target_ld);
  }
  const int m = T / G;
  hipLaunchKernelGGL(importance_update_kernel, dim3(dd_ceil_div(m * m, kWaves), B), dim3(kThreads), 0, S(stream), *desc, records, T, G, use_flip,
                     use_rotate, acc_sum, acc_count);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
