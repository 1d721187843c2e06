// Tile staging shared by the tracked-metric kernel (csrc/dd_metrics.hip) and the histogram kernel (csrc/dd_histogram.hip): the 16 x 4 pixel
// tile of one wave (+ one halo column and row for the variation pairs) of a tensor's prediction or target, read into three channel planes
// in LDS -- float4 loads where the rows allow it, element by element where they do not -- and the wave's fixed-order butterfly sum.
#pragma once
#include "dd_common.h"

namespace {

constexpr int MT_W = 16, MT_H = 4;                 // pixels of a tile = lanes of the wave
constexpr int MT_PW = MT_W + 1, MT_PH = MT_H + 1;  // with the right / lower halo
constexpr int MT_TP = MT_PW * MT_PH;
constexpr int MT_FB = 4;                           // features whose loads are in flight together
constexpr int MT_SOURCES = DD_METRIC_SOURCES;

struct Staged {
  float4 q0, q1;
  float h;
};

// Can the 16 pixels x ld floats of every tile row be read as aligned float4s?  (block-uniform)
__device__ __forceinline__ bool rows_vectorise(const float* base, int ld, int W, int x0) {
  return (reinterpret_cast<uintptr_t>(base) & 15) == 0 && x0 + MT_W <= W && (ld == 4 || (ld == 3 && (W & 3) == 0));
}

// Request the tile of one tensor (vector path): up to two float4 per lane for the 16-pixel body, one scalar for the halo column.
__device__ __forceinline__ Staged stage_issue(const float* tile, int ld, bool one, int W, int nrows, bool halo, int lane) {
  Staged s;
  s.q0 = s.q1 = make_float4(0.f, 0.f, 0.f, 0.f);
  s.h = 0.f;
  const int nv = 4 * ld, items = nrows * nv;       // nv = 16 pixels * ld floats / 4
  const long row = (long)W * ld;
  if (lane < items) {
    const int r = ld == 4 ? lane >> 4 : lane / 12, v = lane - r * nv;
    s.q0 = *reinterpret_cast<const float4*>(tile + r * row + 4 * v);
  }
  if (lane + 64 < items) {
    const int it = lane + 64, r = ld == 4 ? it >> 4 : it / 12, v = it - r * nv;
    s.q1 = *reinterpret_cast<const float4*>(tile + r * row + 4 * v);
  }
  if (halo && lane < nrows * 3) {
    const int r = lane / 3, c = lane - 3 * r;
    s.h = tile[r * row + MT_W * ld + (one ? 0 : c)];
  }
  return s;
}

// planes: [3][MT_TP] of one tensor in LDS.  A 1-channel pass fills all three planes with channel 0 (tf.multiply broadcasting, Training.py:422-426).
__device__ __forceinline__ void stage_put(float* planes, bool one, int r, int px, int c, float v) {
  const int o = r * MT_PW + px;
  if (one) {
    if (c == 0) planes[o] = planes[MT_TP + o] = planes[2 * MT_TP + o] = v;
  } else if (c < 3) {
    planes[c * MT_TP + o] = v;
  }
}
__device__ __forceinline__ void stage_commit(const Staged& s, float* planes, int ld, bool one, int nrows, bool halo, int lane) {
  const int nv = 4 * ld, items = nrows * nv;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int it = lane + 64 * j;
    if (it >= items) continue;
    const int r = ld == 4 ? it >> 4 : it / 12, v = it - r * nv;
    const float4 q = j ? s.q1 : s.q0;
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = 4 * v + k, px = ld == 4 ? v : idx / 3, c = ld == 4 ? k : idx - 3 * px;
      stage_put(planes, one, r, px, c, e[k]);
    }
  }
  if (halo && lane < nrows * 3) {
    const int r = lane / 3, c = lane - 3 * r;
    if (one) { if (c == 0) stage_put(planes, true, r, MT_W, 0, s.h); }
    else stage_put(planes, false, r, MT_W, c, s.h);
  }
}
// Rows that cannot be read as float4s (a clipped tile, an odd width, an unusual pixel stride): element by element, nothing read outside the image.
__device__ __forceinline__ void stage_scalar(const float* tile, float* planes, int ld, bool one, int W, int nrows, int ncols, int lane) {
  const long row = (long)W * ld;
  for (int it = lane; it < nrows * MT_PW * 3; it += 64) {
    const int r = it / (MT_PW * 3), rem = it - r * (MT_PW * 3), px = rem / 3, c = rem - 3 * px;
    if (px < ncols) planes[c * MT_TP + r * MT_PW + px] = tile[r * row + px * ld + (one ? 0 : c)];
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

}  // namespace
