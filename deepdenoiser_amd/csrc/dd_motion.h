// Where a pixel was in the previous frame (include/dd_hip.h: dd_temporal_stabilize states the rule, dd_sequence_quality uses this header):
// the position along the motion pass, the offscreen test, the index of the first bilinear tap, the weights and whether the second tap of a
// row / the second row is another pixel or the clamped same one.  fp32, one rounding per operation: no fused multiply-add.
#pragma once
#include "dd_common.h"

constexpr unsigned DD_MOTION_OFFSCREEN = 1u, DD_MOTION_XSTEP = 2u, DD_MOTION_YSTEP = 4u;

struct dd_motion_position {
  int q00;           // pixel index y0 * W + x0 of the tap (y0, x0); the others are q00 + 1 (XSTEP), q00 + W (YSTEP) and both
  float fx, fy;      // weights of the taps at x0 + 1 and y0 + 1
  unsigned bits;     // DD_MOTION_*; offscreen: q00 = 0, fx = fy = 0 and no step
};

// pixel (x, y) of an H x W frame, H * W <= INT_MAX; motion: [H,W,motion_ld], channels 0 and 1 used
__device__ __forceinline__ dd_motion_position dd_motion_previous(const float* __restrict__ motion, int motion_ld, float sx, float sy, int x, int y, int H,
                                                                 int W) {
#pragma clang fp contract(off)
  dd_motion_position r;
  r.q00 = 0; r.fx = r.fy = 0.f; r.bits = DD_MOTION_OFFSCREEN;
  const float* __restrict__ mv = motion + ((long)y * W + x) * motion_ld;
  const float px = (float)x + sx * mv[0], py = (float)y + sy * mv[1];
  if (!(px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1))) return r;      // (NaN and both infinities fail a comparison)
  const float xf = floorf(px), yf = floorf(py);
  const int ix = min(max((int)xf, 0), W - 1), iy = min(max((int)yf, 0), H - 1);
  r.fx = px - xf; r.fy = py - yf;
  r.q00 = iy * W + ix;
  r.bits = (ix + 1 <= W - 1 ? DD_MOTION_XSTEP : 0u) | (iy + 1 <= H - 1 ? DD_MOTION_YSTEP : 0u);
  return r;
}
