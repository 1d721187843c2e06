// Device helpers shared by the loss kernels (csrc/dd_pointwise.hip), the tracked-metric kernel (csrc/dd_metrics.hip) and the preview kernel
// (csrc/dd_preview.hip): the per-element LossDifference term and the value of a loss "source" (feature, combined feature, combined image) at a
// pixel.
#pragma once
#include "dd_common.h"

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
// loss term and its derivative with respect to the prediction
__device__ __forceinline__ void loss_term(int kind, float eps, float p, float t, float* l, float* dl) {
  const float d = p - t;
  switch (kind) {
    case 1: *l = d; *dl = 1.f; break;
    case 2: *l = fabsf(d); *dl = sgn(d); break;
    case 3: { const float a = fabsf(d); if (a < 1.f) { *l = 0.5f * a * a; *dl = d; } else { *l = a - 0.5f; *dl = sgn(d); } break; }
    case 4: *l = d * d; *dl = 2.f * d; break;
    default: {
      const float a = fabsf(d), den = fabsf(p) + fabsf(t) + eps;
      *l = a / den;
      *dl = sgn(d) / den - a * sgn(p) / (den * den);
    }
  }
}

// Value of one loss "source" at a pixel, 3 channels (1-channel passes broadcast, tf.multiply broadcasting, Training.py:422-426), on NS SIDES
// at once.  A side is a set of tensors the features are read from: the predictions (d.pred / d.pred_ld), the targets (d.target /
// d.target_ld), or any other per-feature pointer table with the descriptor's channel counts (the raw passes of dd_loss_previews).
struct LossSide { const float* const* base; const int* ld; };
template <int NS> struct SideVal { float s[NS][3]; };
__device__ __forceinline__ LossSide pred_side(const dd_loss_desc& d) { return {d.pred, d.pred_ld}; }
__device__ __forceinline__ LossSide target_side(const dd_loss_desc& d) { return {d.target, d.target_ld}; }
template <int NS>
__device__ __forceinline__ SideVal<NS> feature_sides(const dd_loss_desc& d, const LossSide (&sd)[NS], int f, long i) {
  SideVal<NS> v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cf = d.nch[f] == 1 ? 0 : c;
#pragma unroll
    for (int k = 0; k < NS; ++k) v.s[k][c] = sd[k].base[f][i * sd[k].ld[f] + cf];
  }
  return v;
}
template <int NS>
__device__ __forceinline__ SideVal<NS> combined_sides(const dd_loss_desc& d, const LossSide (&sd)[NS], int k, long i) {      // color * (direct + indirect)
#pragma clang fp contract(off)      // one rounding per operation wherever a source value is formed (loss_head_kernel / loss_general_kernel)
  const SideVal<NS> c = feature_sides<NS>(d, sd, d.comb[k][0], i), dr = feature_sides<NS>(d, sd, d.comb[k][1], i), in = feature_sides<NS>(d, sd, d.comb[k][2], i);
  SideVal<NS> v;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int q = 0; q < NS; ++q) v.s[q][ch] = c.s[q][ch] * (dr.s[q][ch] + in.s[q][ch]);
  }
  return v;
}
template <int NS>
__device__ __forceinline__ SideVal<NS> image_sides(const dd_loss_desc& d, const LossSide (&sd)[NS], long i) {      // sum of the combined features and single passes
#pragma clang fp contract(off)
  SideVal<NS> v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int q = 0; q < NS; ++q) v.s[q][c] = 0.f;
  }
  for (int j = 0; j < d.n_image_combined; ++j) {
    const SideVal<NS> a = combined_sides<NS>(d, sd, d.image_combined[j], i);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int q = 0; q < NS; ++q) v.s[q][c] += a.s[q][c];
    }
  }
  for (int j = 0; j < d.n_image_features; ++j) {
    const SideVal<NS> a = feature_sides<NS>(d, sd, d.image_features[j], i);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int q = 0; q < NS; ++q) v.s[q][c] += a.s[q][c];
    }
  }
  return v;
}

// the two sides of the loss: prediction and target
struct Val3 { float p[3], t[3]; };
__device__ __forceinline__ Val3 val3_of(const SideVal<2>& a) {
  Val3 v;
#pragma unroll
  for (int c = 0; c < 3; ++c) { v.p[c] = a.s[0][c]; v.t[c] = a.s[1][c]; }
  return v;
}
__device__ __forceinline__ Val3 feature_value(const dd_loss_desc& d, int f, long i) {
  const LossSide sd[2] = {pred_side(d), target_side(d)};
  return val3_of(feature_sides<2>(d, sd, f, i));
}
__device__ __forceinline__ Val3 combined_value(const dd_loss_desc& d, int k, long i) {
  const LossSide sd[2] = {pred_side(d), target_side(d)};
  return val3_of(combined_sides<2>(d, sd, k, i));
}
__device__ __forceinline__ Val3 image_value(const dd_loss_desc& d, long i) {
  const LossSide sd[2] = {pred_side(d), target_side(d)};
  return val3_of(image_sides<2>(d, sd, i));
}

// Conv2dUtilities.non_zero_mask (Conv2dUtilities.py:69-74) of feature f's target at pixel i: sign(sum_c |t_c|)
__device__ __forceinline__ float target_mask(const dd_loss_desc& d, int f, long i) {
  float s = 0.f;
  for (int c = 0; c < d.nch[f]; ++c) s += fabsf(d.target[f][i * d.target_ld[f] + c]);
  return s > 0.f ? 1.f : 0.f;
}
