// Device helpers shared by the loss kernels (csrc/dd_pointwise.hip) and the tracked-metric kernel (csrc/dd_metrics.hip): the per-element
// LossDifference term and the value of a loss "source" (feature, combined feature, combined image) at a pixel.
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

// Value of one loss "source" at a pixel: prediction and target, 3 channels (1-channel passes broadcast, tf.multiply broadcasting,
// Training.py:422-426).
struct Val3 { float p[3], t[3]; };
__device__ __forceinline__ Val3 feature_value(const dd_loss_desc& d, int f, long i) {
  Val3 v;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cf = d.nch[f] == 1 ? 0 : c;
    v.p[c] = d.pred[f][i * d.pred_ld[f] + cf];
    v.t[c] = d.target[f][i * d.target_ld[f] + cf];
  }
  return v;
}
__device__ __forceinline__ Val3 combined_value(const dd_loss_desc& d, int k, long i) {      // color * (direct + indirect)
#pragma clang fp contract(off)      // one rounding per operation wherever a source value is formed (loss_head_kernel / loss_general_kernel)
  const Val3 c = feature_value(d, d.comb[k][0], i), dr = feature_value(d, d.comb[k][1], i), in = feature_value(d, d.comb[k][2], i);
  Val3 v;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) { v.p[ch] = c.p[ch] * (dr.p[ch] + in.p[ch]); v.t[ch] = c.t[ch] * (dr.t[ch] + in.t[ch]); }
  return v;
}
__device__ __forceinline__ Val3 image_value(const dd_loss_desc& d, long i) {                 // sum of the combined features and single passes
#pragma clang fp contract(off)
  Val3 v = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (int j = 0; j < d.n_image_combined; ++j) {
    const Val3 a = combined_value(d, d.image_combined[j], i);
#pragma unroll
    for (int c = 0; c < 3; ++c) { v.p[c] += a.p[c]; v.t[c] += a.t[c]; }
  }
  for (int j = 0; j < d.n_image_features; ++j) {
    const Val3 a = feature_value(d, d.image_features[j], i);
#pragma unroll
    for (int c = 0; c < 3; ++c) { v.p[c] += a.p[c]; v.t[c] += a.t[c]; }
  }
  return v;
}

// Conv2dUtilities.non_zero_mask (Conv2dUtilities.py:69-74) of feature f's target at pixel i: sign(sum_c |t_c|)
__device__ __forceinline__ float target_mask(const dd_loss_desc& d, int f, long i) {
  float s = 0.f;
  for (int c = 0; c < d.nch[f]; ++c) s += fabsf(d.target[f][i * d.target_ld[f] + c]);
  return s > 0.f ? 1.f : 0.f;
}
