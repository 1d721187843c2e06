// Dynamic loss scaling on the device (include/dd_hip.h, dd_scaler_state): the scale, the skip decision of a step whose gradients overflowed
// and the Adam step counter live in ONE small record of device memory, so an optimisation step needs no host round trip:
//   dd_grads_nonfinite   one streaming pass over the flat gradient arena -> st->found_nonfinite
//   dd_adam_step_scaled  the TF-form update of adam_kernel (csrc/dd_pointwise.hip); writes nothing when the flag is set, divides by st->scale,
//                        derives lr_t from st->adam_t
//   dd_scaler_update     one thread: backoff / growth of the scale, the counters, clears the flag
// launched in this order on one stream.  The loss launches read st->scale through their *_dscale entries (csrc/dd_common.h, dd_grad_scale).
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

// inf or NaN <=> all eight exponent bits set.  A test on the bits: `x != x` / isfinite() are what a fast-math build may fold away.
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// 16-byte loads, grid-stride; the n % 4 last elements are taken one each by the first threads of workgroup 0.  A wave that saw a non-finite
// value issues ONE atomicOr (lane 0, after a ballot); a wave that saw none -- every wave of a healthy step -- writes nothing.
__global__ __launch_bounds__(256) void grads_nonfinite_kernel(const float* __restrict__ g, long n, dd_scaler_state* __restrict__ st) {
  const uint4* gv = reinterpret_cast<const uint4*>(g);
  const long nvec = n >> 2;
  const long tid = blockIdx.x * 256L + threadIdx.x;
  unsigned bad = 0u;
  for (long v = tid; v < nvec; v += (long)gridDim.x * 256L) {
    const uint4 q = gv[v];
    bad |= nonfinite_bits(q.x) | nonfinite_bits(q.y) | nonfinite_bits(q.z) | nonfinite_bits(q.w);
  }
  const long t = (nvec << 2) + tid;
  if (tid < 4 && t < n) bad |= nonfinite_bits(__float_as_uint(g[t]));
  // (every lane of the wave is back here: the ballot sees all 64)
  if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&st->found_nonfinite, 1);
}

// b^t for an integer t >= 0 by repeated squaring (doubles; at most 31 rounds)
__device__ __forceinline__ double powi(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

// adam_kernel's update, element for element, behind the device-side skip decision.  lr_t of step t = adam_t + 1 (the counter advances in
// dd_scaler_update, after this launch) is derived in double by ONE thread of the workgroup and shared through LDS.
__global__ __launch_bounds__(256) void adam_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          long n, double lr, double beta1, double beta2, float eps, float gs_host,
                                                          const dd_scaler_state* __restrict__ st) {
  __shared__ float lr_t_s;
  if (st->found_nonfinite != 0) return;      // uniform over the grid: nothing is written on a skipped step
  if (threadIdx.x == 0) {
    const int t = st->adam_t + 1;
    lr_t_s = (float)(lr * sqrt(1.0 - powi(beta2, t)) / (1.0 - powi(beta1, t)));
  }
  __syncthreads();
  const float lr_t = lr_t_s, b1 = (float)beta1, b2 = (float)beta2;
  const float gs = gs_host / st->scale;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float gi = g[i] * gs;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

// one thread; plain vector loads and stores
__global__ __launch_bounds__(64) void scaler_update_kernel(dd_scaler_state* st, float growth, float backoff, int growth_interval, float min_scale,
                                                           float max_scale) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float scale = st->scale;
  int good = st->good_steps;
  if (st->found_nonfinite != 0) {
    scale = fmaxf(scale * backoff, min_scale);
    good = 0;
    st->skipped_total = st->skipped_total + 1;
  } else {
    st->adam_t = st->adam_t + 1;
    if (++good == growth_interval) {
      scale = fminf(scale * growth, max_scale);
      good = 0;
    }
  }
  st->scale = scale;
  st->good_steps = good;
  st->found_nonfinite = 0;
}

}  // namespace

extern "C" int dd_grads_nonfinite(const float* grads, long n, dd_scaler_state* st, dd_stream stream) {
  DD_REQUIRE(grads && st && n > 0, "dd_grads_nonfinite: bad arguments");
  DD_REQUIRE(((uintptr_t)grads & 15) == 0, "dd_grads_nonfinite: grads must be 16-byte aligned");
  const long want = ((n >> 2) + 255) / 256;      // (the grid cap of adam_kernel)
  hipLaunchKernelGGL(grads_nonfinite_kernel, dim3((unsigned)(want < 1 ? 1 : (want < 2048 ? want : 2048))), dim3(256), 0, S(stream), grads, n, st);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" int dd_adam_step_scaled(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1, double beta2,
                                   float eps, float grad_scale, const dd_scaler_state* st, dd_stream stream) {
  DD_REQUIRE(params && grads && m && v && st && n > 0, "dd_adam_step_scaled: bad arguments");
  DD_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "dd_adam_step_scaled: beta1 and beta2 must be in [0, 1)");
  const long want = (n + 255) / 256;
  hipLaunchKernelGGL(adam_scaled_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, S(stream), params, grads, m, v, n, lr, beta1, beta2,
                     eps, grad_scale, st);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" int dd_scaler_update(dd_scaler_state* st, float growth, float backoff, int growth_interval, float min_scale, float max_scale,
                                dd_stream stream) {
  DD_REQUIRE(st != nullptr, "dd_scaler_update: null state");
  DD_REQUIRE(growth >= 1.f && backoff > 0.f && backoff <= 1.f && growth_interval > 0 && min_scale > 0.f && max_scale >= min_scale,
             "dd_scaler_update: need growth >= 1, 0 < backoff <= 1, growth_interval > 0, 0 < min_scale <= max_scale");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, S(stream), st, growth, backoff, growth_interval, min_scale, max_scale);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
