// Gradient clipping by global norm with per-variable norms (include/dd_hip.h, dd_grad_norms; replaces tf.clip_by_global_norm): one segmented
// reduction over the flat gradient arena and, at the same indices, the value arena.
//   grad_norm_chunks_kernel   one workgroup per chunk of the host's table (<= 4096 elements of ONE variable, no padding word): sum g^2, sum w^2 in
//                             double, the count of inf / NaN gradient elements -> one partial record per chunk
//   grad_norm_finish_kernel   one workgroup: every variable from its chunks in chunk order, the totals in variable order, the clip record
//   adam_clipped_kernel / adam_scaled_clipped_kernel   adam_kernel (csrc/dd_pointwise.hip) / adam_scaled_kernel (csrc/dd_loss_scale.hip) with the
//                             gradient g * gs * clip->coef
// Every sum is taken in an order fixed by the chunk table alone and nothing is accumulated with atomics: the same arena gives the same bytes
// on every run and on every rank of a data-parallel job, which therefore needs no collective to agree on the coefficient.  About 14 MB read
// for the flagship configuration: HBM / launch bound.
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

struct Partial { double grad_sq, weight_sq; unsigned nonfinite, reserved; };
static_assert(sizeof(Partial) == DD_GRAD_PARTIAL_BYTES, "dd_hip.h: DD_GRAD_PARTIAL_BYTES");
static_assert(sizeof(dd_grad_chunk) == 16 && sizeof(dd_grad_var_norms) == 24 && sizeof(dd_grad_clip) == 20, "dd_hip.h: gradient norm records");

// inf or NaN <=> all eight exponent bits set (the bit test of csrc/dd_loss_scale.hip: `x != x` is what a fast-math build may fold away)
__device__ __forceinline__ unsigned nonfinite_bits(unsigned u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// squares and sums in double: 3.4e38^2 = 1.2e77 is far inside the range; a non-finite gradient element counts and adds nothing
__device__ __forceinline__ void take(unsigned gu, unsigned wu, double& gs, double& ws, unsigned& nf) {
  const unsigned bad = nonfinite_bits(gu);
  const double g = bad ? 0.0 : (double)__uint_as_float(gu), w = (double)__uint_as_float(wu);
  gs += g * g;
  ws += w * w;
  nf += bad;
}

// 256 threads, <= 4 x 16 bytes of each arena per thread.  The elements in front of the first 16-byte boundary and behind the last one (none
// for a ParamStore, whose variables start 16-byte aligned) are taken one each by the first threads.  Wave: a shuffle-down tree (lane l adds lane
// l + 32, then l + 16, ...: a fixed order); workgroup: thread 0 adds the four waves' sums in wave order.
__global__ __launch_bounds__(256) void grad_norm_chunks_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                               const dd_grad_chunk* __restrict__ chunks, Partial* __restrict__ partials) {
  __shared__ double s_gs[4], s_ws[4];
  __shared__ unsigned s_nf[4];
  const dd_grad_chunk c = chunks[blockIdx.x];
  const float* gp = g + c.offset;
  const float* wp = w + c.offset;
  const int len = c.length, t = threadIdx.x;
  int head = (int)((4 - (c.offset & 3)) & 3);
  if (head > len) head = len;
  const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
  const uint4* gv = reinterpret_cast<const uint4*>(gp + head);
  const uint4* wv = reinterpret_cast<const uint4*>(wp + head);
  double gs = 0.0, ws = 0.0;
  unsigned nf = 0u;
  for (int v = t; v < nvec; v += 256) {
    const uint4 a = gv[v], b = wv[v];
    take(a.x, b.x, gs, ws, nf);
    take(a.y, b.y, gs, ws, nf);
    take(a.z, b.z, gs, ws, nf);
    take(a.w, b.w, gs, ws, nf);
  }
  if (t < head) take(__float_as_uint(gp[t]), __float_as_uint(wp[t]), gs, ws, nf);
  if (t < len - tail0) take(__float_as_uint(gp[tail0 + t]), __float_as_uint(wp[tail0 + t]), gs, ws, nf);
  for (int off = 32; off > 0; off >>= 1) {
    gs += __shfl_down(gs, off);
    ws += __shfl_down(ws, off);
    nf += __shfl_down(nf, off);
  }
  if ((t & 63) == 0) { s_gs[t >> 6] = gs; s_ws[t >> 6] = ws; s_nf[t >> 6] = nf; }
  __syncthreads();
  if (t == 0) {
    Partial p;
    p.grad_sq = ((s_gs[0] + s_gs[1]) + s_gs[2]) + s_gs[3];
    p.weight_sq = ((s_ws[0] + s_ws[1]) + s_ws[2]) + s_ws[3];
    p.nonfinite = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
    p.reserved = 0u;
    partials[blockIdx.x] = p;
  }
}

// Thread t owns the variables [t * per, (t + 1) * per), per = ceil(n_vars / 256): any number of variables.  A variable's partial records are
// added in chunk order (loaded eight at a time so that the loads are in flight together: a 3 x 3 x 384 x 384 kernel has 324 of them; the
// records past the variable's last chunk are replaced by zeros, which change no sum of squares).  Thread 0 then adds the threads' totals in
// thread order == variable order.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const Partial* __restrict__ partials, const int* __restrict__ var_first, int n_vars,
                                                               dd_grad_var_norms* __restrict__ var_norms, dd_grad_clip* __restrict__ clip,
                                                               float clip_norm, float gs_host, const dd_scaler_state* __restrict__ st) {
  __shared__ double s_gs[256];
  __shared__ unsigned s_nf[256], s_nv[256];
  const int t = threadIdx.x, per = (n_vars + 255) / 256;
  double tg = 0.0;
  unsigned tnf = 0u, tnv = 0u;
  for (int k = 0; k < per; ++k) {
    const int v = t * per + k;
    if (v >= n_vars) break;
    const int lo = var_first[v], hi = var_first[v + 1];
    double a = 0.0, b = 0.0;
    unsigned cnt = 0u;
    for (int i = lo; i < hi; i += 8) {
      Partial p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = partials[i + j < hi ? i + j : lo];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = i + j < hi;
        a += in ? p[j].grad_sq : 0.0;
        b += in ? p[j].weight_sq : 0.0;
        cnt += in ? p[j].nonfinite : 0u;
      }
    }
    dd_grad_var_norms r;
    r.grad_sq = a; r.weight_sq = b; r.nonfinite = cnt; r.reserved = 0u;
    var_norms[v] = r;
    tg += a;
    tnf += cnt;
    tnv += cnt != 0u ? 1u : 0u;
  }
  s_gs[t] = tg; s_nf[t] = tnf; s_nv[t] = tnv;
  __syncthreads();
  if (t != 0) return;
  double total = 0.0;
  unsigned nf = 0u, nv = 0u;
  for (int i = 0; i < 256; ++i) { total += s_gs[i]; nf += s_nf[i]; nv += s_nv[i]; }
  const float gs = st ? gs_host / st->scale : gs_host;      // (the expression of adam_scaled_kernel)
  const double norm = fabs((double)gs) * sqrt(total);
  dd_grad_clip r;
  r.grad_factor = gs;
  r.nonfinite_variables = nv;
  r.nonfinite_total = nf;
  r.coef = 1.f;
  if (nf != 0u) {
    r.grad_norm = __uint_as_float(0x7f800000u);      // the step is the scaler's (or the static fp16 check's) to skip: nothing is clipped
  } else {
    r.grad_norm = (float)norm;
    if (clip_norm > 0.f) r.coef = (float)((double)clip_norm / fmax(norm, (double)clip_norm));      // tf.clip_by_global_norm
  }
  *clip = r;
}

// adam_kernel (csrc/dd_pointwise.hip) with one more factor; coef == 1: (g * gs) * 1 is g * gs, bit for bit
__global__ void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    long n, float lr_t, float b1, float b2, float eps, float gs, const dd_grad_clip* __restrict__ clip) {
  const float coef = clip->coef;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float gi = g[i] * gs * coef;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

// b^t for an integer t >= 0 by repeated squaring (doubles; at most 31 rounds)
__device__ __forceinline__ double powi(double b, int t) {
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

// adam_scaled_kernel (csrc/dd_loss_scale.hip) with one more factor: the same skip, the same lr_t, the same gs
__global__ __launch_bounds__(256) void adam_scaled_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, long n, double lr, double beta1, double beta2, float eps,
                                                                  float gs_host, const dd_scaler_state* __restrict__ st,
                                                                  const dd_grad_clip* __restrict__ clip) {
  __shared__ float lr_t_s;
  if (st->found_nonfinite != 0) return;      // uniform over the grid: nothing is written on a skipped step
  if (threadIdx.x == 0) {
    const int t = st->adam_t + 1;
    lr_t_s = (float)(lr * sqrt(1.0 - powi(beta2, t)) / (1.0 - powi(beta1, t)));
  }
  __syncthreads();
  const float lr_t = lr_t_s, b1 = (float)beta1, b2 = (float)beta2;
  const float gs = gs_host / st->scale, coef = clip->coef;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float gi = g[i] * gs * coef;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    p[i] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

}  // namespace

extern "C" int dd_grad_norms(const float* grads, const float* values, const dd_grad_chunk* chunks, int n_chunks, const int* var_first, int n_vars,
                             void* partials, dd_grad_var_norms* var_norms, dd_grad_clip* clip, float clip_norm, float grad_scale,
                             const dd_scaler_state* st, dd_stream stream) {
  DD_REQUIRE(grads && values && chunks && var_first && partials && var_norms && clip, "dd_grad_norms: null argument");
  DD_REQUIRE(n_chunks > 0 && n_vars > 0 && n_vars <= n_chunks, "dd_grad_norms: need 0 < n_vars <= n_chunks");
  DD_REQUIRE((((uintptr_t)grads | (uintptr_t)values) & 15) == 0, "dd_grad_norms: grads and values must be 16-byte aligned");
  DD_REQUIRE(clip_norm == clip_norm && clip_norm < __builtin_huge_valf(), "dd_grad_norms: clip_norm must be finite (<= 0: measure only)");
  hipLaunchKernelGGL(grad_norm_chunks_kernel, dim3((unsigned)n_chunks), dim3(256), 0, S(stream), grads, values, chunks,
                     reinterpret_cast<Partial*>(partials));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, S(stream), reinterpret_cast<const Partial*>(partials), var_first, n_vars,
                     var_norms, clip, clip_norm, grad_scale, st);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" int dd_adam_step_clipped(float* params, const float* grads, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                                    float eps, float grad_scale, const dd_grad_clip* clip, dd_stream stream) {
  DD_REQUIRE(params && grads && m && v && clip && n > 0, "dd_adam_step_clipped: bad arguments");
  const long want = (n + 255) / 256;      // (the grid of dd_adam_step)
  hipLaunchKernelGGL(adam_clipped_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, S(stream), params, grads, m, v, n, lr_t, beta1,
                     beta2, eps, grad_scale, clip);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" int dd_adam_step_scaled_clipped(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1, double beta2,
                                           float eps, float grad_scale, const dd_scaler_state* st, const dd_grad_clip* clip, dd_stream stream) {
  DD_REQUIRE(params && grads && m && v && st && clip && n > 0, "dd_adam_step_scaled_clipped: bad arguments");
  DD_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "dd_adam_step_scaled_clipped: beta1 and beta2 must be in [0, 1)");
  const long want = (n + 255) / 256;
  hipLaunchKernelGGL(adam_scaled_clipped_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, S(stream), params, grads, m, v, n, lr,
                     beta1, beta2, eps, grad_scale, st, clip);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
