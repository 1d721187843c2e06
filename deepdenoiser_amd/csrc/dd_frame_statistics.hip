// Data-set statistics of frames that stay in device memory (include/dd_hip.h, dd_stat_desc): ONE launch reduces every (window, pass) of a table
// of T x T windows to a row of DD_STAT_FIELDS doubles -- minimum, maximum, shifted sums and coverage count, raw and in signed-log1p space,
// and the sums weighted by the non-black mask of a target colour pass (TFRecordsStatistics.py:236-316, both sweeps in one read).
//
// Shape.  grid = (window, pass), one workgroup of kThreads threads per row of the table.  A thread owns PIXELS t, t + kThreads, ... of the
// window in row-major order: consecutive lanes read consecutive pixels of a frame row (T * C contiguous floats per row), and the per-pixel
// quantities -- the coverage test sum_c |x_c| != 0 and the mask sign(sum_c |mask_c|) -- need no exchange between lanes; the mask window is
// read once.  Everything is accumulated in double; log1p is the double one.
//
// Order of the sums (fixed, no atomics: two launches give the same bytes): a thread adds its pixels in ascending order, channels 0 .. C-1
// inside a pixel; the 64 partial results of a wave are combined by a shift-down tree (lane i += lane i + 32, 16, 8, 4, 2, 1); lane 0 of
// every wave leaves its result in LDS and thread 0 adds the waves in wave order.  Plain C++: no inline assembly, no scratch.
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSums = 8;        // sum(x-K), sum(x-K)^2, sum(l-Kl), sum(l-Kl)^2, and the same four weighted by the mask

__device__ __forceinline__ double signed_log1p(double x) { return copysign(log1p(fabs(x)), x); }      // Utilities.signed_log1p (sign(0) = 0: log1p(0) = 0)

// ---- signed_log1p of a row's minimum and maximum, correctly rounded.  signed_log1p is monotone, so min l = signed_log1p(min x) and
// max l = signed_log1p(max x): the two values a row reports are computed once, by one thread, in double-double arithmetic (a value as an
// unevaluated sum hi + lo of two doubles, ~106 bits; the error-free transformations of Dekker and Knuth).  The library log1p the sums use is
// within an ulp of the true value but not always the nearest double (it missed the 0.505-ulp cases of the op-level test's data), and a
// minimum that is one ulp off is a different number in the file.
struct dd { double hi, lo; };
// (no contraction in here: a product fused into one of these sums but rounded in the next breaks the identities; the explicit fma stays fused)
#define DD_EXACT _Pragma("clang fp contract(off)")
__device__ __forceinline__ dd quick_two_sum(double a, double b) { DD_EXACT const double s = a + b; return {s, b - (s - a)}; }      // |a| >= |b|
__device__ __forceinline__ dd two_sum(double a, double b) {
  DD_EXACT
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y) {
  DD_EXACT
  const dd s = two_sum(x.hi, y.hi);
  return quick_two_sum(s.hi, s.lo + (x.lo + y.lo));
}
__device__ __forceinline__ dd dd_mul(dd x, dd y) {
  DD_EXACT
  const double p = x.hi * y.hi, e = fma(x.hi, y.hi, -p);
  return quick_two_sum(p, e + (x.hi * y.lo + x.lo * y.hi));
}
__device__ __forceinline__ dd dd_div(dd x, dd y) {
  DD_EXACT
  const double q1 = x.hi / y.hi;
  dd r = dd_add(x, dd_mul(y, {-q1, 0.0}));
  const double q2 = r.hi / y.hi;
  r = dd_add(r, dd_mul(y, {-q2, 0.0}));
  const double q3 = r.hi / y.hi;
  return dd_add(quick_two_sum(q1, q2), {q3, 0.0});
}
// log1p(u) for a finite u >= 0: w = 1 + u exactly (two_sum), w = 2^k m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s) with
// s = (m - 1) / (m + 1), |s| <= 0.172: sixteen terms of 2 s (1 + s^2 / 3 + s^4 / 5 + ...) leave less than 2^-80 of the result
__device__ double log1p_nearest(double u) {
  DD_EXACT
  if (u == 0.0) return 0.0;
  const dd w = two_sum(1.0, u);
  int k;
  double m = frexp(w.hi, &k);
  if (m < 0.70710678118654752) k -= 1;
  const dd mm = {ldexp(w.hi, -k), ldexp(w.lo, -k)};
  const dd s = dd_div(dd_add(mm, {-1.0, 0.0}), dd_add(mm, {1.0, 0.0}));
  const dd s2 = dd_mul(s, s);
  dd p = {0.0, 0.0};
#pragma nounroll
  for (int n = 16; n >= 1; --n) {
    const double d = 2.0 * n + 1.0, c = 1.0 / d;
    p = dd_mul(s2, dd_add(p, {c, fma(-d, c, 1.0) / d}));       // (p + 1 / (2 n + 1)) s^2
  }
  dd r = dd_mul({2.0 * s.hi, 2.0 * s.lo}, dd_add(p, {1.0, 0.0}));
  r = dd_add(dd_mul({(double)k, 0.0}, {0.69314718055994530942, 2.3190468138462996e-17}), r);
  return r.hi;
}
__device__ __forceinline__ double signed_log1p_nearest(double x) { return copysign(log1p_nearest(fabs(x)), x); }

struct Acc {
  double mn, mx;
  double s[kSums];
  int count, mask_sum;
};

__device__ __forceinline__ void combine(Acc& a, const Acc& b) {
  a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx);
#pragma unroll
  for (int k = 0; k < kSums; ++k) a.s[k] += b.s[k];
  a.count += b.count; a.mask_sum += b.mask_sum;
}

__device__ __forceinline__ Acc shifted_down(const Acc& a, int delta) {
  Acc b;
  b.mn = __shfl_down(a.mn, delta); b.mx = __shfl_down(a.mx, delta);
#pragma unroll
  for (int k = 0; k < kSums; ++k) b.s[k] = __shfl_down(a.s[k], delta);
  b.count = __shfl_down(a.count, delta); b.mask_sum = __shfl_down(a.mask_sum, delta);
  return b;
}

template <int C>
__device__ __forceinline__ void accumulate_window(Acc& a, const float* __restrict__ win, long row_floats, const float* __restrict__ mask,
                                                  long mask_row_floats, int T, bool is_alpha, double K, double Kl) {
  const int pixels = T * T;
  for (int i = threadIdx.x; i < pixels; i += kThreads) {
    const int y = i / T, x = i - y * T;
    const float* p = win + (long)y * row_floats + (long)x * C;
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
    double m = 0.0;
    if (mask != nullptr) {                              // (C == 3: the launcher refuses a mask on a 1-channel pass)
      const float* q = mask + (long)y * mask_row_floats + (long)x * 3;
      m = (q[0] != 0.f || q[1] != 0.f || q[2] != 0.f) ? 1.0 : 0.0;      // Conv2dUtilities.non_zero_mask: sign(sum_c |mask_c|), a sum of
                                                                        // non-negative terms: not zero exactly when one of them is not
      a.mask_sum += (int)m;
    }
    bool cover = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      cover = cover || (is_alpha ? v[c] != 1.f : v[c] != 0.f);      // TFRecordsStatistics.py:262-264, 277-280 (x - 1 != 0 exactly when x != 1)
      const double xd = (double)v[c], l = signed_log1p(xd);
      a.mn = fmin(a.mn, xd); a.mx = fmax(a.mx, xd);
      const double d = xd - K, dl = l - Kl;
      a.s[0] += d; a.s[1] += d * d; a.s[2] += dl; a.s[3] += dl * dl;
      a.s[4] += m * d; a.s[5] += m * (d * d); a.s[6] += m * dl; a.s[7] += m * (dl * dl);
    }
    a.count += cover ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void frame_statistics_kernel(const dd_stat_desc desc, const dd_stat_window* __restrict__ windows, int T,
                                                                    double* __restrict__ out) {
  __shared__ Acc partial[kWaves];
  const dd_stat_pass& p = desc.pass[blockIdx.y];
  const dd_stat_window& r = windows[blockIdx.x];
  double* row = out + ((long)blockIdx.x * desc.n_passes + blockIdx.y) * DD_STAT_FIELDS;
  // a window cannot be checked on the host (the table lives in device memory): plane and origin are clamped, so no read leaves a plane
  const int plane = min(max(r.plane, 0), desc.n_planes - 1);
  const int h = desc.plane_hw[2 * plane], w = desc.plane_hw[2 * plane + 1];
  const float* __restrict__ frame = p.planes[plane];
  if (frame == nullptr || h < T || w < T) {             // (uniform over the workgroup: before any barrier) the row is marked absent
    if (threadIdx.x < DD_STAT_FIELDS) row[threadIdx.x] = 0.0;
    return;
  }
  const int y0 = min(max(r.y0, 0), h - T), x0 = min(max(r.x0, 0), w - T);
  const int C = p.C;
  const long row_floats = (long)w * C;
  const float* win = frame + ((long)y0 * w + x0) * C;
  // the mask window: the same origin in the mask plane, clamped by THAT plane's size
  const float* mask = nullptr;
  long mask_row_floats = 0;
  if (p.mask_planes != nullptr) {
    const int mp = min(max(r.mask_plane, 0), desc.n_planes - 1);
    const int mh = desc.plane_hw[2 * mp], mw = desc.plane_hw[2 * mp + 1];
    const float* mframe = p.mask_planes[mp];
    if (mframe != nullptr && mh >= T && mw >= T) {
      const int my0 = min(max(r.y0, 0), mh - T), mx0 = min(max(r.x0, 0), mw - T);
      mask_row_floats = (long)mw * 3;
      mask = mframe + ((long)my0 * mw + mx0) * 3;
    }
  }
  const double K = (double)win[0], Kl = signed_log1p(K);
  Acc a;
  a.mn = INFINITY; a.mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < kSums; ++k) a.s[k] = 0.0;
  a.count = a.mask_sum = 0;
  if (C == 3) accumulate_window<3>(a, win, row_floats, mask, mask_row_floats, T, p.is_alpha != 0, K, Kl);
  else accumulate_window<1>(a, win, row_floats, nullptr, 0, T, p.is_alpha != 0, K, Kl);
  // the wave's tree: after the step with delta, lanes 0 .. delta-1 hold the sums of lanes i, i + delta, ...
  for (int delta = 32; delta >= 1; delta >>= 1) {
    const Acc b = shifted_down(a, delta);
    combine(a, b);
  }
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc t = partial[0];
    for (int wv = 1; wv < kWaves; ++wv) combine(t, partial[wv]);
    row[DD_STAT_PRESENT] = 1.0;
    row[DD_STAT_MIN] = t.mn; row[DD_STAT_MAX] = t.mx; 
    row[DD_STAT_MIN_LOG1P] = signed_log1p_nearest(t.mn); row[DD_STAT_MAX_LOG1P] = signed_log1p_nearest(t.mx);
    row[DD_STAT_PIVOT] = K; row[DD_STAT_PIVOT_LOG1P] = Kl;
    row[DD_STAT_SUM] = t.s[0]; row[DD_STAT_SUM_SQ] = t.s[1]; row[DD_STAT_SUM_LOG1P] = t.s[2]; row[DD_STAT_SUM_SQ_LOG1P] = t.s[3];
    row[DD_STAT_COUNT] = (double)t.count; row[DD_STAT_MASK_SUM] = (double)t.mask_sum;
    row[DD_STAT_MASKED_SUM] = t.s[4]; row[DD_STAT_MASKED_SUM_SQ] = t.s[5];
    row[DD_STAT_MASKED_SUM_LOG1P] = t.s[6]; row[DD_STAT_MASKED_SUM_SQ_LOG1P] = t.s[7];
  }
}

}  // namespace

extern "C" int dd_tile_statistics(const dd_stat_desc* desc, const dd_stat_window* windows, int n_windows, int T, double* out, dd_stream stream) {
  DD_REQUIRE(desc && windows && out, "dd_tile_statistics: null descriptor, window table or output");
  DD_REQUIRE(desc->n_passes >= 1 && desc->n_passes <= DD_STAT_MAX_PASSES, "dd_tile_statistics: n_passes=%d (1 .. %d passes fit the descriptor)",
             desc->n_passes, DD_STAT_MAX_PASSES);
  DD_REQUIRE(desc->plane_hw && desc->n_planes >= 1, "dd_tile_statistics: null plane size table or n_planes=%d", desc->n_planes);
  DD_REQUIRE(T >= 1 && T <= 16384, "dd_tile_statistics: T=%d (1 .. 16384)", T);
  DD_REQUIRE(n_windows >= 1, "dd_tile_statistics: n_windows=%d", n_windows);
  for (int i = 0; i < desc->n_passes; ++i) {
    const dd_stat_pass& p = desc->pass[i];
    DD_REQUIRE(p.planes, "dd_tile_statistics: pass %d has a null plane array", i);
    DD_REQUIRE(p.C == 1 || p.C == 3, "dd_tile_statistics: pass %d has C=%d (1 or 3)", i, p.C);
    DD_REQUIRE(!p.mask_planes || p.C == 3, "dd_tile_statistics: pass %d has a mask pass and C=%d: a mask needs 3 channels (TFRecordsStatistics.py:252)",
               i, p.C);
  }
  hipLaunchKernelGGL(frame_statistics_kernel, dim3(n_windows, desc->n_passes), dim3(kThreads), 0, S(stream), *desc, windows, T, out);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
