// TensorBoard histograms of the tracked differences (track_difference_histogram / track_variation_difference_histogram of the statistics
// sections of Training.json; BaseFeatureTraining.add_tracked_histograms, Training.py:267-281), binned where the values are
// (include/dd_hip.h: dd_histogram_values, dd_loss_histograms).
//
//   hist_add   : the binning core, one value per lane.  The bucket is upper_bound(limits, (double)v) on the limit table the host uploaded
//                (staged in LDS): a log2 first guess, then a comparison fix-up against the table, so the guess only costs time when it is off.
//                Counts are uint32 in LDS, private to the workgroup; lanes of the wave that hit the same bucket are folded into one LDS
//                atomic first (a tile of zeros is one add, not 64 serialised ones).  sum / sum_squares in double, min / max as
//                order-preserving integer keys of the fp32 value, all per lane.
//   values     : a workgroup walks a contiguous chunk of a flat buffer.
//   fused      : a workgroup owns ONE source and a chunk of the 16 x 4 tiles of the batch; each of its waves stages the tile it is at (the
//                features that source is made of, with the helpers of dd_metrics_stage.h) and adds the values of up to three kinds.
//                (All sources of a tile from one staging, as loss_metrics_kernel does, would need the private counts of every source at
//                once: 22 sources x 3 kinds x 6.2 KB is more than the 160 KB of a CU.)
//   both end   : non-zero buckets go to the record with one integer atomic each, once per workgroup; the statistics go to a per-workgroup
//                partial.
//   finalize   : one wave per record adds the partials in index order.
// Integer atomics only, no float order that depends on scheduling: two runs give the same bits.
#include "dd_common.h"
#include "dd_loss_common.h"
#include "dd_metrics_stage.h"

namespace {

constexpr int HV_MAX_WG = DD_HISTOGRAM_VALUES_SCRATCH_BYTES / 40;      // workgroups of a dd_histogram_values launch
constexpr int HC_MAX = DD_HISTOGRAM_MAX_CHUNKS;                        // tile chunks (workgroups per source) of a dd_loss_histograms launch
constexpr int H_KINDS = 3;
constexpr int H_SLOTS = DD_METRIC_SOURCES;

struct HistLane {      // what one lane has seen
  double sum, sq;
  unsigned kmin, kmax, num, bad;
};
struct HistPartial {   // what one workgroup has seen (40 bytes)
  double sum, sq;
  unsigned kmin, kmax;
  unsigned long long num, bad;
};
static_assert(sizeof(HistPartial) == 40, "partial layout");

__device__ __forceinline__ void hist_lane_init(HistLane& a) {
  a.sum = a.sq = 0.0;
  a.kmin = 0xffffffffu; a.kmax = 0u; a.num = a.bad = 0u;
}
// fp32 -> unsigned key with the same order (-0.0 below +0.0), and back
__device__ __forceinline__ unsigned hist_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float hist_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// upper_bound(lim[0 .. nb), (double)v) for a finite v: the first index whose limit is greater than v (Histogram::Add, histogram.cc).  The
// guess assumes TensorFlow's default table (zero in the middle, 1e-12 * 1.1^j outwards); the fix-up (a few comparisons next to the guess, else a binary search) makes
// the result exact for ANY increasing table whose last entry is above every fp32.
__device__ __forceinline__ int hist_bucket(const double* lim, int nb, float v) {
  const int zero = (nb - 1) >> 1;
  const float a = fabsf(v);
  int c = 0;      // about how many positive limits are <= |v|
  if (a >= 1e-12f) c = min(max((int)((__log2f(a) + 39.863137f) * 7.2725409f) + 1, 0), zero);      // log2(1e-12), 1 / log2(1.1)
  int idx = v >= 0.f ? zero + 1 + c : zero - c;
  idx = min(max(idx, 0), nb - 1);
  const double dv = (double)v;
  int steps = 0;      // the default table needs 0 - 2 of them; any other table falls through to the binary search
  while (idx > 0 && lim[idx - 1] > dv && steps < 4) { --idx; ++steps; }
  while (idx < nb - 1 && lim[idx] <= dv && steps < 8) { ++idx; ++steps; }
  if ((idx > 0 && lim[idx - 1] > dv) || (idx < nb - 1 && lim[idx] <= dv)) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lim[mid] <= dv) lo = mid + 1; else hi = mid;
    }
    idx = lo;
  }
  return idx;
}

// Adds the value of every active lane.  Called by ALL lanes of a wave (wave-uniform control flow around it).
__device__ __forceinline__ void hist_add(const double* lim, int nb, unsigned* counts, float v, bool active, int lane, HistLane& a) {
  if (active && !(fabsf(v) <= 3.4028234664e38f)) {      // NaN, +-inf: counted, nothing else
    ++a.bad;
    active = false;
  }
  int bin = -1;
  if (active) {
    bin = hist_bucket(lim, nb, v);
    const double dv = (double)v;
    a.sum += dv;
    a.sq += dv * dv;
    const unsigned k = hist_key(v);
    a.kmin = min(a.kmin, k);
    a.kmax = max(a.kmax, k);
    ++a.num;
  }
  // fold the lanes of the most common buckets (at most 4 rounds), the rest add on their own
  unsigned long long rem = __ballot(active);
#pragma unroll 1
  for (int round = 0; round < 4 && rem; ++round) {
    const int leader = __ffsll((long long)rem) - 1;
    const int b = __shfl(bin, leader);
    const unsigned long long same = __ballot(active && bin == b);
    if (lane == leader) atomicAdd(&counts[b], (unsigned)__popcll(same));
    if (bin == b) active = false;
    rem &= ~same;
  }
  if (active) atomicAdd(&counts[bin], 1u);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ HistPartial hist_wave_reduce(const HistLane& a) {
  HistPartial p;
  p.sum = wave_sum_f64(a.sum);
  p.sq = wave_sum_f64(a.sq);
  unsigned kmin = a.kmin, kmax = a.kmax, num = a.num, bad = a.bad;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    num += (unsigned)__shfl_xor((int)num, o);
    bad += (unsigned)__shfl_xor((int)bad, o);
  }
  p.kmin = kmin; p.kmax = kmax; p.num = num; p.bad = bad;
  return p;
}
__device__ __forceinline__ void hist_merge(HistPartial& p, const HistPartial& q) {
  p.sum += q.sum; p.sq += q.sq;
  p.kmin = min(p.kmin, q.kmin); p.kmax = max(p.kmax, q.kmax);
  p.num += q.num; p.bad += q.bad;
}

// non-zero private buckets -> the record's counts, one integer atomic each
__device__ __forceinline__ void hist_flush(const unsigned* counts, int nb, unsigned* rec_counts) {
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    const unsigned c = counts[i];
    if (c) atomicAdd(&rec_counts[i], c);
  }
}

// ------------------------------------------------------------------------------------------------ flat buffer
__global__ __launch_bounds__(256) void histogram_values_kernel(const float* __restrict__ values, long n, long per_wg, const double* __restrict__ limits,
                                                               int nb, unsigned* __restrict__ rec_counts, HistPartial* __restrict__ partial) {
  extern __shared__ double hv_sm[];                 // [nb] limits | [4] wave partials | [nb] counts
  double* lim = hv_sm;
  HistPartial* red = reinterpret_cast<HistPartial*>(hv_sm + nb);
  unsigned* counts = reinterpret_cast<unsigned*>(hv_sm + nb + 5 * 4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < nb; i += 256) { lim[i] = limits[i]; counts[i] = 0u; }
  __syncthreads();
  HistLane a;
  hist_lane_init(a);
  const long begin = (long)blockIdx.x * per_wg, end = min(begin + per_wg, n);      // per_wg is a multiple of 256
  for (long base = begin; base < end; base += 256) {                               // (workgroup-uniform)
    const long i = base + threadIdx.x;
    const bool active = i < end;
    const float v = active ? values[i] : 0.f;
    hist_add(lim, nb, counts, v, active, lane, a);
  }
  const HistPartial p = hist_wave_reduce(a);
  if (lane == 0) red[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    HistPartial t = red[0];
    for (int w = 1; w < 4; ++w) hist_merge(t, red[w]);
    partial[blockIdx.x] = t;
  }
  hist_flush(counts, nb, rec_counts);
}

// ------------------------------------------------------------------------------------------------ one scale of a loss descriptor
struct HistSel {       // the sources of one launch: blockIdx.y -> slot, kind -> record index (-1: not selected)
  int n_src;
  unsigned char slot[H_SLOTS];
  signed char rec[H_SLOTS][H_KINDS];
};

// The features a source is made of (feature indices, in first-use order); masked: the mask feature's target is needed too.  Host and device.
__host__ __device__ inline int hist_needed(const dd_loss_desc& d, int slot, bool masked, int* need /*[DD_MAX_FEATURES]*/, int* fmap /*[DD_MAX_FEATURES]*/) {
  int n = 0;
  for (int f = 0; f < DD_MAX_FEATURES; ++f) fmap[f] = -1;
  auto add = [&](int f) { if (fmap[f] < 0) { fmap[f] = n; need[n++] = f; } };
  if (slot < DD_MAX_FEATURES) {
    add(slot);
    if (masked) add(d.mask_feature[slot]);
  } else if (slot < DD_MAX_FEATURES + DD_MAX_COMBINED) {
    const int k = slot - DD_MAX_FEATURES;
    for (int c = 0; c < 3; ++c) add(d.comb[k][c]);
    if (masked) add(d.comb_mask_feature[k]);
  } else {
    for (int j = 0; j < d.n_image_combined; ++j)
      for (int c = 0; c < 3; ++c) add(d.comb[d.image_combined[j]][c]);
    for (int j = 0; j < d.n_image_features; ++j) add(d.image_features[j]);
  }
  return n;
}

template <int NW>      // waves per workgroup; every wave walks tiles of its own
__global__ __launch_bounds__(64 * NW) void loss_histograms_kernel(const dd_loss_desc d, const HistSel sel, int B, int H, int W, int ntx, int ntiles,
                                                                  int stage_features, const double* __restrict__ limits, int nb,
                                                                  unsigned char* __restrict__ records, long rec_bytes,
                                                                  HistPartial* __restrict__ partial) {
  extern __shared__ double hl_sm[];                 // [nb] limits | [NW][3] wave partials | [3][nb] counts | fmap, need | [NW][stage_features][2][3][MT_TP]
  double* lim = hl_sm;
  HistPartial* red = reinterpret_cast<HistPartial*>(hl_sm + nb);
  unsigned* counts = reinterpret_cast<unsigned*>(hl_sm + nb + 5 * NW * H_KINDS);
  int* fmap = reinterpret_cast<int*>(counts + H_KINDS * nb);
  int* need = fmap + DD_MAX_FEATURES;
  int* nneed_sm = need + DD_MAX_FEATURES;
  float* stage = reinterpret_cast<float*>(nneed_sm + 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = sel.slot[blockIdx.y];
  int rec[H_KINDS];
#pragma unroll
  for (int k = 0; k < H_KINDS; ++k) rec[k] = sel.rec[blockIdx.y][k];

  for (int i = threadIdx.x; i < nb; i += 64 * NW) lim[i] = limits[i];
  for (int i = threadIdx.x; i < H_KINDS * nb; i += 64 * NW) counts[i] = 0u;
  if (threadIdx.x == 0) *nneed_sm = hist_needed(d, slot, rec[2] >= 0, need, fmap);
  __syncthreads();
  const int nneed = min(*nneed_sm, stage_features);      // (the launcher sized the staging area with the same function)
  float* mine = stage + (long)wave * stage_features * 6 * MT_TP;
  auto planes = [&](int i, int side) -> float* { return mine + (i * 2 + side) * 3 * MT_TP; };

  // what the source is (block-uniform)
  const int type = slot < DD_MAX_FEATURES ? 0 : (slot < DD_MAX_FEATURES + DD_MAX_COMBINED ? 1 : 2);
  const int comb_k = slot - DD_MAX_FEATURES;
  const int nch = (type == 0 && d.nch[slot] == 1) ? 1 : 3;
  const int mask_f = rec[2] >= 0 ? (type == 0 ? d.mask_feature[slot] : d.comb_mask_feature[comb_k]) : -1;
  const int mask_nch = mask_f >= 0 ? d.nch[mask_f] : 0;
  const int kind = d.kind;
  const float eps = d.epsilon;

  auto feat_val = [&](int f, int at, float (&p)[3], float (&t)[3]) {
    const float* pp = planes(fmap[f], 0);
    const float* tp = planes(fmap[f], 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = pp[c * MT_TP + at]; t[c] = tp[c * MT_TP + at]; }
  };
  auto comb_val = [&](int k, int at, float (&p)[3], float (&t)[3]) {      // color * (direct + indirect)
    float cp[3], ct[3], dp[3], dt[3], ip[3], it[3];
    feat_val(d.comb[k][0], at, cp, ct);
    feat_val(d.comb[k][1], at, dp, dt);
    feat_val(d.comb[k][2], at, ip, it);
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = cp[c] * (dp[c] + ip[c]); t[c] = ct[c] * (dt[c] + it[c]); }
  };
  auto value = [&](int at, float (&p)[3], float (&t)[3]) {
    if (type == 0) { feat_val(slot, at, p, t); return; }
    if (type == 1) { comb_val(comb_k, at, p, t); return; }
    p[0] = p[1] = p[2] = t[0] = t[1] = t[2] = 0.f;      // the image: sum of the combined features and single passes
    float ap[3], at3[3];
    for (int j = 0; j < d.n_image_combined; ++j) {
      comb_val(d.image_combined[j], at, ap, at3);
#pragma unroll
      for (int c = 0; c < 3; ++c) { p[c] += ap[c]; t[c] += at3[c]; }
    }
    for (int j = 0; j < d.n_image_features; ++j) {
      feat_val(d.image_features[j], at, ap, at3);
#pragma unroll
      for (int c = 0; c < 3; ++c) { p[c] += ap[c]; t[c] += at3[c]; }
    }
  };
  auto diff3 = [&](const float (&p)[3], const float (&t)[3]) -> float {      // channel-summed LossDifference (LossDifference.py:15-36)
    float s = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (ch >= nch) break;
      float l, dl;
      loss_term(kind, eps, p[ch], t[ch], &l, &dl);
      s += l;
    }
    return s;
  };

  HistLane acc[H_KINDS];
#pragma unroll
  for (int k = 0; k < H_KINDS; ++k) hist_lane_init(acc[k]);

  // this workgroup's chunk of the B * ntiles tiles; every wave makes the same number of rounds (the barriers)
  const long total = (long)B * ntiles, per = (total + gridDim.x - 1) / gridDim.x;
  const long begin = (long)blockIdx.x * per, end = min(begin + per, total);
  const int tx = lane & (MT_W - 1), ty = lane >> 4, o = ty * MT_PW + tx;
  for (long t0 = begin; t0 < end; t0 += NW) {       // (workgroup-uniform)
    const long t = t0 + wave;
    const bool valid = t < end;                     // (wave-uniform)
    int x0 = 0, y0 = 0;
    if (valid) {
      const int b = (int)(t / ntiles), tile = (int)(t - (long)b * ntiles);
      x0 = (tile % ntx) * MT_W;
      y0 = (tile / ntx) * MT_H;
      const int nrows = min(MT_PH, H - y0), ncols = min(MT_PW, W - x0);
      const bool halo = x0 + MT_W < W;
      const long pix0 = ((long)b * H + y0) * W + x0;
      for (int i0 = 0; i0 < nneed; i0 += MT_FB) {
        Staged st[MT_FB][2];
#pragma unroll
        for (int u = 0; u < MT_FB; ++u) {
          const int f = need[min(i0 + u, nneed - 1)];
          const bool one = d.nch[f] == 1;
#pragma unroll
          for (int side = 0; side < 2; ++side) {
            const float* base = side ? d.target[f] : d.pred[f];
            const int ld = side ? d.target_ld[f] : d.pred_ld[f];
            if (rows_vectorise(base, ld, W, x0)) st[u][side] = stage_issue(base + pix0 * ld, ld, one, W, nrows, halo, lane);
          }
        }
#pragma unroll
        for (int u = 0; u < MT_FB; ++u) {
          const int i = i0 + u;
          if (i >= nneed) break;
          const int f = need[i];
          const bool one = d.nch[f] == 1;
#pragma unroll
          for (int side = 0; side < 2; ++side) {
            const float* base = side ? d.target[f] : d.pred[f];
            const int ld = side ? d.target_ld[f] : d.pred_ld[f];
            if (rows_vectorise(base, ld, W, x0)) stage_commit(st[u][side], planes(i, side), ld, one, nrows, halo, lane);
            else stage_scalar(base + pix0 * ld, planes(i, side), ld, one, W, nrows, ncols, lane);
          }
        }
      }
    }
    __syncthreads();      // the tile is in LDS
    if (valid) {
      const bool live = x0 + tx < W && y0 + ty < H;
      const bool has_r = live && x0 + tx + 1 < W, has_d = live && y0 + ty + 1 < H;
      float v0 = 0.f, vr = 0.f, vd = 0.f, m = 0.f;
      if (live) {
        float cp[3], ct[3];
        value(o, cp, ct);
        v0 = diff3(cp, ct);
        if (rec[1] >= 0) {      // variation = second - first (Training.py:305-316); a pair belongs to its left / upper pixel
          const int off[2] = {1, MT_PW};
          const bool has[2] = {has_r, has_d};
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            if (!has[k]) continue;
            float np[3], nt[3], vp[3], vt[3];
            value(o + off[k], np, nt);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { vp[ch] = np[ch] - cp[ch]; vt[ch] = nt[ch] - ct[ch]; }
            (k ? vd : vr) = diff3(vp, vt);
          }
        }
        if (mask_f >= 0) {      // Conv2dUtilities.non_zero_mask of the colour pass's target
          const float* tm = planes(fmap[mask_f], 1);
          float sa = 0.f;
          for (int c = 0; c < mask_nch; ++c) sa += fabsf(tm[c * MT_TP + o]);
          m = sa > 0.f ? 1.f : 0.f;
        }
      }
      if (rec[0] >= 0) hist_add(lim, nb, counts, v0, live, lane, acc[0]);
      if (rec[1] >= 0) {
        hist_add(lim, nb, counts + nb, vr, has_r, lane, acc[1]);
        hist_add(lim, nb, counts + nb, vd, has_d, lane, acc[1]);
      }
      if (rec[2] >= 0) hist_add(lim, nb, counts + 2 * nb, v0 * m, live, lane, acc[2]);
    }
    __syncthreads();      // every wave is done with its tile before the next one is staged over it
  }

#pragma unroll
  for (int k = 0; k < H_KINDS; ++k) {
    const HistPartial p = hist_wave_reduce(acc[k]);
    if (lane == 0) red[wave * H_KINDS + k] = p;
  }
  __syncthreads();
  if (threadIdx.x < H_KINDS) {
    const int k = threadIdx.x, r = k == 0 ? rec[0] : (k == 1 ? rec[1] : rec[2]);
    if (r >= 0) {
      HistPartial t = red[k];
      for (int w = 1; w < NW; ++w) hist_merge(t, red[w * H_KINDS + k]);
      partial[(long)r * HC_MAX + blockIdx.x] = t;
    }
  }
#pragma unroll
  for (int k = 0; k < H_KINDS; ++k)
    if (rec[k] >= 0) hist_flush(counts + k * nb, nb, reinterpret_cast<unsigned*>(records + rec[k] * rec_bytes));
}

// record r: min, max, sum, sum_squares (double), num, nonfinite (64-bit) behind its counts, from partial[r * stride + 0 .. nwg) in index order
__global__ __launch_bounds__(64) void histogram_finalize_kernel(const HistPartial* __restrict__ partial, int nwg, int stride,
                                                                unsigned char* __restrict__ records, long rec_bytes, long stat_off) {
  const int r = blockIdx.x, lane = threadIdx.x;
  double sum = 0.0, sq = 0.0;
  unsigned kmin = 0xffffffffu, kmax = 0u;
  unsigned long long num = 0, bad = 0;
  for (int t = lane; t < nwg; t += 64) {
    const HistPartial q = partial[(long)r * stride + t];
    sum += q.sum; sq += q.sq;
    kmin = min(kmin, q.kmin); kmax = max(kmax, q.kmax);
    num += q.num; bad += q.bad;
  }
  sum = wave_sum_f64(sum);
  sq = wave_sum_f64(sq);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    num += (unsigned long long)__shfl_xor((long long)num, o);
    bad += (unsigned long long)__shfl_xor((long long)bad, o);
  }
  if (lane == 0) {
    double* s = reinterpret_cast<double*>(records + r * rec_bytes + stat_off);
    // an empty histogram keeps Histogram::Clear's min = DBL_MAX, max = -DBL_MAX
    s[0] = num ? (double)hist_unkey(kmin) : 1.7976931348623157e308;
    s[1] = num ? (double)hist_unkey(kmax) : -1.7976931348623157e308;
    s[2] = sum;
    s[3] = sq;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(s + 4);
    c[0] = num;
    c[1] = bad;
  }
}

size_t fixed_lds(int nb, int nw, int kinds) { return (size_t)nb * 8 + (size_t)40 * nw * kinds + (size_t)kinds * nb * 4; }

}  // namespace

extern "C" int dd_histogram_values(const float* values, long n, const double* limits, int nb, void* record, void* scratch, dd_stream stream) {
  DD_REQUIRE(values && limits && record && scratch, "dd_histogram_values: null values / limits / record / scratch");
  DD_REQUIRE(n > 0 && n < (1l << 32), "dd_histogram_values: n = %ld (1 .. 2^32 - 1: counts are 32-bit)", n);
  DD_REQUIRE(nb >= 3 && nb <= DD_HISTOGRAM_MAX_BUCKETS && (nb & 1), "dd_histogram_values: %d bucket limits (an odd number of 3 .. %d expected)", nb,
             DD_HISTOGRAM_MAX_BUCKETS);
  DD_REQUIRE(((uintptr_t)values & 3) == 0 && ((uintptr_t)limits & 7) == 0 && ((uintptr_t)record & 7) == 0 && ((uintptr_t)scratch & 7) == 0,
             "dd_histogram_values: values must be 4-byte aligned, limits / record / scratch 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long rec_bytes = DD_HISTOGRAM_RECORD_BYTES(nb), stat_off = DD_HISTOGRAM_STATS_OFFSET(nb);
  long nwg = (n + 4095) / 4096;
  if (nwg > HV_MAX_WG) nwg = HV_MAX_WG;
  const long per_wg = ((n + nwg - 1) / nwg + 255) / 256 * 256;
  nwg = (n + per_wg - 1) / per_wg;
  if (hipMemsetAsync(record, 0, (size_t)rec_bytes, st) != hipSuccess) {
    dd_set_error("dd_histogram_values: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return DD_ERR_LAUNCH;
  }
  const size_t lds = (size_t)nb * 8 + 40 * 4 + (size_t)nb * 4;
  hipLaunchKernelGGL(histogram_values_kernel, dim3((unsigned)nwg), dim3(256), lds, st, values, n, per_wg, limits, nb, reinterpret_cast<unsigned*>(record),
                     reinterpret_cast<HistPartial*>(scratch));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(histogram_finalize_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const HistPartial*>(scratch), (int)nwg, (int)nwg,
                     reinterpret_cast<unsigned char*>(record), rec_bytes, stat_off);
  DD_LAUNCH_CHECK();
  return DD_OK;
}

extern "C" long dd_loss_histograms_scratch_bytes(int B, int H, int W, int n_records) {
  if (B <= 0 || H <= 0 || W <= 0 || n_records <= 0 || n_records > DD_METRIC_SOURCES * H_KINDS) {
    dd_set_error("dd_loss_histograms_scratch_bytes: bad shape %d x %d x %d or record count %d", B, H, W, n_records);
    return DD_ERR_INVALID;
  }
  return (long)n_records * HC_MAX * (long)sizeof(HistPartial);
}

extern "C" int dd_loss_histograms(const dd_loss_desc* desc, int B, int H, int W, const int* selection, int n_records, const double* limits, int nb,
                                  void* records, void* scratch, dd_stream stream) {
  DD_REQUIRE(desc && selection && limits && records && scratch, "dd_loss_histograms: null descriptor / selection / limits / records / scratch");
  DD_REQUIRE(B > 0 && H > 0 && W > 0 && 2l * B * H * W < (1l << 32), "dd_loss_histograms: bad shape %d x %d x %d (2 B H W < 2^32: counts are 32-bit)", B, H, W);
  DD_REQUIRE(n_records > 0 && n_records <= DD_METRIC_SOURCES * H_KINDS, "dd_loss_histograms: %d records", n_records);
  DD_REQUIRE(nb >= 3 && nb <= DD_HISTOGRAM_MAX_BUCKETS && (nb & 1), "dd_loss_histograms: %d bucket limits (an odd number of 3 .. %d expected)", nb,
             DD_HISTOGRAM_MAX_BUCKETS);
  DD_REQUIRE(((uintptr_t)limits & 7) == 0 && ((uintptr_t)records & 7) == 0 && ((uintptr_t)scratch & 7) == 0,
             "dd_loss_histograms: limits, records and scratch must be 8-byte aligned");
  DD_REQUIRE(desc->n_features > 0 && desc->n_features <= DD_MAX_FEATURES && desc->n_combined >= 0 && desc->n_combined <= DD_MAX_COMBINED,
             "dd_loss_histograms: n_features / n_combined out of range");
  DD_REQUIRE(desc->n_image_combined >= 0 && desc->n_image_combined <= DD_MAX_COMBINED && desc->n_image_features >= 0 &&
                 desc->n_image_features <= DD_MAX_FEATURES, "dd_loss_histograms: image member counts out of range");
  DD_REQUIRE(desc->kind >= 1 && desc->kind <= 5, "dd_loss_histograms: unknown loss kind %d", desc->kind);
  for (int f = 0; f < desc->n_features; ++f) {
    DD_REQUIRE(desc->pred[f] && desc->target[f], "dd_loss_histograms: feature %d has a null pred / target", f);
    DD_REQUIRE(desc->nch[f] == 1 || desc->nch[f] == 3, "dd_loss_histograms: feature %d has %d channels (1 or 3 expected)", f, desc->nch[f]);
    DD_REQUIRE(desc->pred_ld[f] >= desc->nch[f] && desc->target_ld[f] >= desc->nch[f], "dd_loss_histograms: feature %d has a pixel stride below its channels", f);
    DD_REQUIRE(((uintptr_t)desc->pred[f] & 3) == 0 && ((uintptr_t)desc->target[f] & 3) == 0, "dd_loss_histograms: feature %d is not 4-byte aligned", f);
    DD_REQUIRE(desc->mask_feature[f] >= -1 && desc->mask_feature[f] < desc->n_features, "dd_loss_histograms: mask_feature[%d] is not a feature index", f);
  }
  for (int k = 0; k < desc->n_combined; ++k) {
    for (int c = 0; c < 3; ++c)
      DD_REQUIRE(desc->comb[k][c] >= 0 && desc->comb[k][c] < desc->n_features, "dd_loss_histograms: comb[%d][%d] is not a feature index", k, c);
    DD_REQUIRE(desc->comb_mask_feature[k] >= -1 && desc->comb_mask_feature[k] < desc->n_features,
               "dd_loss_histograms: comb_mask_feature[%d] is not a feature index", k);
  }
  for (int i = 0; i < desc->n_image_combined; ++i)
    DD_REQUIRE(desc->image_combined[i] >= 0 && desc->image_combined[i] < desc->n_combined, "dd_loss_histograms: image_combined[%d] is not a combined index", i);
  for (int i = 0; i < desc->n_image_features; ++i)
    DD_REQUIRE(desc->image_features[i] >= 0 && desc->image_features[i] < desc->n_features, "dd_loss_histograms: image_features[%d] is not a feature index", i);

  // selection[2 r] = slot, selection[2 r + 1] = kind of record r
  int rec_of[H_SLOTS][H_KINDS];
  for (int s = 0; s < H_SLOTS; ++s)
    for (int k = 0; k < H_KINDS; ++k) rec_of[s][k] = -1;
  for (int r = 0; r < n_records; ++r) {
    const int slot = selection[2 * r], kind = selection[2 * r + 1];
    DD_REQUIRE(kind >= 0 && kind < H_KINDS, "dd_loss_histograms: selection %d has kind %d", r, kind);
    const bool is_f = slot >= 0 && slot < desc->n_features, is_c = slot >= DD_MAX_FEATURES && slot < DD_MAX_FEATURES + desc->n_combined;
    const bool is_i = slot == DD_MAX_FEATURES + DD_MAX_COMBINED && (desc->n_image_combined > 0 || desc->n_image_features > 0);
    DD_REQUIRE(is_f || is_c || is_i, "dd_loss_histograms: selection %d names slot %d, which the descriptor does not have", r, slot);
    if (kind == DD_HISTOGRAM_MASKED_DIFFERENCE)
      DD_REQUIRE((is_f && desc->mask_feature[slot] >= 0) || (is_c && desc->comb_mask_feature[slot - DD_MAX_FEATURES] >= 0),
                 "dd_loss_histograms: selection %d asks for the masked difference of slot %d, which has no mask feature", r, slot);
    DD_REQUIRE(rec_of[slot][kind] < 0, "dd_loss_histograms: selection %d repeats (slot %d, kind %d)", r, slot, kind);
    rec_of[slot][kind] = r;
  }
  // two launches: sources made of few features (4 tiles in flight per workgroup) and the others (the image: as many waves as LDS allows)
  HistSel few, many;
  few.n_src = many.n_src = 0;
  int few_need = 0, many_need = 0;
  for (int s = 0; s < H_SLOTS; ++s) {
    if (rec_of[s][0] < 0 && rec_of[s][1] < 0 && rec_of[s][2] < 0) continue;
    int need[DD_MAX_FEATURES], fmap[DD_MAX_FEATURES];
    const int n = hist_needed(*desc, s, rec_of[s][2] >= 0, need, fmap);
    HistSel& g = n <= 4 ? few : many;
    int& gn = n <= 4 ? few_need : many_need;
    g.slot[g.n_src] = (unsigned char)s;
    for (int k = 0; k < H_KINDS; ++k) g.rec[g.n_src][k] = (signed char)rec_of[s][k];
    ++g.n_src;
    if (n > gn) gn = n;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long rec_bytes = DD_HISTOGRAM_RECORD_BYTES(nb), stat_off = DD_HISTOGRAM_STATS_OFFSET(nb);
  if (hipMemsetAsync(records, 0, (size_t)rec_bytes * n_records, st) != hipSuccess) {
    dd_set_error("dd_loss_histograms: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return DD_ERR_LAUNCH;
  }
  const int ntx = (W + MT_W - 1) / MT_W, ntiles = ntx * ((H + MT_H - 1) / MT_H);
  const long total = (long)B * ntiles;
  int chunks = (int)((total + 15) / 16);
  if (chunks > HC_MAX) chunks = HC_MAX;
  const long per = (total + chunks - 1) / chunks;
  chunks = (int)((total + per - 1) / per);      // (no empty workgroup: every partial of 0 .. chunks-1 is written)
  auto lds_of = [&](int nw, int nneed) { return fixed_lds(nb, nw, H_KINDS) + (2 * DD_MAX_FEATURES + 2) * sizeof(int) + (size_t)nw * nneed * 6 * MT_TP * sizeof(float); };
  unsigned char* recs = reinterpret_cast<unsigned char*>(records);
  HistPartial* part = reinterpret_cast<HistPartial*>(scratch);
  if (few.n_src) {
    dd_allow_max_lds(reinterpret_cast<const void*>(loss_histograms_kernel<4>), 160 * 1024);
    hipLaunchKernelGGL(loss_histograms_kernel<4>, dim3((unsigned)chunks, (unsigned)few.n_src), dim3(256), lds_of(4, few_need), st, *desc, few, B, H, W, ntx,
                       ntiles, few_need, limits, nb, recs, rec_bytes, part);
    DD_LAUNCH_CHECK();
  }
  if (many.n_src) {
    const size_t cap = 152 * 1024;
    if (lds_of(4, many_need) <= cap) {
      dd_allow_max_lds(reinterpret_cast<const void*>(loss_histograms_kernel<4>), 160 * 1024);
      hipLaunchKernelGGL(loss_histograms_kernel<4>, dim3((unsigned)chunks, (unsigned)many.n_src), dim3(256), lds_of(4, many_need), st, *desc, many, B, H, W,
                         ntx, ntiles, many_need, limits, nb, recs, rec_bytes, part);
    } else if (lds_of(2, many_need) <= cap) {
      dd_allow_max_lds(reinterpret_cast<const void*>(loss_histograms_kernel<2>), 160 * 1024);
      hipLaunchKernelGGL(loss_histograms_kernel<2>, dim3((unsigned)chunks, (unsigned)many.n_src), dim3(128), lds_of(2, many_need), st, *desc, many, B, H, W,
                         ntx, ntiles, many_need, limits, nb, recs, rec_bytes, part);
    } else {
      DD_REQUIRE(lds_of(1, many_need) <= cap, "dd_loss_histograms: a source of %d features does not fit in LDS", many_need);
      dd_allow_max_lds(reinterpret_cast<const void*>(loss_histograms_kernel<1>), 160 * 1024);
      hipLaunchKernelGGL(loss_histograms_kernel<1>, dim3((unsigned)chunks, (unsigned)many.n_src), dim3(64), lds_of(1, many_need), st, *desc, many, B, H, W,
                         ntx, ntiles, many_need, limits, nb, recs, rec_bytes, part);
    }
    DD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(histogram_finalize_kernel, dim3((unsigned)n_records), dim3(64), 0, st, part, chunks, HC_MAX, recs, rec_bytes, stat_off);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
