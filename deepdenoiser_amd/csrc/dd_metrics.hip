// Tracked metrics (the `statistics` / `statistics_masked` sections of Training.json; BaseFeatureTraining.add_tracked_metrics_to_dictionary,
// Training.py:283-302): for every loss source of ONE scale (features, combined features, the combined image) and every image of the batch the
// four sums the tracked scalars are made of -- difference, variation difference, masked difference, mask (include/dd_hip.h: dd_loss_metrics).
//
//   metrics : one workgroup per 16 x 4 pixel tile of one image.  The tile (+ one halo column and row for the variation pairs) of EVERY
//             feature's prediction and target is staged in LDS once -- float4 loads where the rows allow it, the loads of 4 features per
//             wave in flight together -- and all sources are evaluated from there: the combined products and the image sum are formed from
//             LDS, as loss_general_kernel does.  A wave owns the 64 pixels of the tile; with many sources (the 17-pass example network has
//             17 + 4 + 1) the workgroup has 4 waves that share the staging and take every 4th source each: one wave's chain of dependent
//             loads and reductions is what bounds a launch of a few thousand tiles, not the bytes.  A wave adds its 64 pixels in a fixed
//             butterfly and stores one float4 per source into the scratch.
//   reduce  : one wave per (source, image) adds the tile partials in index order (lane-strided, then the same butterfly).
// No atomics, no float order that depends on scheduling: two runs give the same bits.
#include "dd_common.h"
#include "dd_loss_common.h"
#include "dd_metrics_stage.h"

namespace {

template <int NW>      // waves per workgroup
__global__ __launch_bounds__(64 * NW) void loss_metrics_kernel(const dd_loss_desc d, int B, int H, int W, int ntx, float4* __restrict__ partial) {
  extern __shared__ float mt_sm[];                  // [n_features][2 (pred, target)][3][MT_TP]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tile = blockIdx.x, b = blockIdx.y, ntiles = gridDim.x;
  const int x0 = (tile % ntx) * MT_W, y0 = (tile / ntx) * MT_H;
  const int nrows = min(MT_PH, H - y0), ncols = min(MT_PW, W - x0);      // staged rows / columns (halo included where it exists)
  const bool halo = x0 + MT_W < W;
  const long pix0 = ((long)b * H + y0) * W + x0;
  auto planes = [&](int f, int side) -> float* { return mt_sm + (f * 2 + side) * 3 * MT_TP; };

  for (int f0 = wave * MT_FB; f0 < d.n_features; f0 += NW * MT_FB) {      // (wave-uniform)
    Staged st[MT_FB][2];
#pragma unroll
    for (int u = 0; u < MT_FB; ++u) {
      const int f = min(f0 + u, d.n_features - 1);
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
      const int f = f0 + u;
      if (f >= d.n_features) break;
      const bool one = d.nch[f] == 1;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const float* base = side ? d.target[f] : d.pred[f];
        const int ld = side ? d.target_ld[f] : d.pred_ld[f];
        if (rows_vectorise(base, ld, W, x0)) stage_commit(st[u][side], planes(f, side), ld, one, nrows, halo, lane);
        else stage_scalar(base + pix0 * ld, planes(f, side), ld, one, W, nrows, ncols, lane);
      }
    }
  }
  __syncthreads();

  const int tx = lane & (MT_W - 1), ty = lane >> 4;
  const bool live = x0 + tx < W && y0 + ty < H;
  const bool has_r = live && x0 + tx + 1 < W, has_d = live && y0 + ty + 1 < H;
  const int o = ty * MT_PW + tx;
  const int kind = d.kind;
  const float eps = d.epsilon;

  // channel-summed LossDifference of (p, t) (LossDifference.py:15-36)
  auto diff3 = [&](const float (&p)[3], const float (&t)[3], int nch) -> float {
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
  // the four sums of one source; value(offset, p, t) gives the source at a tile position
  auto emit = [&](auto value, int nch, int mask_f, int slot) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      float cp[3], ct[3];
      value(o, cp, ct);
      v[0] = diff3(cp, ct, nch);
      // variation = second - first (Training.py:305-316: shift_left - shift_right = x[j+1] - x[j]); a pair belongs to its left / upper pixel
      const int off[2] = {1, MT_PW};
      const bool has[2] = {has_r, has_d};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (!has[k]) continue;
        float np[3], nt[3], vp[3], vt[3];
        value(o + off[k], np, nt);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { vp[ch] = np[ch] - cp[ch]; vt[ch] = nt[ch] - ct[ch]; }
        v[1] += diff3(vp, vt, nch);
      }
      if (mask_f >= 0) {      // Conv2dUtilities.non_zero_mask of the colour pass's target (target_mask of dd_loss_common.h, from LDS)
        const float* tm = planes(mask_f, 1);
        float sa = 0.f;
        for (int c = 0; c < d.nch[mask_f]; ++c) sa += fabsf(tm[c * MT_TP + o]);
        const float m = sa > 0.f ? 1.f : 0.f;
        v[2] = v[0] * m;
        v[3] = m;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) partial[((long)slot * B + b) * ntiles + tile] = make_float4(v[0], v[1], v[2], v[3]);
  };
  auto feat_val = [&](int f, int at, float (&p)[3], float (&t)[3]) {
    const float* pp = planes(f, 0);
    const float* tp = planes(f, 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = pp[c * MT_TP + at]; t[c] = tp[c * MT_TP + at]; }
  };
  auto comb_val = [&](int k, int at, float (&p)[3], float (&t)[3]) {      // color * (direct + indirect), as combined_value
    float cp[3], ct[3], dp[3], dt[3], ip[3], it[3];
    feat_val(d.comb[k][0], at, cp, ct);
    feat_val(d.comb[k][1], at, dp, dt);
    feat_val(d.comb[k][2], at, ip, it);
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = cp[c] * (dp[c] + ip[c]); t[c] = ct[c] * (dt[c] + it[c]); }
  };
  auto image_val = [&](int at, float (&p)[3], float (&t)[3]) {            // sum of the combined features and single passes, as image_value
    p[0] = p[1] = p[2] = t[0] = t[1] = t[2] = 0.f;
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

  // sources are dealt to the waves in turn, the most expensive ones (image, combined) first
  int turn = 0;
  auto mine = [&]() { return (turn++ % NW) == wave; };
  if ((d.n_image_combined > 0 || d.n_image_features > 0) && mine())
    emit([&](int at, float (&p)[3], float (&t)[3]) { image_val(at, p, t); }, 3, -1, DD_MAX_FEATURES + DD_MAX_COMBINED);
  for (int k = 0; k < d.n_combined; ++k)
    if (mine()) emit([&](int at, float (&p)[3], float (&t)[3]) { comb_val(k, at, p, t); }, 3, d.comb_mask_feature[k], DD_MAX_FEATURES + k);
  for (int f = 0; f < d.n_features; ++f)
    if (mine()) emit([&](int at, float (&p)[3], float (&t)[3]) { feat_val(f, at, p, t); }, d.nch[f] == 1 ? 1 : 3, d.mask_feature[f], f);
}

// table[slot][b] = sum over the tiles, in index order; rows of sources the descriptor does not have are zero
__global__ __launch_bounds__(64) void loss_metrics_reduce_kernel(const float4* __restrict__ partial, float4* __restrict__ table, int B, int ntiles,
                                                                 unsigned long long active) {
  const int row = blockIdx.x, slot = row / B, lane = threadIdx.x;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((active >> slot) & 1ull) {
    for (int t = lane; t < ntiles; t += 64) {
      const float4 q = partial[(long)row * ntiles + t];
      a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
    }
    a.x = wave_sum(a.x); a.y = wave_sum(a.y); a.z = wave_sum(a.z); a.w = wave_sum(a.w);
  }
  if (lane == 0) table[row] = a;
}

int tiles_of(int H, int W, int* ntx) {
  *ntx = (W + MT_W - 1) / MT_W;
  return *ntx * ((H + MT_H - 1) / MT_H);
}

}  // namespace

extern "C" long dd_loss_metrics_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535) {
    dd_set_error("dd_loss_metrics_scratch_bytes: bad shape %d x %d x %d", B, H, W);
    return DD_ERR_INVALID;
  }
  int ntx;
  return (long)MT_SOURCES * B * tiles_of(H, W, &ntx) * (long)sizeof(float4);
}

extern "C" int dd_loss_metrics(const dd_loss_desc* desc, int B, int H, int W, float* scratch, float* table, dd_stream stream) {
  DD_REQUIRE(desc && scratch && table, "dd_loss_metrics: null descriptor / scratch / table");
  DD_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535, "dd_loss_metrics: bad shape %d x %d x %d", B, H, W);
  DD_REQUIRE(desc->n_features > 0 && desc->n_features <= DD_MAX_FEATURES && desc->n_combined >= 0 && desc->n_combined <= DD_MAX_COMBINED,
             "dd_loss_metrics: n_features / n_combined out of range");
  DD_REQUIRE(desc->n_image_combined >= 0 && desc->n_image_combined <= DD_MAX_COMBINED && desc->n_image_features >= 0 &&
                 desc->n_image_features <= DD_MAX_FEATURES, "dd_loss_metrics: image member counts out of range");
  DD_REQUIRE(desc->kind >= 1 && desc->kind <= 5, "dd_loss_metrics: unknown loss kind %d", desc->kind);
  DD_REQUIRE(((uintptr_t)scratch & 15) == 0 && ((uintptr_t)table & 15) == 0, "dd_loss_metrics: scratch and table must be 16-byte aligned");
  unsigned long long active = 0;
  for (int f = 0; f < desc->n_features; ++f) {
    DD_REQUIRE(desc->pred[f] && desc->target[f], "dd_loss_metrics: feature %d has a null pred / target", f);
    DD_REQUIRE(desc->nch[f] == 1 || desc->nch[f] == 3, "dd_loss_metrics: feature %d has %d channels (1 or 3 expected)", f, desc->nch[f]);
    DD_REQUIRE(desc->pred_ld[f] >= desc->nch[f] && desc->target_ld[f] >= desc->nch[f], "dd_loss_metrics: feature %d has a pixel stride below its channels", f);
    DD_REQUIRE(desc->mask_feature[f] >= -1 && desc->mask_feature[f] < desc->n_features, "dd_loss_metrics: mask_feature[%d] is not a feature index", f);
    active |= 1ull << f;
  }
  for (int k = 0; k < desc->n_combined; ++k) {
    for (int c = 0; c < 3; ++c)
      DD_REQUIRE(desc->comb[k][c] >= 0 && desc->comb[k][c] < desc->n_features, "dd_loss_metrics: comb[%d][%d] is not a feature index", k, c);
    DD_REQUIRE(desc->comb_mask_feature[k] >= -1 && desc->comb_mask_feature[k] < desc->n_features,
               "dd_loss_metrics: comb_mask_feature[%d] is not a feature index", k);
    active |= 1ull << (DD_MAX_FEATURES + k);
  }
  for (int i = 0; i < desc->n_image_combined; ++i)
    DD_REQUIRE(desc->image_combined[i] >= 0 && desc->image_combined[i] < desc->n_combined, "dd_loss_metrics: image_combined[%d] is not a combined index", i);
  for (int i = 0; i < desc->n_image_features; ++i)
    DD_REQUIRE(desc->image_features[i] >= 0 && desc->image_features[i] < desc->n_features, "dd_loss_metrics: image_features[%d] is not a feature index", i);
  if (desc->n_image_combined > 0 || desc->n_image_features > 0) active |= 1ull << (DD_MAX_FEATURES + DD_MAX_COMBINED);
  int ntx;
  const int ntiles = tiles_of(H, W, &ntx);
  const size_t lds = (size_t)desc->n_features * 6 * MT_TP * sizeof(float);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n_sources = desc->n_features + desc->n_combined + ((active >> (DD_MAX_FEATURES + DD_MAX_COMBINED)) & 1ull ? 1 : 0);
  if (n_sources > 2) {
    dd_allow_max_lds(reinterpret_cast<const void*>(loss_metrics_kernel<4>), 96 * 1024);
    hipLaunchKernelGGL(loss_metrics_kernel<4>, dim3((unsigned)ntiles, (unsigned)B), dim3(256), lds, st, *desc, B, H, W, ntx, reinterpret_cast<float4*>(scratch));
  } else {
    dd_allow_max_lds(reinterpret_cast<const void*>(loss_metrics_kernel<1>), 96 * 1024);
    hipLaunchKernelGGL(loss_metrics_kernel<1>, dim3((unsigned)ntiles, (unsigned)B), dim3(64), lds, st, *desc, B, H, W, ntx, reinterpret_cast<float4*>(scratch));
  }
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_metrics_reduce_kernel, dim3((unsigned)(MT_SOURCES * B)), dim3(64), 0, st, reinterpret_cast<const float4*>(scratch),
                     reinterpret_cast<float4*>(table), B, ntiles, active);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
