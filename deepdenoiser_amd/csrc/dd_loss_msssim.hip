// dd_loss_msssim.hip -- the MS-SSIM loss term of BaseFeatureTraining (Training.py:178-204, added to the loss at :231-232):
//   term = weight * (1 - mean_b MS(pred_b, target_b)),  MS = mean_c relu(cs_0)^0.0448 relu(cs_1)^0.2856 relu(ssim_2)^0.3001
// = tf.image.ssim_multiscale(pred, target, 1.0, power_factors=(0.0448, 0.2856, 0.3001)) of TF 1.x (11x11 Gaussian, sigma 1.5, k1 0.01, k2 0.03).
//
// All arithmetic is fp32 on the vector pipe (s2 - mx^2 - my^2 cancels in flat regions against c2 = 9e-4: no half precision, no reduced-
// precision matrix instructions).  One workgroup = one 16x16 tile of one (source, image, channel) plane at one level:
//   forward : tile + 10-pixel halo of both tensors -> LDS once, separable 11-tap row pass (4 maps as one float4) and column pass, cs / lum*cs
//             reduced over the tile in a fixed order -> partial[source][image][channel][level tile]; the level-k pass also writes the 2x2
//             pooled planes of level k+1 (planar fp32 in scratch: the backward reads them again).  Combined sources color*(direct+indirect)
//             and the image sum are formed from their parts while the tile is loaded, never stored at full size.
//   coef    : adds the tile partials in index order, forms MS and dMS/d cs_0, dMS/d cs_1, dMS/d ssim_2 per (source, image, channel);
//   total   : one workgroup adds (1 - MS) in a fixed tree and adds the weighted terms to loss_out[0].
//   backward: per level, the filtered maps are RECOMPUTED from LDS on the tile + 20-pixel halo, the three partial-derivative maps
//             (d/d mx, d/d sxy, d/d s2) at the valid positions are filtered by the transposed Gaussian, combined pointwise
//             (g = G^T a + y G^T b + 2 x G^T c), a quarter of the coarser level's gradient is added; level 0 routes g into dpred.
// No fp32 atomics anywhere: every reduction has a fixed order, so the term and its gradient are bit-identical run to run.
#include <hip/hip_runtime.h>

#include "../../include/dd_hip.h"
#include "dd_common.h"

namespace {

constexpr int T = 16;            // tile edge
constexpr int FS = 11;           // filter size
constexpr int HALO = FS - 1;
constexpr int FIN = T + HALO;    // forward input tile edge (26)
constexpr int BP = T + HALO;     // backward: positions whose windows touch the tile (26)
constexpr int BIN = BP + HALO;   // backward input tile edge (36)
constexpr int NTHREADS = 256;
constexpr int MAX_SRC = DD_MAX_FEATURES + DD_MAX_COMBINED + 1;
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

// softmax(-i^2 / (2 sigma^2)), i = -5 .. 5, sigma = 1.5 (_fspecial_gauss: the 2-D kernel is the outer product of this, exp(a + b))
__device__ __forceinline__ float gauss(int t) {
  constexpr float G[FS] = {1.0283800845e-03f, 7.5987581352e-03f, 3.6000772128e-02f, 1.0936068951e-01f, 2.1300553771e-01f, 2.6601172486e-01f,
                           2.1300553771e-01f, 1.0936068951e-01f, 3.6000772128e-02f, 7.5987581352e-03f, 1.0283800845e-03f};
  return G[t];
}

struct MsArgs {
  const float* pred[DD_MAX_FEATURES];
  const float* target[DD_MAX_FEATURES];
  float* dpred[DD_MAX_FEATURES];
  int pred_ld[DD_MAX_FEATURES];
  int target_ld[DD_MAX_FEATURES];
  int comb[DD_MAX_COMBINED][3];
  int n_img_comb, n_img_feat;
  int img_comb[DD_MAX_COMBINED];
  int img_feat[DD_MAX_FEATURES];
  int n_src;
  int src_kind[MAX_SRC];   // 0 feature, 1 combined, 2 image
  int src_idx[MAX_SRC];
  float src_w[MAX_SRC];
  int B, H, W;
  // scratch sections (floats)
  float* pool[2];          // [level-1]: [S][B][3][2 (x, y)][h][w]
  float* grad[2];          // [level-1]: [S][B][3][h][w]
  float* partial;          // [S][B][3][nt0 + nt1 + nt2][2]
  float* coef;             // [S][B][3][4]: d term / d (sum of cs_0), (sum of cs_1), (sum of ssim_2); MS
};

struct Level {
  int h, w, ntx, nty, btx, bty;
};
__host__ __device__ inline Level level_of(int H, int W, int k) {
  Level l;
  l.h = H >> k, l.w = W >> k;
  l.ntx = (l.w - HALO + T - 1) / T, l.nty = (l.h - HALO + T - 1) / T;   // forward tiles over the (h-10) x (w-10) valid positions
  l.btx = (l.w + T - 1) / T, l.bty = (l.h + T - 1) / T;                 // backward tiles over the h x w pixels
  return l;
}

// ---- level-0 sources, formed from their parts
template <bool TGT> __device__ __forceinline__ float feat_at(const MsArgs& a, int f, long pix, int ch) {
  return TGT ? a.target[f][pix * a.target_ld[f] + ch] : a.pred[f][pix * a.pred_ld[f] + ch];
}
template <bool TGT> __device__ __forceinline__ float comb_at(const MsArgs& a, int k, long pix, int ch) {
  return feat_at<TGT>(a, a.comb[k][0], pix, ch) * (feat_at<TGT>(a, a.comb[k][1], pix, ch) + feat_at<TGT>(a, a.comb[k][2], pix, ch));
}
template <bool TGT> __device__ __forceinline__ float source_at(const MsArgs& a, int kind, int idx, long pix, int ch) {
  if (kind == 0) return feat_at<TGT>(a, idx, pix, ch);
  if (kind == 1) return comb_at<TGT>(a, idx, pix, ch);
  float s = 0.f;
  for (int i = 0; i < a.n_img_comb; ++i) s += comb_at<TGT>(a, a.img_comb[i], pix, ch);
  for (int i = 0; i < a.n_img_feat; ++i) s += feat_at<TGT>(a, a.img_feat[i], pix, ch);
  return s;
}

// x / y of plane (s, b, ch) at level k, pixel (r, c); zero outside the plane
template <int K> __device__ __forceinline__ void load_xy(const MsArgs& a, const Level& l, int s, int b, int ch, int r, int c, float& x, float& y) {
  x = y = 0.f;
  if (r < 0 || c < 0 || r >= l.h || c >= l.w) return;
  if (K == 0) {
    long pix = ((long)b * l.h + r) * l.w + c;
    x = source_at<false>(a, a.src_kind[s], a.src_idx[s], pix, ch);
    y = source_at<true>(a, a.src_kind[s], a.src_idx[s], pix, ch);
  } else {
    const float* p = a.pool[K - 1] + (((long)s * a.B + b) * 3 + ch) * 2 * l.h * l.w;
    x = p[(long)r * l.w + c];
    y = p[(long)(l.h + r) * l.w + c];
  }
}

// forward tiles of one (source, image, channel) plane over the three levels = entries of its row of `partial`
__device__ __forceinline__ int tiles_per_plane(const MsArgs& a) {
  Level l0 = level_of(a.H, a.W, 0), l1 = level_of(a.H, a.W, 1), l2 = level_of(a.H, a.W, 2);
  return l0.ntx * l0.nty + l1.ntx * l1.nty + l2.ntx * l2.nty;
}
__device__ __forceinline__ long partial_index(const MsArgs& a, int s, int b, int ch) {
  return (((long)s * a.B + b) * 3 + ch) * tiles_per_plane(a);
}
__device__ __forceinline__ int partial_level_offset(const MsArgs& a, int k) {
  int off = 0;
  for (int j = 0; j < k; ++j) {
    Level l = level_of(a.H, a.W, j);
    off += l.ntx * l.nty;
  }
  return off;
}

// filtered maps (mx, my, sxy, s2) -> cs, lum
__device__ __forceinline__ void ssim_point(float4 m, float& cs, float& lum, float& D, float& Bq) {
  float N = 2.f * m.z - 2.f * m.x * m.y + C2;
  D = m.w - m.x * m.x - m.y * m.y + C2;
  cs = N / D;
  Bq = m.x * m.x + m.y * m.y + C1;
  lum = (2.f * m.x * m.y + C1) / Bq;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int K> __global__ __launch_bounds__(NTHREADS) void msssim_fwd_kernel(MsArgs a) {
  __shared__ float sx[FIN][FIN + 1], sy[FIN][FIN + 1];
  __shared__ float4 R[FIN][T];
  __shared__ float red[2][NTHREADS / 64];
  const Level l = level_of(a.H, a.W, K);
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, ty = tile / l.ntx, tx = tile % l.ntx;
  const int b = blockIdx.y / 3, ch = blockIdx.y % 3, s = blockIdx.z;
  const int r0 = ty * T, c0 = tx * T;
  for (int i = tid; i < FIN * FIN; i += NTHREADS) {
    int r = i / FIN, c = i % FIN;
    load_xy<K>(a, l, s, b, ch, r0 + r, c0 + c, sx[r][c], sy[r][c]);
  }
  __syncthreads();
  if (K < 2) {   // 2x2 / stride-2 average pool of the pixels this tile owns (the last tile of a row / column also owns its halo)
    const int hn = l.h >> 1, wn = l.w >> 1;
    const int own_r = (ty == l.nty - 1 ? l.h - r0 : T) >> 1, own_c = (tx == l.ntx - 1 ? l.w - c0 : T) >> 1;
    float* p = a.pool[K] + (((long)s * a.B + b) * 3 + ch) * 2 * hn * wn;
    for (int i = tid; i < own_r * own_c; i += NTHREADS) {
      int r = i / own_c, c = i % own_c;
      long o = (long)((r0 >> 1) + r) * wn + (c0 >> 1) + c;
      p[o] = 0.25f * (sx[2 * r][2 * c] + sx[2 * r][2 * c + 1] + sx[2 * r + 1][2 * c] + sx[2 * r + 1][2 * c + 1]);
      p[o + (long)hn * wn] = 0.25f * (sy[2 * r][2 * c] + sy[2 * r][2 * c + 1] + sy[2 * r + 1][2 * c] + sy[2 * r + 1][2 * c + 1]);
    }
  }
  for (int i = tid; i < FIN * T; i += NTHREADS) {   // row pass
    int r = i / T, c = i % T;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t), x = sx[r][c + t], y = sy[r][c + t];
      m.x += g * x, m.y += g * y, m.z += g * (x * y), m.w += g * (x * x + y * y);
    }
    R[r][c] = m;
  }
  __syncthreads();
  float vcs = 0.f, vss = 0.f;
  {   // column pass: one valid position per thread
    int r = tid / T, c = tid % T;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t);
      float4 v = R[r + t][c];
      m.x += g * v.x, m.y += g * v.y, m.z += g * v.z, m.w += g * v.w;
    }
    if (r0 + r < l.h - HALO && c0 + c < l.w - HALO) {
      float cs, lum, D, Bq;
      ssim_point(m, cs, lum, D, Bq);
      vcs = cs, vss = lum * cs;
    }
  }
  // fixed-order reduction: butterfly inside each wave, then the four waves in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vcs += __shfl_down(vcs, o), vss += __shfl_down(vss, o);
  if ((tid & 63) == 0) red[0][tid >> 6] = vcs, red[1][tid >> 6] = vss;
  __syncthreads();
  if (tid == 0) {
    float* p = a.partial + (partial_index(a, s, b, ch) + partial_level_offset(a, K) + tile) * 2;
    p[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    p[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// ---------------------------------------------------------------------------------------------------------------- coefficients
__global__ __launch_bounds__(64) void msssim_coef_kernel(MsArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_src * a.B * 3) return;
  const int s = i / (a.B * 3);
  const float* p = a.partial + (long)i * tiles_per_plane(a) * 2;      // i = (s * B + b) * 3 + ch
  const float pw[3] = {0.0448f, 0.2856f, 0.3001f};
  float v[3], n[3];
  for (int k = 0; k < 3; ++k) {
    Level l = level_of(a.H, a.W, k);
    float sum = 0.f;
    for (int t = 0; t < l.ntx * l.nty; ++t) sum += p[2 * t + (k == 2 ? 1 : 0)];   // mcs.pop(): level 2 contributes ssim, 0 and 1 cs
    p += 2 * l.ntx * l.nty;
    n[k] = (float)((l.h - HALO) * (l.w - HALO));
    v[k] = sum / n[k];
  }
  float* c = a.coef + (long)i * 4;
  if (!(v[0] <= 0.f || v[1] <= 0.f || v[2] <= 0.f)) {      // (a NaN is not a clamp: it goes through pow into MS and the coefficients)
    float ms = powf(v[0], pw[0]) * powf(v[1], pw[1]) * powf(v[2], pw[2]);
    float scale = -a.src_w[s] / (3.f * (float)a.B);      // term = w (1 - mean over images and channels of MS)
    for (int k = 0; k < 3; ++k) c[k] = scale * pw[k] * ms / (v[k] * n[k]);
    c[3] = ms;
  } else {   // a clamped factor: MS = 0 as in TF; the gradient (0 * inf there) is defined as 0 for this image and channel
    c[0] = c[1] = c[2] = c[3] = 0.f;
  }
}

__global__ __launch_bounds__(NTHREADS) void msssim_total_kernel(MsArgs a, float* loss_out) {
  __shared__ float red[NTHREADS];
  const int tid = threadIdx.x, n = a.B * 3;
  float total = 0.f;
  for (int s = 0; s < a.n_src; ++s) {
    float v = 0.f;
    for (int i = tid; i < n; i += NTHREADS) v += 1.f - a.coef[((long)s * n + i) * 4 + 3];
    red[tid] = v;
    __syncthreads();
    for (int o = NTHREADS / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    total += a.src_w[s] * (red[0] / (float)n);
    __syncthreads();
  }
  if (tid == 0) loss_out[0] += total;
}

// ---------------------------------------------------------------------------------------------------------------- tracked values
// ms_out[s * B + b] = MS of source s, image b: the mean over the channels of what msssim_coef_kernel left (fixed order)
__global__ __launch_bounds__(64) void msssim_values_kernel(MsArgs a, float* __restrict__ ms_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_src * a.B) return;
  const float* c = a.coef + (long)i * 3 * 4;
  ms_out[i] = ((c[3] + c[7]) + c[11]) / 3.f;
}

// ---------------------------------------------------------------------------------------------------------------- backward
__device__ __forceinline__ void add_to(float* p, long o, float v) {
  if (p) p[o] += v;
}
__device__ __forceinline__ void route_comb(const MsArgs& a, int k, long pix, int ch, float g) {
  const int fc = a.comb[k][0], fd = a.comb[k][1], fi = a.comb[k][2];
  float c = feat_at<false>(a, fc, pix, ch), d = feat_at<false>(a, fd, pix, ch), i = feat_at<false>(a, fi, pix, ch);
  add_to(a.dpred[fc], pix * 3 + ch, g * (d + i));
  add_to(a.dpred[fd], pix * 3 + ch, g * c);
  add_to(a.dpred[fi], pix * 3 + ch, g * c);
}

// sources [s_first, s_first + gridDim.z) -- at level 0 one launch per kind, so that no two workgroups of a launch add into the same dpred
template <int K> __global__ __launch_bounds__(NTHREADS) void msssim_bwd_kernel(MsArgs a, int s_first, const dd_grad_scale grad_scale) {
  __shared__ float sx[BIN][BIN + 1], sy[BIN][BIN + 1];
  __shared__ float4 R[BIN][BP];          // row-pass maps; reused as the transposed row pass [BP][T]
  __shared__ float4 A[BP][BP + 1];       // (a, b, c) = coefficient * d value / d (mx, sxy, s2) at the valid positions
  const Level l = level_of(a.H, a.W, K);
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / l.btx, tx = blockIdx.x % l.btx;
  const int b = blockIdx.y / 3, ch = blockIdx.y % 3, s = s_first + blockIdx.z;
  const int r0 = ty * T - HALO, c0 = tx * T - HALO;      // plane coordinates of local (0, 0)
  const float coef = grad_scale.get() * a.coef[(((long)s * a.B + b) * 3 + ch) * 4 + K];
  for (int i = tid; i < BIN * BIN; i += NTHREADS) {
    int r = i / BIN, c = i % BIN;
    load_xy<K>(a, l, s, b, ch, r0 + r, c0 + c, sx[r][c], sy[r][c]);
  }
  __syncthreads();
  for (int i = tid; i < BIN * BP; i += NTHREADS) {   // row pass at the BP position columns
    int r = i / BP, c = i % BP;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t), x = sx[r][c + t], y = sy[r][c + t];
      m.x += g * x, m.y += g * y, m.z += g * (x * y), m.w += g * (x * x + y * y);
    }
    R[r][c] = m;
  }
  __syncthreads();
  for (int i = tid; i < BP * BP; i += NTHREADS) {   // column pass + pointwise partial derivatives
    int r = i / BP, c = i % BP;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t);
      float4 v = R[r + t][c];
      m.x += g * v.x, m.y += g * v.y, m.z += g * v.z, m.w += g * v.w;
    }
    float4 d = {0.f, 0.f, 0.f, 0.f};
    const int pr = r0 + r, pc = c0 + c;
    if (pr >= 0 && pc >= 0 && pr < l.h - HALO && pc < l.w - HALO) {
      float cs, lum, D, Bq;
      ssim_point(m, cs, lum, D, Bq);
      float dcs_mx = (2.f * m.x * cs - 2.f * m.y) / D, dcs_sxy = 2.f / D, dcs_s2 = -cs / D;
      if (K < 2) {
        d.x = coef * dcs_mx, d.y = coef * dcs_sxy, d.z = coef * dcs_s2;
      } else {
        float dlum_mx = (2.f * m.y - 2.f * m.x * lum) / Bq;
        d.x = coef * (cs * dlum_mx + lum * dcs_mx), d.y = coef * (lum * dcs_sxy), d.z = coef * (lum * dcs_s2);
      }
    }
    A[r][c] = d;
  }
  __syncthreads();
  float4(*Tr)[T] = reinterpret_cast<float4(*)[T]>(&R[0][0]);
  for (int i = tid; i < BP * T; i += NTHREADS) {   // transposed row pass: pixel column j collects positions j - t
    int r = i / T, j = i % T;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t);
      float4 v = A[r][j + HALO - t];
      m.x += g * v.x, m.y += g * v.y, m.z += g * v.z;
    }
    Tr[r][j] = m;
  }
  __syncthreads();
  {   // transposed column pass: one pixel per thread
    int i = tid / T, j = tid % T;
    float4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FS; ++t) {
      float g = gauss(t);
      float4 v = Tr[i + HALO - t][j];
      m.x += g * v.x, m.y += g * v.y, m.z += g * v.z;
    }
    const int r = r0 + HALO + i, c = c0 + HALO + j;
    if (r < l.h && c < l.w) {
      float g = m.x + sy[i + HALO][j + HALO] * m.y + 2.f * sx[i + HALO][j + HALO] * m.z;
      const long plane = ((long)s * a.B + b) * 3 + ch;
      if (K < 2) {   // the coarser level's gradient through the 2x2 average pool: a quarter to each pixel
        const int hn = l.h >> 1, wn = l.w >> 1;
        g += 0.25f * a.grad[K][plane * hn * wn + (long)(r >> 1) * wn + (c >> 1)];
      }
      if (K > 0) {
        a.grad[K - 1][plane * l.h * l.w + (long)r * l.w + c] = g;
      } else {
        const long pix = ((long)b * l.h + r) * l.w + c;
        const int kind = a.src_kind[s], idx = a.src_idx[s];
        if (kind == 0) {
          add_to(a.dpred[idx], pix * 3 + ch, g);
        } else if (kind == 1) {
          route_comb(a, idx, pix, ch, g);
        } else {
          for (int q = 0; q < a.n_img_comb; ++q) route_comb(a, a.img_comb[q], pix, ch, g);
          for (int q = 0; q < a.n_img_feat; ++q) add_to(a.dpred[a.img_feat[q]], pix * 3 + ch, g);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
inline long align64(long n) { return (n + 63) & ~63L; }

struct Layout {
  long pool[2], grad[2], partial, coef, total;
};
Layout layout_of(int B, int H, int W, int S) {
  Layout L;
  long o = 0, planes = (long)S * B * 3, nt = 0;
  for (int k = 0; k < 3; ++k) {
    Level l = level_of(H, W, k);
    nt += l.ntx * l.nty;
  }
  for (int k = 1; k <= 2; ++k) {
    Level l = level_of(H, W, k);
    L.pool[k - 1] = o, o += align64(planes * 2 * l.h * l.w);
    L.grad[k - 1] = o, o += align64(planes * l.h * l.w);
  }
  L.partial = o, o += align64(planes * nt * 2);
  L.coef = o, o += align64(planes * 4);
  L.total = o;
  return L;
}

int check_shape(int B, int H, int W) {
  DD_REQUIRE(B > 0 && H > 0 && W > 0, "dd_loss_msssim: B, H, W must be positive (got %d, %d, %d)", B, H, W);
  DD_REQUIRE(H % 4 == 0 && W % 4 == 0, "dd_loss_msssim: H and W must be multiples of 4 (got %d x %d): odd levels would need TF's symmetric pad", H, W);
  DD_REQUIRE(H / 4 >= FS && W / 4 >= FS, "dd_loss_msssim: the coarsest of the 3 levels (%d x %d) is smaller than the 11 x 11 filter", H / 4, W / 4);
  DD_REQUIRE((long)B * 3 <= 65535, "dd_loss_msssim: B * 3 exceeds the grid limit (B = %d)", B);
  return 0;
}

// the device argument block; also validates the descriptor.  kinds[] = number of sources per kind.
int make_args(const dd_loss_msssim_desc* d, int B, int H, int W, float* scratch, MsArgs& a, int kinds[3]) {
  DD_REQUIRE(d != nullptr && scratch != nullptr, "dd_loss_msssim: null descriptor / scratch");
  if (check_shape(B, H, W)) return DD_ERR_INVALID;
  DD_REQUIRE(d->n_features >= 0 && d->n_features <= DD_MAX_FEATURES && d->n_combined >= 0 && d->n_combined <= DD_MAX_COMBINED,
             "dd_loss_msssim: n_features / n_combined out of range");
  DD_REQUIRE(d->n_image_combined >= 0 && d->n_image_combined <= DD_MAX_COMBINED && d->n_image_features >= 0 &&
                 d->n_image_features <= DD_MAX_FEATURES, "dd_loss_msssim: image member counts out of range");
  a = MsArgs{};
  bool used[DD_MAX_FEATURES] = {};
  kinds[0] = kinds[1] = kinds[2] = 0;
  int n = 0;
  for (int f = 0; f < d->n_features; ++f) {
    a.pred[f] = d->pred[f], a.target[f] = d->target[f], a.dpred[f] = d->dpred[f];
    a.pred_ld[f] = d->pred_ld[f], a.target_ld[f] = d->target_ld[f];
    DD_REQUIRE(d->ssim_weight[f] >= 0.f, "dd_loss_msssim: negative weight");
    if (d->ssim_weight[f] > 0.f) {
      a.src_kind[n] = 0, a.src_idx[n] = f, a.src_w[n] = d->ssim_weight[f], ++n, ++kinds[0];
      used[f] = true;
    }
  }
  for (int k = 0; k < d->n_combined; ++k) {
    for (int c = 0; c < 3; ++c) {
      a.comb[k][c] = d->comb[k][c];
      DD_REQUIRE(d->comb[k][c] >= 0 && d->comb[k][c] < d->n_features, "dd_loss_msssim: comb[%d][%d] is not a feature index", k, c);
    }
    DD_REQUIRE(d->comb[k][0] != d->comb[k][1] && d->comb[k][0] != d->comb[k][2] && d->comb[k][1] != d->comb[k][2],
               "dd_loss_msssim: comb[%d] names one feature twice", k);
    DD_REQUIRE(d->comb_ssim_weight[k] >= 0.f, "dd_loss_msssim: negative weight");
    if (d->comb_ssim_weight[k] > 0.f) {
      a.src_kind[n] = 1, a.src_idx[n] = k, a.src_w[n] = d->comb_ssim_weight[k], ++n, ++kinds[1];
      for (int c = 0; c < 3; ++c) used[d->comb[k][c]] = true;
    }
  }
  // the level-0 backward of one kind is one launch whose workgroups add into dpred without atomics: its sources must not share a feature
  int owner[DD_MAX_FEATURES];
  for (int f = 0; f < DD_MAX_FEATURES; ++f) owner[f] = -1;
  for (int k = 0; k < d->n_combined; ++k)
    if (d->comb_ssim_weight[k] > 0.f)
      for (int c = 0; c < 3; ++c) {
        DD_REQUIRE(owner[d->comb[k][c]] < 0, "dd_loss_msssim: feature %d is a member of two combined sources", d->comb[k][c]);
        owner[d->comb[k][c]] = k;
      }
  DD_REQUIRE(d->image_ssim_weight >= 0.f, "dd_loss_msssim: negative weight");
  a.n_img_comb = d->n_image_combined, a.n_img_feat = d->n_image_features;
  if (d->image_ssim_weight > 0.f) {
    DD_REQUIRE(d->n_image_combined + d->n_image_features > 0, "dd_loss_msssim: image weight without image members");
    bool member[DD_MAX_FEATURES] = {};
    for (int i = 0; i < d->n_image_combined; ++i) {
      int k = d->image_combined[i];
      DD_REQUIRE(k >= 0 && k < d->n_combined, "dd_loss_msssim: image_combined[%d] is not a combined index", i);
      a.img_comb[i] = k;
      for (int c = 0; c < 3; ++c) {
        DD_REQUIRE(!member[d->comb[k][c]], "dd_loss_msssim: feature %d enters the image twice", d->comb[k][c]);
        member[d->comb[k][c]] = used[d->comb[k][c]] = true;
      }
    }
    for (int i = 0; i < d->n_image_features; ++i) {
      int f = d->image_features[i];
      DD_REQUIRE(f >= 0 && f < d->n_features, "dd_loss_msssim: image_features[%d] is not a feature index", i);
      DD_REQUIRE(!member[f], "dd_loss_msssim: feature %d enters the image twice", f);
      member[f] = used[f] = true;
      a.img_feat[i] = f;
    }
    a.src_kind[n] = 2, a.src_idx[n] = 0, a.src_w[n] = d->image_ssim_weight, ++n, ++kinds[2];
  } else {
    a.n_img_comb = a.n_img_feat = 0;
  }
  DD_REQUIRE(n > 0, "dd_loss_msssim: no source has a positive ms_ssim weight");
  for (int f = 0; f < d->n_features; ++f) {
    if (!used[f]) continue;
    DD_REQUIRE(d->pred[f] != nullptr && d->target[f] != nullptr, "dd_loss_msssim: feature %d is used but has a null pred / target", f);
    DD_REQUIRE(d->nch[f] == 3, "dd_loss_msssim: feature %d has %d channels; the term needs 3 (Training.py:187-190)", f, d->nch[f]);
    DD_REQUIRE(d->pred_ld[f] >= 3 && d->target_ld[f] >= 3, "dd_loss_msssim: feature %d has a pixel stride below 3", f);
  }
  a.n_src = n, a.B = B, a.H = H, a.W = W;
  Layout L = layout_of(B, H, W, n);
  for (int k = 0; k < 2; ++k) a.pool[k] = scratch + L.pool[k], a.grad[k] = scratch + L.grad[k];
  a.partial = scratch + L.partial, a.coef = scratch + L.coef;
  return 0;
}

template <int K> int launch_fwd(const MsArgs& a, hipStream_t st) {
  Level l = level_of(a.H, a.W, K);
  hipLaunchKernelGGL(msssim_fwd_kernel<K>, dim3(l.ntx * l.nty, a.B * 3, a.n_src), dim3(NTHREADS), 0, st, a);
  DD_LAUNCH_CHECK();
  return 0;
}
template <int K> int launch_bwd(const MsArgs& a, int s_first, int count, dd_grad_scale grad_scale, hipStream_t st) {
  if (count == 0) return 0;
  Level l = level_of(a.H, a.W, K);
  hipLaunchKernelGGL(msssim_bwd_kernel<K>, dim3(l.btx * l.bty, a.B * 3, count), dim3(NTHREADS), 0, st, a, s_first, grad_scale);
  DD_LAUNCH_CHECK();
  return 0;
}

int bwd_launches(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, dd_grad_scale grad_scale, dd_stream stream) {
  MsArgs a;
  int kinds[3];
  if (int e = make_args(desc, B, H, W, scratch, a, kinds)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (int e = launch_bwd<2>(a, 0, a.n_src, grad_scale, st)) return e;
  if (int e = launch_bwd<1>(a, 0, a.n_src, grad_scale, st)) return e;
  // sources are listed by kind (features, combined, image): one launch per kind, in stream order
  if (int e = launch_bwd<0>(a, 0, kinds[0], grad_scale, st)) return e;
  if (int e = launch_bwd<0>(a, kinds[0], kinds[1], grad_scale, st)) return e;
  if (int e = launch_bwd<0>(a, kinds[0] + kinds[1], kinds[2], grad_scale, st)) return e;
  return 0;
}

}  // namespace

extern "C" long dd_loss_msssim_scratch_bytes(int B, int H, int W, int n_sources) {
  if (check_shape(B, H, W)) return DD_ERR_INVALID;
  if (n_sources <= 0 || n_sources > MAX_SRC) {
    dd_set_error("dd_loss_msssim_scratch_bytes: n_sources must be in 1 .. %d (got %d)", MAX_SRC, n_sources);
    return DD_ERR_INVALID;
  }
  return layout_of(B, H, W, n_sources).total * (long)sizeof(float);
}

extern "C" int dd_loss_msssim_fwd(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float* loss_out, dd_stream stream) {
  DD_REQUIRE(loss_out != nullptr, "dd_loss_msssim_fwd: null loss_out");
  MsArgs a;
  int kinds[3];
  if (int e = make_args(desc, B, H, W, scratch, a, kinds)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (int e = launch_fwd<0>(a, st)) return e;
  if (int e = launch_fwd<1>(a, st)) return e;
  if (int e = launch_fwd<2>(a, st)) return e;
  hipLaunchKernelGGL(msssim_coef_kernel, dim3((a.n_src * B * 3 + 63) / 64), dim3(64), 0, st, a);
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(msssim_total_kernel, dim3(1), dim3(NTHREADS), 0, st, a, loss_out);
  DD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dd_loss_msssim_values(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float* ms_out, dd_stream stream) {
  DD_REQUIRE(ms_out != nullptr, "dd_loss_msssim_values: null ms_out");
  MsArgs a;
  int kinds[3];
  if (int e = make_args(desc, B, H, W, scratch, a, kinds)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (int e = launch_fwd<0>(a, st)) return e;
  if (int e = launch_fwd<1>(a, st)) return e;
  if (int e = launch_fwd<2>(a, st)) return e;
  hipLaunchKernelGGL(msssim_coef_kernel, dim3((a.n_src * B * 3 + 63) / 64), dim3(64), 0, st, a);
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(msssim_values_kernel, dim3((a.n_src * B + 63) / 64), dim3(64), 0, st, a, ms_out);
  DD_LAUNCH_CHECK();
  return 0;
}

extern "C" int dd_loss_msssim_bwd(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float grad_scale, dd_stream stream) {
  return bwd_launches(desc, B, H, W, scratch, dd_grad_scale{grad_scale, nullptr}, stream);
}
// the same launches with the factor read from device memory when the kernels run (dynamic loss scaling, csrc/dd_loss_scale.hip)
extern "C" int dd_loss_msssim_bwd_dscale(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, const float* grad_scale_dev,
                                         dd_stream stream) {
  DD_REQUIRE(grad_scale_dev != nullptr, "dd_loss_msssim_bwd_dscale: null grad_scale_dev");
  return bwd_launches(desc, B, H, W, scratch, dd_grad_scale{1.f, grad_scale_dev}, stream);
}
