// Temporal stabilisation of a denoised frame (include/dd_hip.h: dd_temporal_stabilize): every pass of the frame just denoised is blended with
// the stabilised previous frame, fetched along the motion vectors and clamped to what the 3 x 3 neighbourhood of the current frame allows.
//
//   temporal_stabilize_kernel : a workgroup of 256 threads owns TT x TT pixels, one per thread (a wave's lanes are four rows of 16 neighbours; with
//                               four pixels per thread on a 32 x 32 tile the taps and the staged values of a pass did not fit 128 registers).
//                               ONCE per pixel: the previous position from the motion pass, the offscreen test,
//                               the four tap indices and weights, and the guide test at the nearest previous pixel.  Then the loop over the
//                               passes, per pass:
//                               stage     the (TT + 2)^2 patch of `current` (coordinates clamped to the image) from HBM into LDS, consecutive
//                                         lanes consecutive floats; every load of a thread is issued before the first is stored, and so are
//                                         the loads of its four history taps per pixel (straight from global memory: neighbouring lanes
//                                         share lines; 12-byte loads where ld == nch == 3)
//                               blend     per channel the nine window values from LDS (lane stride nch floats: no bank conflict), their mean
//                                         and standard deviation, the bilinear sample, clamp, blend, one store per pixel
//                               sums      fp32 terms added in double per thread, a shuffle tree inside a wave, the four waves in order -> one
//                                         partial record per (pass, workgroup), written by thread 0 while the next pass is staged
//   temporal_finalize_kernel  : one workgroup per pass adds its partial records in a fixed order (integers exactly, the rest in double).
// No atomics at all: two runs give the same bits; a pass's record and output do not depend on its index or on its neighbours in the call.
// The standard deviation is taken as sqrt(mean((v - m)^2)): the same quantity as sqrt(E[v^2] - m^2) without its cancellation, which in fp32
// would leave a deviation of 3e-4 on a flat window of ones.
#include <limits.h>
#include <math.h>

#include "dd_common.h"

namespace {

constexpr int TT = DD_TEMPORAL_TILE;           // pixels per workgroup side
constexpr int TP = TT + 2;                     // patch side: the tile and a one-pixel halo
constexpr int TTHREADS = 256;
constexpr int TROWS = TTHREADS / TT;           // tile rows one sweep of the threads covers
constexpr int TK = TT / TROWS;                 // pixels per thread
static_assert(TROWS * TT == TTHREADS && TK * TROWS == TT && (TT & (TT - 1)) == 0, "a thread owns column tid % TT and the rows tid / TT + TROWS k");

constexpr unsigned ST_INSIDE = 1u, ST_OFFSCREEN = 2u, ST_GUIDE = 4u, ST_XSTEP = 8u, ST_YSTEP = 16u;

struct TemporalArgs {
  dd_temporal_pass pass[DD_TEMPORAL_MAX_PASSES];
  dd_temporal_guide guide[DD_TEMPORAL_MAX_GUIDES];
  const float* motion;
  int motion_ld, n_passes, n_guides;
  float sx, sy, alpha, gamma;
};

struct __attribute__((packed, aligned(4))) Float3 { float x, y, z; };

__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <int NCH>
__device__ __forceinline__ void load_pixel(const float* __restrict__ base, long q, int ld, float (&v)[NCH]) {
  if constexpr (NCH == 3) {
    if (ld == 3) {
      const Float3 w = *reinterpret_cast<const Float3*>(base + 3 * q);
      v[0] = w.x; v[1] = w.y; v[2] = w.z;
      return;
    }
  }
  const float* __restrict__ s = base + q * ld;
#pragma unroll
  for (int c = 0; c < NCH; ++c) v[c] = s[c];
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

struct PixelState {
  int q00[TK];           // pixel index of the tap (y0, x0)
  float fx[TK], fy[TK];
  unsigned st[TK];       // ST_* bits
};

// One pass of the tile.  tile: the LDS patch; wave_d / wave_u: this pass's buffers of the per-wave sums.
template <int NCH>
__device__ __forceinline__ void stabilize_pass(const dd_temporal_pass& P, const TemporalArgs& a, const PixelState& s, int H, int W, float* __restrict__ tile,
                                               double (*wave_d)[TTHREADS / 64], unsigned (*wave_u)[TTHREADS / 64]) {
#pragma clang fp contract(off)
  constexpr int RS = TP * NCH, E = TP * RS, ITER = (E + TTHREADS - 1) / TTHREADS;
  const int tid = threadIdx.x, tx = tid & (TT - 1), ty = tid / TT, x0 = blockIdx.x * TT, y0 = blockIdx.y * TT;
  // ---------------------------------------------------------------------------------------------- stage the patch, fetch the taps
  float sv[ITER];
#pragma unroll
  for (int i = 0; i < ITER; ++i) {
    const int e = tid + i * TTHREADS;
    sv[i] = 0.f;
    if (e < E) {
      const int r = e / RS, rem = e - r * RS, pp = rem / NCH, c = rem - pp * NCH;
      const int y = min(max(y0 - 1 + r, 0), H - 1), x = min(max(x0 - 1 + pp, 0), W - 1);
      sv[i] = P.current[((long)y * W + x) * P.current_ld + c];
    }
  }
  float t[TK][4][NCH];
#pragma unroll
  for (int k = 0; k < TK; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < NCH; ++c) t[k][j][c] = 0.f;
    if ((s.st[k] & (ST_INSIDE | ST_OFFSCREEN | ST_GUIDE)) == ST_INSIDE) {
      const long q = s.q00[k], dx = (s.st[k] & ST_XSTEP) ? 1 : 0, dy = (s.st[k] & ST_YSTEP) ? W : 0;
      load_pixel<NCH>(P.history, q, P.history_ld, t[k][0]);
      load_pixel<NCH>(P.history, q + dx, P.history_ld, t[k][1]);
      load_pixel<NCH>(P.history, q + dy, P.history_ld, t[k][2]);
      load_pixel<NCH>(P.history, q + dy + dx, P.history_ld, t[k][3]);
    }
  }
#pragma unroll
  for (int i = 0; i < ITER; ++i) {
    const int e = tid + i * TTHREADS;
    if (e < E) tile[e] = sv[i];
  }
  __syncthreads();

  // ---------------------------------------------------------------------------------------------- blend
  double change = 0.0, before = 0.0, after = 0.0;
  unsigned n_nonfinite = 0u, n_blended = 0u, n_clamped = 0u;
#pragma unroll
  for (int k = 0; k < TK; ++k) {
    if (!(s.st[k] & ST_INSIDE)) continue;
    const int ly = ty + k * TROWS + 1, lx = tx + 1;
    const bool candidate = (s.st[k] & (ST_OFFSCREEN | ST_GUIDE)) == 0u;
    float cur[NCH], h[NCH], lo[NCH], hi[NCH];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      cur[c] = tile[ly * RS + lx * NCH + c];
      h[c] = lo[c] = hi[c] = 0.f;
      if (candidate) {
        float v[9], sum = 0.f, dev = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          v[j] = tile[(ly + j / 3 - 1) * RS + (lx + j % 3 - 1) * NCH + c];
          bad = bad || nonfinite(v[j]);
          sum += v[j];
        }
        const float m = sum * (1.0f / 9.0f);
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const float d = v[j] - m;
          dev += d * d;
        }
        const float sd = sqrtf(dev * (1.0f / 9.0f)), fx = s.fx[k], fy = s.fy[k];
        lo[c] = m - a.gamma * sd;
        hi[c] = m + a.gamma * sd;
        h[c] = (t[k][0][c] * (1.0f - fx) + t[k][1][c] * fx) * (1.0f - fy) + (t[k][2][c] * (1.0f - fx) + t[k][3][c] * fx) * fy;
        bad = bad || nonfinite(h[c]);
      }
    }
    const bool blended = candidate && !bad;
    n_nonfinite += (candidate && bad) ? 1u : 0u;
    n_blended += blended ? 1u : 0u;
    float o[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      o[c] = cur[c];
      if (blended) {
        const float hc = fminf(fmaxf(h[c], lo[c]), hi[c]);
        n_clamped += (h[c] < lo[c] || h[c] > hi[c]) ? 1u : 0u;
        o[c] = cur[c] + a.alpha * (hc - cur[c]);
        change += (double)fabsf(o[c] - cur[c]);
        before += (double)fabsf(cur[c] - h[c]);
        after += (double)fabsf(o[c] - h[c]);
      }
    }
    const long q = (long)(y0 + ty + k * TROWS) * W + (x0 + tx);
    bool stored = false;
    if constexpr (NCH == 3) {
      if (P.out_ld == 3) {
        Float3 w;
        w.x = o[0]; w.y = o[1]; w.z = o[2];
        *reinterpret_cast<Float3*>(P.out + 3 * q) = w;
        stored = true;
      }
    }
    if (!stored) {
      float* __restrict__ d = P.out + q * P.out_ld;
#pragma unroll
      for (int c = 0; c < NCH; ++c) d[c] = o[c];
    }
  }
  change = wave_sum(change); before = wave_sum(before); after = wave_sum(after);
  n_nonfinite = wave_sum(n_nonfinite); n_blended = wave_sum(n_blended); n_clamped = wave_sum(n_clamped);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    wave_d[0][w] = change; wave_d[1][w] = before; wave_d[2][w] = after;
    wave_u[0][w] = n_nonfinite; wave_u[1][w] = n_blended; wave_u[2][w] = n_clamped;
  }
}

__global__ __launch_bounds__(TTHREADS) void temporal_stabilize_kernel(const TemporalArgs a, int H, int W, dd_temporal_record* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ float tile[TP * TP * 3];
  __shared__ double wave_d[2][3][TTHREADS / 64];       // [pass parity][change | flicker_before | flicker_after]
  __shared__ unsigned wave_u[2][3][TTHREADS / 64];     // [pass parity][nonfinite | blended | clamped]
  __shared__ unsigned wave_c[2][TTHREADS / 64];        // offscreen | guide: the same for every pass

  const int tid = threadIdx.x, tx = tid & (TT - 1), ty = tid / TT, x0 = blockIdx.x * TT, y0 = blockIdx.y * TT;
  // ---------------------------------------------------------------------------------------------- once per pixel
  PixelState s;
  unsigned n_offscreen = 0u, n_guide = 0u;
#pragma unroll
  for (int k = 0; k < TK; ++k) {
    const int y = y0 + ty + k * TROWS, x = x0 + tx;
    s.q00[k] = 0; s.fx[k] = s.fy[k] = 0.f; s.st[k] = 0u;
    if (y >= H || x >= W) continue;
    const float* __restrict__ mv = a.motion + ((long)y * W + x) * a.motion_ld;
    const float px = (float)x + a.sx * mv[0], py = (float)y + a.sy * mv[1];
    if (!(px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1))) {      // (NaN and both infinities fail a comparison)
      s.st[k] = ST_INSIDE | ST_OFFSCREEN;
      ++n_offscreen;
      continue;
    }
    const float xf = floorf(px), yf = floorf(py);
    const int ix = min(max((int)xf, 0), W - 1), iy = min(max((int)yf, 0), H - 1);
    s.fx[k] = px - xf; s.fy[k] = py - yf;
    s.q00[k] = iy * W + ix;
    unsigned st = ST_INSIDE | (ix + 1 <= W - 1 ? ST_XSTEP : 0u) | (iy + 1 <= H - 1 ? ST_YSTEP : 0u);
    const int nx = min(max((int)floorf(px + 0.5f), 0), W - 1), ny = min(max((int)floorf(py + 0.5f), 0), H - 1);
    bool rejected = false;
    for (int g = 0; g < a.n_guides; ++g) {
      const dd_temporal_guide G = a.guide[g];
      const float* __restrict__ gc = G.current + ((long)y * W + x) * G.current_ld;
      const float* __restrict__ gp = G.previous + ((long)ny * W + nx) * G.previous_ld;
      for (int c = 0; c < G.nch; ++c) rejected = rejected || !(fabsf(gc[c] - gp[c]) <= G.tolerance);      // (a NaN difference rejects)
    }
    if (rejected) {
      st |= ST_GUIDE;
      ++n_guide;
    }
    s.st[k] = st;
  }
  n_offscreen = wave_sum(n_offscreen); n_guide = wave_sum(n_guide);
  if ((tid & 63) == 0) { wave_c[0][tid >> 6] = n_offscreen; wave_c[1][tid >> 6] = n_guide; }

  // ---------------------------------------------------------------------------------------------- the passes
  const long block = (long)blockIdx.y * gridDim.x + blockIdx.x, blocks = (long)gridDim.x * gridDim.y;
  auto write_partial = [&](int p) {      // thread 0, behind a barrier that follows pass p's sums
    const int b = p & 1;
    dd_temporal_record r;
    r.pixels_offscreen = wave_c[0][0] + wave_c[0][1] + wave_c[0][2] + wave_c[0][3];
    r.pixels_guide = wave_c[1][0] + wave_c[1][1] + wave_c[1][2] + wave_c[1][3];
    r.pixels_nonfinite = wave_u[b][0][0] + wave_u[b][0][1] + wave_u[b][0][2] + wave_u[b][0][3];
    r.pixels_blended = wave_u[b][1][0] + wave_u[b][1][1] + wave_u[b][1][2] + wave_u[b][1][3];
    r.values_clamped = wave_u[b][2][0] + wave_u[b][2][1] + wave_u[b][2][2] + wave_u[b][2][3];
    r.change = ((wave_d[b][0][0] + wave_d[b][0][1]) + wave_d[b][0][2]) + wave_d[b][0][3];
    r.flicker_before = ((wave_d[b][1][0] + wave_d[b][1][1]) + wave_d[b][1][2]) + wave_d[b][1][3];
    r.flicker_after = ((wave_d[b][2][0] + wave_d[b][2][1]) + wave_d[b][2][2]) + wave_d[b][2][3];
    partials[(long)p * blocks + block] = r;
  };
  for (int p = 0; p < a.n_passes; ++p) {
    __syncthreads();      // the pass before has read `tile` and left its sums (two buffers: pass p + 1 fills the other one)
    if (tid == 0 && p > 0) write_partial(p - 1);
    const dd_temporal_pass P = a.pass[p];
    if (P.nch == 3)
      stabilize_pass<3>(P, a, s, H, W, tile, wave_d[p & 1], wave_u[p & 1]);
    else
      stabilize_pass<1>(P, a, s, H, W, tile, wave_d[p & 1], wave_u[p & 1]);
  }
  __syncthreads();
  if (tid == 0) write_partial(a.n_passes - 1);
}

// records[pass] = the sum of the pass's `tiles` partial records: thread t adds records t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(TTHREADS) void temporal_finalize_kernel(const dd_temporal_record* __restrict__ partials, int tiles,
                                                                     dd_temporal_record* __restrict__ records) {
  __shared__ double sd[3][TTHREADS];
  __shared__ unsigned long long su[5][TTHREADS];
  const int tid = threadIdx.x;
  const dd_temporal_record* __restrict__ p = partials + (long)blockIdx.x * tiles;
  double d[3] = {0.0, 0.0, 0.0};
  unsigned long long u[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
  for (int b = tid; b < tiles; b += TTHREADS) {
    const dd_temporal_record r = p[b];
    u[0] += r.pixels_offscreen; u[1] += r.pixels_guide; u[2] += r.pixels_nonfinite; u[3] += r.pixels_blended; u[4] += r.values_clamped;
    d[0] += r.change; d[1] += r.flicker_before; d[2] += r.flicker_after;
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) sd[m][tid] = d[m];
#pragma unroll
  for (int m = 0; m < 5; ++m) su[m][tid] = u[m];
  __syncthreads();
  for (int half = TTHREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int m = 0; m < 3; ++m) sd[m][tid] += sd[m][tid + half];
#pragma unroll
      for (int m = 0; m < 5; ++m) su[m][tid] += su[m][tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    dd_temporal_record r;
    r.pixels_offscreen = su[0][0]; r.pixels_guide = su[1][0]; r.pixels_nonfinite = su[2][0]; r.pixels_blended = su[3][0]; r.values_clamped = su[4][0];
    r.change = sd[0][0]; r.flicker_before = sd[1][0]; r.flicker_after = sd[2][0];
    records[blockIdx.x] = r;
  }
}

inline long tiles_of(int n) { return ((long)n + TT - 1) / TT; }

}  // namespace

extern "C" long dd_temporal_scratch_bytes(int n_passes, int H, int W) {
  if (n_passes < 1 || n_passes > DD_TEMPORAL_MAX_PASSES || H < 1 || W < 1) {
    dd_set_error("dd_temporal_scratch_bytes: n_passes = %d (1 .. %d), H = %d, W = %d", n_passes, DD_TEMPORAL_MAX_PASSES, H, W);
    return DD_ERR_INVALID;
  }
  return (long)n_passes * tiles_of(H) * tiles_of(W) * (long)sizeof(dd_temporal_record);
}

extern "C" int dd_temporal_stabilize(const dd_temporal_pass* passes, int n_passes, const dd_temporal_guide* guides, int n_guides, int H, int W,
                                     const float* motion, int motion_ld, float sx, float sy, float alpha, float gamma, void* records, void* scratch,
                                     dd_stream stream) {
  static_assert(sizeof(dd_temporal_record) == 64, "dd_temporal_record is 64 bytes (include/dd_hip.h, _lib.TemporalRecord)");
  static_assert(sizeof(dd_temporal_pass) == 40 && sizeof(dd_temporal_guide) == 32, "include/dd_hip.h, _lib.TemporalPass / TemporalGuide");
  DD_REQUIRE(passes, "dd_temporal_stabilize: null pass table");
  DD_REQUIRE(n_passes >= 1 && n_passes <= DD_TEMPORAL_MAX_PASSES, "dd_temporal_stabilize: n_passes = %d (1 .. %d)", n_passes, DD_TEMPORAL_MAX_PASSES);
  DD_REQUIRE(n_guides >= 0 && n_guides <= DD_TEMPORAL_MAX_GUIDES, "dd_temporal_stabilize: n_guides = %d (0 .. %d)", n_guides, DD_TEMPORAL_MAX_GUIDES);
  DD_REQUIRE(n_guides == 0 || guides, "dd_temporal_stabilize: null guide table");
  DD_REQUIRE(H >= 1 && W >= 1, "dd_temporal_stabilize: bad shape %d x %d", H, W);
  DD_REQUIRE((long)H * W <= INT_MAX && H <= (1 << 24) && W <= (1 << 24) && tiles_of(H) <= 65535,
             "dd_temporal_stabilize: %d x %d does not fit a grid or a 32-bit pixel index", H, W);
  DD_REQUIRE(motion && ((uintptr_t)motion & 3) == 0, "dd_temporal_stabilize: motion is null or not 4-byte aligned");
  DD_REQUIRE(motion_ld >= 2, "dd_temporal_stabilize: motion_ld = %d (the pass has two used channels)", motion_ld);
  DD_REQUIRE(isfinite(sx) && isfinite(sy), "dd_temporal_stabilize: the motion scale is not finite");
  DD_REQUIRE(alpha >= 0.f && alpha <= 1.f, "dd_temporal_stabilize: alpha = %g (0 .. 1)", (double)alpha);
  DD_REQUIRE(gamma >= 0.f && isfinite(gamma), "dd_temporal_stabilize: gamma = %g (finite, not negative)", (double)gamma);
  DD_REQUIRE(records && ((uintptr_t)records & 7) == 0, "dd_temporal_stabilize: records is null or not 8-byte aligned");
  DD_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "dd_temporal_stabilize: scratch is null or not 8-byte aligned");
  TemporalArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_passes; ++i) {
    const dd_temporal_pass& p = passes[i];
    DD_REQUIRE(p.current && p.history && p.out, "dd_temporal_stabilize: pass %d has a null current / history / out", i);
    DD_REQUIRE((((uintptr_t)p.current | (uintptr_t)p.history | (uintptr_t)p.out) & 3) == 0, "dd_temporal_stabilize: pass %d is not 4-byte aligned", i);
    DD_REQUIRE(p.nch == 1 || p.nch == 3, "dd_temporal_stabilize: pass %d has %d channels (1 or 3 expected)", i, p.nch);
    DD_REQUIRE(p.current_ld >= p.nch && p.history_ld >= p.nch && p.out_ld >= p.nch, "dd_temporal_stabilize: pass %d has a pixel stride (ld) below its channels", i);
    a.pass[i] = p;
  }
  for (int i = 0; i < n_passes; ++i)
    for (int j = 0; j < n_passes; ++j)
      DD_REQUIRE(passes[i].out != passes[j].current && passes[i].out != passes[j].history,
                 "dd_temporal_stabilize: out of pass %d is current or history of pass %d (neighbours read both: in place is not possible)", i, j);
  for (int g = 0; g < n_guides; ++g) {
    const dd_temporal_guide& q = guides[g];
    DD_REQUIRE(q.current && q.previous, "dd_temporal_stabilize: guide %d has a null current / previous", g);
    DD_REQUIRE((((uintptr_t)q.current | (uintptr_t)q.previous) & 3) == 0, "dd_temporal_stabilize: guide %d is not 4-byte aligned", g);
    DD_REQUIRE(q.nch == 1 || q.nch == 3, "dd_temporal_stabilize: guide %d has %d channels (1 or 3 expected)", g, q.nch);
    DD_REQUIRE(q.current_ld >= q.nch && q.previous_ld >= q.nch, "dd_temporal_stabilize: guide %d has a pixel stride (ld) below its channels", g);
    DD_REQUIRE(q.tolerance >= 0.f && isfinite(q.tolerance), "dd_temporal_stabilize: guide %d has tolerance %g (finite, not negative)", g, (double)q.tolerance);
    a.guide[g] = q;
  }
  a.motion = motion; a.motion_ld = motion_ld; a.n_passes = n_passes; a.n_guides = n_guides;
  a.sx = sx; a.sy = sy; a.alpha = alpha; a.gamma = gamma;
  const int tx = (int)tiles_of(W), ty = (int)tiles_of(H);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(temporal_stabilize_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(TTHREADS), 0, s, a, H, W, reinterpret_cast<dd_temporal_record*>(scratch));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(temporal_finalize_kernel, dim3((unsigned)n_passes), dim3(TTHREADS), 0, s, reinterpret_cast<const dd_temporal_record*>(scratch), tx * ty,
                     reinterpret_cast<dd_temporal_record*>(records));
  DD_LAUNCH_CHECK();
  return DD_OK;
}
