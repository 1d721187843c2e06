// Temporal stabilisation of a denoised frame (include/dd_hip.h: dd_temporal_stabilize): every pass of the frame just denoised is blended with
// the stabilised previous frame, fetched along the motion vectors and clamped to what the 3 x 3 neighbourhood of the current frame allows.
//
//   temporal_stabilize_kernel : a workgroup of 256 threads owns TT x TT pixels, one per thread (a wave's lanes are four rows of 16 neighbours; with
//                               four pixels per thread on a 32 x 32 tile the taps and the staged values of a pass did not fit 128 registers).
//                               ONCE per pixel: the previous position from the motion pass, the offscreen test,
//                               the tap index and the weights (csrc/dd_frame_common.h: dd_motion_previous, the function the sequence scorer
//                               compiles too), and the guide test at the nearest previous pixel.  Then the loop over the passes, per pass:
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
#include "dd_frame_common.h"

namespace {

constexpr int TT = DD_TEMPORAL_TILE;           // pixels per workgroup side
constexpr int TP = TT + 2;                     // patch side: the tile and a one-pixel halo
constexpr int TTHREADS = FRAME_THREADS;
constexpr int TWAVES = FRAME_WAVES;
constexpr int TU = 5, TD = 3;                  // counts and sums of a dd_temporal_record
static_assert(TT * TT == TTHREADS && (TT & (TT - 1)) == 0 && TWAVES == 4, "a thread owns the pixel (tid / TT, tid % TT) of the tile");
static_assert(frame_record_is<dd_temporal_record, TU, TD, false>(offsetof(dd_temporal_record, pixels_offscreen), offsetof(dd_temporal_record, change),
                                                                 sizeof(dd_temporal_record)), "dd_temporal_record: five uint64 counts, three double sums");

constexpr unsigned ST_INSIDE = 8u, ST_GUIDE = 16u;      // next to the DD_MOTION_* bits: the thread's pixel lies in the image; a guide rejected it

struct TemporalArgs {
  dd_temporal_pass pass[DD_TEMPORAL_MAX_PASSES];
  dd_temporal_guide guide[DD_TEMPORAL_MAX_GUIDES];
  const float* motion;
  int motion_ld, n_passes, n_guides;
  float sx, sy, alpha, gamma;
};

// One pass of the tile.  tile: the LDS patch; wave_d / wave_u: this pass's buffers of the per-wave sums.
template <int NCH>
__device__ __forceinline__ void stabilize_pass(const dd_temporal_pass& P, const TemporalArgs& a, const dd_motion_position& s, int H, int W, float* __restrict__ tile,
                                               double (*wave_d)[TWAVES], unsigned (*wave_u)[TWAVES]) {
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
  float t[4][NCH];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < NCH; ++c) t[j][c] = 0.f;
  if ((s.bits & (ST_INSIDE | DD_MOTION_OFFSCREEN | ST_GUIDE)) == ST_INSIDE) {
    const long q = s.q00, dx = (s.bits & DD_MOTION_XSTEP) ? 1 : 0, dy = (s.bits & DD_MOTION_YSTEP) ? W : 0;
    load_pixel<NCH>(P.history, q, P.history_ld, t[0]);
    load_pixel<NCH>(P.history, q + dx, P.history_ld, t[1]);
    load_pixel<NCH>(P.history, q + dy, P.history_ld, t[2]);
    load_pixel<NCH>(P.history, q + dy + dx, P.history_ld, t[3]);
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
  if (s.bits & ST_INSIDE) {
    const int ly = ty + 1, lx = tx + 1;
    const bool candidate = (s.bits & (DD_MOTION_OFFSCREEN | ST_GUIDE)) == 0u;
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
        const float sd = sqrtf(dev * (1.0f / 9.0f)), fx = s.fx, fy = s.fy;
        lo[c] = m - a.gamma * sd;
        hi[c] = m + a.gamma * sd;
        h[c] = (t[0][c] * (1.0f - fx) + t[1][c] * fx) * (1.0f - fy) + (t[2][c] * (1.0f - fx) + t[3][c] * fx) * fy;
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
    store_pixel<NCH>(P.out, (long)(y0 + ty) * W + (x0 + tx), P.out_ld, o);
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
  __shared__ double wave_d[2][TD][TWAVES];          // [pass parity][change | flicker_before | flicker_after]
  __shared__ unsigned wave_u[2][3][TWAVES];         // [pass parity][nonfinite | blended | clamped]
  __shared__ unsigned wave_c[2][TWAVES];            // offscreen | guide: the same for every pass

  const int tid = threadIdx.x, x = blockIdx.x * TT + (tid & (TT - 1)), y = blockIdx.y * TT + tid / TT;
  // ---------------------------------------------------------------------------------------------- once per pixel
  dd_motion_position s;
  s.q00 = 0; s.fx = s.fy = 0.f; s.bits = 0u;
  if (y < H && x < W) {
    s = dd_motion_previous(a.motion, a.motion_ld, a.sx, a.sy, x, y, H, W);
    s.bits |= ST_INSIDE;
    if (!(s.bits & DD_MOTION_OFFSCREEN)) {
      const int nx = min(max((int)floorf(s.px + 0.5f), 0), W - 1), ny = min(max((int)floorf(s.py + 0.5f), 0), H - 1);
      bool rejected = false;
      for (int g = 0; g < a.n_guides; ++g) {
        const dd_temporal_guide G = a.guide[g];
        const float* __restrict__ gc = G.current + ((long)y * W + x) * G.current_ld;
        const float* __restrict__ gp = G.previous + ((long)ny * W + nx) * G.previous_ld;
        for (int c = 0; c < G.nch; ++c) rejected = rejected || !(fabsf(gc[c] - gp[c]) <= G.tolerance);      // (a NaN difference rejects)
      }
      if (rejected) s.bits |= ST_GUIDE;
    }
  }
  const unsigned n_offscreen = wave_sum((s.bits & (ST_INSIDE | DD_MOTION_OFFSCREEN)) == (ST_INSIDE | DD_MOTION_OFFSCREEN) ? 1u : 0u);
  const unsigned n_guide = wave_sum((s.bits & ST_GUIDE) ? 1u : 0u);
  if ((tid & 63) == 0) { wave_c[0][tid >> 6] = n_offscreen; wave_c[1][tid >> 6] = n_guide; }

  // ---------------------------------------------------------------------------------------------- the passes
  const long block = (long)blockIdx.y * gridDim.x + blockIdx.x, blocks = (long)gridDim.x * gridDim.y;
  auto write_partial = [&](int p) {      // thread 0, behind a barrier that follows pass p's sums
    const int b = p & 1;
    FrameSums<TU, TD, false> r;
    frame_wave_partial<TU, TD>(r.u, r.d, {wave_c[0], wave_c[1], wave_u[b][0], wave_u[b][1], wave_u[b][2]}, wave_d[b]);
    reinterpret_cast<FrameSums<TU, TD, false>*>(partials)[(long)p * blocks + block] = r;
  };
#pragma nounroll      // (also: not peeled.  Peeling the first pass, where p > 0 is known, doubles the code and costs two registers)
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

// records[pass] = the sum of the pass's `tiles` partial records (csrc/dd_frame_common.h: frame_finalize)
__global__ __launch_bounds__(TTHREADS) void temporal_finalize_kernel(const dd_temporal_record* __restrict__ partials, int tiles,
                                                                     dd_temporal_record* __restrict__ records) {
  frame_finalize<dd_temporal_record, TU, TD, false>(partials, tiles, records);
}

}  // namespace

extern "C" long dd_temporal_scratch_bytes(int n_passes, int H, int W) {
  return frame_scratch_bytes<TT, dd_temporal_record>("dd_temporal_scratch_bytes", "n_passes", n_passes, DD_TEMPORAL_MAX_PASSES, H, W);
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
  if (int rc = frame_check_motion<TT>("dd_temporal_stabilize", H, W, motion, motion_ld, sx, sy)) return rc;
  DD_REQUIRE(alpha >= 0.f && alpha <= 1.f, "dd_temporal_stabilize: alpha = %g (0 .. 1)", (double)alpha);
  DD_REQUIRE(gamma >= 0.f && isfinite(gamma), "dd_temporal_stabilize: gamma = %g (finite, not negative)", (double)gamma);
  if (int rc = frame_check_buffers("dd_temporal_stabilize", records, scratch)) return rc;
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
  const int tx = (int)frame_tiles_of<TT>(W), ty = (int)frame_tiles_of<TT>(H);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(temporal_stabilize_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(TTHREADS), 0, s, a, H, W, reinterpret_cast<dd_temporal_record*>(scratch));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(temporal_finalize_kernel, dim3((unsigned)n_passes), dim3(TTHREADS), 0, s, reinterpret_cast<const dd_temporal_record*>(scratch), tx * ty,
                     reinterpret_cast<dd_temporal_record*>(records));
  DD_LAUNCH_CHECK();
  return DD_OK;
}
