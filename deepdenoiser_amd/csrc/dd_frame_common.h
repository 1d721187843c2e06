// What the frame-level launches share (dd_quality.hip, dd_temporal.hip, dd_sequence_quality.hip; the first group also dd_nonfinite.hip):
//   values     Float3, nonfinite, load_pixel / store_pixel, the wave reductions
//   motion     where a pixel was in the previous frame (include/dd_hip.h: dd_temporal_stabilize states the rule): ONE function, compiled into
//              the stabiliser and into the sequence scorer, so that the scorer measures exactly what the stabiliser fetched
//   records    a record is NU uint64 counts, then ND double sums, then (dd_quality_record) a float max and a float reserved: the workgroup's
//              partial record from its four waves, and the finalize kernel's body.  Every addition is made in a fixed order: the records of
//              two runs have the same bits.
//   host       the tile count, the scratch size and the argument checks the entry points repeat, under the caller's name
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "dd_common.h"

// ---------------------------------------------------------------------------------------------------------------- values
struct __attribute__((packed, aligned(4))) Float3 { float x, y, z; };

// inf or NaN <=> all eight exponent bits set (on the bits: nothing a fast-math build may fold away)
__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// pixel q of a [.., ld] frame, NCH channels: one 12-byte access where ld == NCH == 3
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

template <int NCH>
__device__ __forceinline__ void store_pixel(float* __restrict__ base, long q, int ld, const float (&v)[NCH]) {
  if constexpr (NCH == 3) {
    if (ld == 3) {
      Float3 w;
      w.x = v[0]; w.y = v[1]; w.z = v[2];
      *reinterpret_cast<Float3*>(base + 3 * q) = w;
      return;
    }
  }
  float* __restrict__ d = base + q * ld;
#pragma unroll
  for (int c = 0; c < NCH; ++c) d[c] = v[c];
}

// a shuffle tree over the 64 lanes: lane 0 holds the result
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- motion
// The position along the motion pass, the offscreen test, the index of the first bilinear tap, the weights and whether the second tap of a
// row / the second row is another pixel or the clamped same one.  fp32, one rounding per operation: no fused multiply-add.
constexpr unsigned DD_MOTION_OFFSCREEN = 1u, DD_MOTION_XSTEP = 2u, DD_MOTION_YSTEP = 4u;

struct dd_motion_position {
  int q00;           // pixel index y0 * W + x0 of the tap (y0, x0); the others are q00 + 1 (XSTEP), q00 + W (YSTEP) and both
  float fx, fy;      // weights of the taps at x0 + 1 and y0 + 1
  unsigned bits;     // DD_MOTION_*; offscreen: q00 = 0, fx = fy = 0 and no step
  float px, py;      // the previous position itself, not rounded (the stabiliser's guides look at the pixel nearest to it)
};

// pixel (x, y) of an H x W frame, H * W <= INT_MAX; motion: [H,W,motion_ld], channels 0 and 1 used.  Force-inlined: a field the caller does
// not read costs nothing.
__device__ __forceinline__ dd_motion_position dd_motion_previous(const float* __restrict__ motion, int motion_ld, float sx, float sy, int x, int y, int H,
                                                                 int W) {
#pragma clang fp contract(off)
  dd_motion_position r;
  r.q00 = 0; r.fx = r.fy = 0.f; r.bits = DD_MOTION_OFFSCREEN;
  const float* __restrict__ mv = motion + ((long)y * W + x) * motion_ld;
  const float px = (float)x + sx * mv[0], py = (float)y + sy * mv[1];
  r.px = px; r.py = py;
  if (!(px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1))) return r;      // (NaN and both infinities fail a comparison)
  const float xf = floorf(px), yf = floorf(py);
  const int ix = min(max((int)xf, 0), W - 1), iy = min(max((int)yf, 0), H - 1);
  r.fx = px - xf; r.fy = py - yf;
  r.q00 = iy * W + ix;
  r.bits = (ix + 1 <= W - 1 ? DD_MOTION_XSTEP : 0u) | (iy + 1 <= H - 1 ? DD_MOTION_YSTEP : 0u);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------- records
constexpr int FRAME_THREADS = 256;                 // threads of every frame-level workgroup
constexpr int FRAME_WAVES = FRAME_THREADS / 64;

// The layout the three record types of include/dd_hip.h have in common; each .hip file asserts it of its own record (frame_record_is).
template <int NU, int ND, bool HAS_MAX>
struct FrameSums {
  unsigned long long u[NU];
  double d[ND];
};
template <int NU, int ND>
struct FrameSums<NU, ND, true> {
  unsigned long long u[NU];
  double d[ND];
  float mx, reserved;
};
// what a .hip file static_asserts of its record: the offsets of its first count, its first sum and its max (without a max: its size)
template <typename Record, int NU, int ND, bool HAS_MAX>
constexpr bool frame_record_is(size_t first_count, size_t first_sum, size_t max_or_size) {
  return first_count == 0 && first_sum == 8 * NU && max_or_size == 8 * (NU + ND) && sizeof(Record) == 8 * (NU + ND) + (HAS_MAX ? 8 : 0) &&
         sizeof(Record) == sizeof(FrameSums<NU, ND, HAS_MAX>) && alignof(Record) == alignof(FrameSums<NU, ND, HAS_MAX>);
}

// The workgroup's counts and sums from what lane 0 of each of its four waves left in LDS: count m from u[m][0 .. 3], sum m from d[m][0 .. 3],
// the waves added in the order ((w0 + w1) + w2) + w3.  One thread, behind a barrier that follows the waves' stores.
template <int NU, int ND>
__device__ __forceinline__ void frame_wave_partial(unsigned long long (&counts)[NU], double (&sums)[ND], const unsigned* const (&u)[NU],
                                                   const double (*d)[FRAME_WAVES]) {
#pragma unroll
  for (int m = 0; m < NU; ++m) counts[m] = u[m][0] + u[m][1] + u[m][2] + u[m][3];
#pragma unroll
  for (int m = 0; m < ND; ++m) sums[m] = ((d[m][0] + d[m][1]) + d[m][2]) + d[m][3];
}

// The body of a finalize kernel, one workgroup of FRAME_THREADS per record: records[blockIdx.x] = the sum of the `tiles` partial records
// partials[blockIdx.x * tiles ..].  Thread t adds records t, t + 256, ... in index order, then a fixed halving tree over the threads: integers
// exactly, the sums in double, the max by fmaxf.
template <typename Record, int NU, int ND, bool HAS_MAX>
__device__ __forceinline__ void frame_finalize(const Record* __restrict__ partials, int tiles, Record* __restrict__ records) {
  using Sums = FrameSums<NU, ND, HAS_MAX>;
  static_assert(sizeof(Record) == sizeof(Sums) && alignof(Record) == alignof(Sums), "the record has the layout of FrameSums");
  __shared__ double sd[ND][FRAME_THREADS];
  __shared__ unsigned long long su[NU][FRAME_THREADS];
  [[maybe_unused]] __shared__ float sf[FRAME_THREADS];      // (without a max: never referenced, no LDS)
  const int tid = threadIdx.x;
  const Sums* __restrict__ p = reinterpret_cast<const Sums*>(partials) + (long)blockIdx.x * tiles;
  Sums t;
#pragma unroll
  for (int m = 0; m < NU; ++m) t.u[m] = 0ull;
#pragma unroll
  for (int m = 0; m < ND; ++m) t.d[m] = 0.0;
  if constexpr (HAS_MAX) t.mx = t.reserved = 0.f;
  for (int b = tid; b < tiles; b += FRAME_THREADS) {
    const Sums r = p[b];
#pragma unroll
    for (int m = 0; m < NU; ++m) t.u[m] += r.u[m];
#pragma unroll
    for (int m = 0; m < ND; ++m) t.d[m] += r.d[m];
    if constexpr (HAS_MAX) t.mx = fmaxf(t.mx, r.mx);
  }
#pragma unroll
  for (int m = 0; m < ND; ++m) sd[m][tid] = t.d[m];
#pragma unroll
  for (int m = 0; m < NU; ++m) su[m][tid] = t.u[m];
  if constexpr (HAS_MAX) sf[tid] = t.mx;
  __syncthreads();
  for (int half = FRAME_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int m = 0; m < ND; ++m) sd[m][tid] += sd[m][tid + half];
#pragma unroll
      for (int m = 0; m < NU; ++m) su[m][tid] += su[m][tid + half];
      if constexpr (HAS_MAX) sf[tid] = fmaxf(sf[tid], sf[tid + half]);
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < NU; ++m) t.u[m] = su[m][0];
#pragma unroll
    for (int m = 0; m < ND; ++m) t.d[m] = sd[m][0];
    if constexpr (HAS_MAX) t.mx = sf[0];
    reinterpret_cast<Sums*>(records)[blockIdx.x] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
template <int TILE>
inline long frame_tiles_of(int n) { return ((long)n + TILE - 1) / TILE; }

// bytes of the partial records of n images of H x W, or DD_ERR_INVALID with the message every *_scratch_bytes gives (count: "n_pairs", ...)
template <int TILE, typename Record>
inline long frame_scratch_bytes(const char* fn, const char* count, int n, int most, int H, int W) {
  DD_REQUIRE(n >= 1 && n <= most && H >= 1 && W >= 1, "%s: %s = %d (1 .. %d), H = %d, W = %d", fn, count, n, most, H, W);
  return (long)n * frame_tiles_of<TILE>(H) * frame_tiles_of<TILE>(W) * (long)sizeof(Record);
}

// The argument checks the entry points repeat, under the caller's name `fn` (the messages are pinned by the ABI tests).
// A frame whose pixels are followed along a motion pass: the shape, the 32-bit pixel index and the grid, the pass and its scale.
template <int TILE>
inline int frame_check_motion(const char* fn, int H, int W, const float* motion, int motion_ld, float sx, float sy) {
  DD_REQUIRE(H >= 1 && W >= 1, "%s: bad shape %d x %d", fn, H, W);
  DD_REQUIRE((long)H * W <= INT_MAX && H <= (1 << 24) && W <= (1 << 24) && frame_tiles_of<TILE>(H) <= 65535,
             "%s: %d x %d does not fit a grid or a 32-bit pixel index", fn, H, W);
  DD_REQUIRE(motion && ((uintptr_t)motion & 3) == 0, "%s: motion is null or not 4-byte aligned", fn);
  DD_REQUIRE(motion_ld >= 2, "%s: motion_ld = %d (the pass has two used channels)", fn, motion_ld);
  DD_REQUIRE(isfinite(sx) && isfinite(sy), "%s: the motion scale is not finite", fn);
  return DD_OK;
}

inline int frame_check_buffers(const char* fn, const void* records, const void* scratch) {
  DD_REQUIRE(records && ((uintptr_t)records & 7) == 0, "%s: records is null or not 8-byte aligned", fn);
  DD_REQUIRE(scratch && ((uintptr_t)scratch & 7) == 0, "%s: scratch is null or not 8-byte aligned", fn);
  return DD_OK;
}
