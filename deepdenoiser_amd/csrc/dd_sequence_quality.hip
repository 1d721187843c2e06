// Temporal error of a denoised frame sequence against its target frames (include/dd_hip.h: dd_sequence_quality): per pair of (prediction,
// target) images how much each changed against its own previous frame fetched along the motion vectors, and how much the ERROR changed,
// scene-referred and on the 8-bit display bytes.
//
//   sequence_quality_kernel          : a workgroup of 256 threads owns ST x ST pixels, one per thread (a wave's lanes are four rows of 16
//                                      neighbours).  ONCE per pixel: the previous position from the motion pass, the offscreen test, the tap
//                                      index and the weights (csrc/dd_frame_common.h: dd_motion_previous, the function the stabiliser
//                                      compiles too): four registers for the whole launch.  Then the loop over the pairs, per pair:
//                                      fetch     the pixel of `pred` and `target` and the four taps of both previous frames straight from
//                                                global memory, all ten issued before the first is used (12-byte loads where ld == nch == 3;
//                                                neighbouring lanes share lines)
//                                      test      the bits of all ten for inf / NaN
//                                      terms     the two bilinear samples, dp, dt, e; the bytes of the ten values by a binary search of the
//                                                threshold table (its two upper levels from three registers, the six lower ones from LDS,
//                                                staged once per workgroup LEVEL BY LEVEL: the entries one step of the search chooses among
//                                                are neighbours in LDS and lie on different banks; in the table's own order they are 2 * step
//                                                apart and the 4 / 8 / 16 / 32 candidates of the upper levels share one, one, two and four
//                                                banks), the same bilinear form on the bytes
//                                      sums      fp32 terms added in double per thread, a shuffle tree inside a wave, the four waves in order
//                                                -> one partial record per (pair, workgroup), written by thread 0 while the next pair is
//                                                fetched
//   sequence_quality_finalize_kernel : one workgroup per pair adds its partial records in a fixed order (integers exactly, the rest in double).
// No atomics at all: two runs give the same bits; a pair's record does not depend on its index or on its neighbours in the call.  Nothing but
// the partial records and the records is written.
#include "dd_frame_common.h"

namespace {

constexpr int ST = DD_SEQQ_TILE;               // pixels per workgroup side
constexpr int STHREADS = FRAME_THREADS;
constexpr int SWAVES = FRAME_WAVES;
constexpr int SU = 3, SD = 6;                  // counts and sums of a dd_seqq_record
constexpr int STABLE = DD_PREVIEW_THRESHOLDS;
static_assert(ST * ST == STHREADS && (ST & (ST - 1)) == 0 && SWAVES == 4, "a thread owns the pixel (tid / ST, tid % ST) of the tile");
static_assert(STABLE == 255, "the binary search takes steps of 128 .. 1 over 255 entries");
static_assert(frame_record_is<dd_seqq_record, SU, SD, false>(offsetof(dd_seqq_record, pixels_offscreen), offsetof(dd_seqq_record, change_prediction),
                                                             sizeof(dd_seqq_record)), "dd_seqq_record: three uint64 counts, six double sums");
constexpr int SLEVELS = 6;                     // the levels of the search that read LDS: steps 32 .. 1
constexpr int SNODES = 4 * ((1 << SLEVELS) - 1);      // 4 + 8 + .. + 128 entries; level l (step 32 >> l) starts at 4 * (2^l - 1)

constexpr unsigned SQ_INSIDE = 8u;             // next to the DD_MOTION_* bits: the thread's pixel lies in the image

struct SequenceArgs {
  dd_seqq_pair pair[DD_SEQQ_MAX_PAIRS];
  const float* motion;
  const float* thresholds;
  int motion_ld, n_pairs;
  float sx, sy, exposure;
};

// the upper two levels of the search: entries 63, 127 and 191 of the table
struct Pivots { float t63, t127, t191; };

// number of table entries <= v, as a float.  The definition it must equal is dd_png_quantise (csrc/dd_png_core.h), which the other launches
// call: the same eight comparisons (entry lo + step - 1 with lo a multiple of 2 * step), the entry read as node j = lo / (2 * step) of its
// level; j doubles and takes the comparison's bit, and ends as the count.  Kept apart for its data layout (the level-ordered table in LDS).
__device__ __forceinline__ float quantise(const float* nodes, const Pivots& k, float v) {
  unsigned j = k.t127 <= v ? 1u : 0u;
  j = 2u * j + ((j ? k.t191 : k.t63) <= v ? 1u : 0u);
#pragma unroll
  for (int l = 0; l < SLEVELS; ++l) j = 2u * j + (nodes[4 * ((1 << l) - 1) + j] <= v ? 1u : 0u);
  return (float)j;
}

__device__ __forceinline__ float bilinear(float a00, float a01, float a10, float a11, float fx, float gx, float fy, float gy) {
#pragma clang fp contract(off)
  return (a00 * gx + a01 * fx) * gy + (a10 * gx + a11 * fx) * fy;
}

// One pair of the tile.  q: the thread's pixel index; wave_d / wave_u: this pair's buffers of the per-wave sums.
template <int NCH>
__device__ __forceinline__ void score_pair(const dd_seqq_pair& P, const dd_motion_position& s, long q, int W, const float* thr, const Pivots& k, float exposure,
                                           double (*wave_d)[SWAVES], unsigned (*wave_u)[SWAVES]) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const bool candidate = (s.bits & (SQ_INSIDE | DD_MOTION_OFFSCREEN)) == SQ_INSIDE;
  // ---------------------------------------------------------------------------------------------- fetch
  float p[NCH], t[NCH], a[4][NCH], b[4][NCH];      // a: the taps of pred_previous, b: of target_previous
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    p[c] = t[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j][c] = b[j][c] = 0.f;
  }
  if (candidate) {
    const long q0 = s.q00, dx = (s.bits & DD_MOTION_XSTEP) ? 1 : 0, dy = (s.bits & DD_MOTION_YSTEP) ? W : 0;
    load_pixel<NCH>(P.pred, q, P.pred_ld, p);
    load_pixel<NCH>(P.target, q, P.target_ld, t);
    load_pixel<NCH>(P.pred_previous, q0, P.pred_previous_ld, a[0]);
    load_pixel<NCH>(P.pred_previous, q0 + dx, P.pred_previous_ld, a[1]);
    load_pixel<NCH>(P.pred_previous, q0 + dy, P.pred_previous_ld, a[2]);
    load_pixel<NCH>(P.pred_previous, q0 + dy + dx, P.pred_previous_ld, a[3]);
    load_pixel<NCH>(P.target_previous, q0, P.target_previous_ld, b[0]);
    load_pixel<NCH>(P.target_previous, q0 + dx, P.target_previous_ld, b[1]);
    load_pixel<NCH>(P.target_previous, q0 + dy, P.target_previous_ld, b[2]);
    load_pixel<NCH>(P.target_previous, q0 + dy + dx, P.target_previous_ld, b[3]);
  }
  // ---------------------------------------------------------------------------------------------- test
  bool bad = false;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    bad = bad || nonfinite(p[c]) || nonfinite(t[c]);
#pragma unroll
    for (int j = 0; j < 4; ++j) bad = bad || nonfinite(a[j][c]) || nonfinite(b[j][c]);
  }
  const bool valid = candidate && !bad;
  // ---------------------------------------------------------------------------------------------- terms
  double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // |dp| |dt| |e| |DP| |DT| |DP - DT|
  if (valid) {
    const float fx = s.fx, fy = s.fy, gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float hp = bilinear(a[0][c], a[1][c], a[2][c], a[3][c], fx, gx, fy, gy);
      const float ht = bilinear(b[0][c], b[1][c], b[2][c], b[3][c], fx, gx, fy, gy);
      const float dp = p[c] - hp, dt = t[c] - ht;
      d[0] += (double)fabsf(dp);
      d[1] += (double)fabsf(dt);
      d[2] += (double)fabsf(dp - dt);
      const float Hp = bilinear(quantise(thr, k, exposure * a[0][c]), quantise(thr, k, exposure * a[1][c]), quantise(thr, k, exposure * a[2][c]),
                                quantise(thr, k, exposure * a[3][c]), fx, gx, fy, gy);
      const float Ht = bilinear(quantise(thr, k, exposure * b[0][c]), quantise(thr, k, exposure * b[1][c]), quantise(thr, k, exposure * b[2][c]),
                                quantise(thr, k, exposure * b[3][c]), fx, gx, fy, gy);
      const float DP = quantise(thr, k, exposure * p[c]) - Hp, DT = quantise(thr, k, exposure * t[c]) - Ht;
      d[3] += (double)fabsf(DP);
      d[4] += (double)fabsf(DT);
      d[5] += (double)fabsf(DP - DT);
    }
  }
  // ---------------------------------------------------------------------------------------------- sums
  unsigned n_nonfinite = (candidate && bad) ? 1u : 0u, n_valid = valid ? 1u : 0u;
#pragma unroll
  for (int m = 0; m < 6; ++m) d[m] = wave_sum(d[m]);
  n_nonfinite = wave_sum(n_nonfinite); n_valid = wave_sum(n_valid);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
#pragma unroll
    for (int m = 0; m < 6; ++m) wave_d[m][w] = d[m];
    wave_u[0][w] = n_nonfinite; wave_u[1][w] = n_valid;
  }
}

__global__ __launch_bounds__(STHREADS) void sequence_quality_kernel(const SequenceArgs a, int H, int W, dd_seqq_record* __restrict__ partials) {
  __shared__ float thr[SNODES];                  // the table's entries 2 s j + s - 1 in the order (s = 32, 16, .. 1; j): quantise
  __shared__ double wave_d[2][SD][SWAVES];       // [pair parity][sum]
  __shared__ unsigned wave_u[2][2][SWAVES];      // [pair parity][nonfinite | valid]
  __shared__ unsigned wave_c[SWAVES];            // offscreen: the same for every pair

  const int tid = threadIdx.x, x = blockIdx.x * ST + (tid & (ST - 1)), y = blockIdx.y * ST + tid / ST;
  if (tid < SNODES) {
    const int l = 31 - __clz(tid / 4 + 1), j = tid - 4 * ((1 << l) - 1), step = 32 >> l;
    thr[tid] = a.thresholds[2 * step * j + step - 1];
  }
  const Pivots k = {a.thresholds[63], a.thresholds[127], a.thresholds[191]};
  // ---------------------------------------------------------------------------------------------- once per pixel
  dd_motion_position s;
  s.q00 = 0; s.fx = s.fy = 0.f; s.bits = 0u;
  if (y < H && x < W) {
    s = dd_motion_previous(a.motion, a.motion_ld, a.sx, a.sy, x, y, H, W);
    s.bits |= SQ_INSIDE;
  }
  const unsigned n_offscreen = wave_sum((s.bits & (SQ_INSIDE | DD_MOTION_OFFSCREEN)) == (SQ_INSIDE | DD_MOTION_OFFSCREEN) ? 1u : 0u);
  if ((tid & 63) == 0) wave_c[tid >> 6] = n_offscreen;
  const long q = (s.bits & SQ_INSIDE) ? (long)y * W + x : 0;

  // ---------------------------------------------------------------------------------------------- the pairs
  const long block = (long)blockIdx.y * gridDim.x + blockIdx.x, blocks = (long)gridDim.x * gridDim.y;
  auto write_partial = [&](int p) {      // thread 0, behind a barrier that follows pair p's sums
    const int b = p & 1;
    FrameSums<SU, SD, false> r;
    frame_wave_partial<SU, SD>(r.u, r.d, {wave_c, wave_u[b][0], wave_u[b][1]}, wave_d[b]);
    reinterpret_cast<FrameSums<SU, SD, false>*>(partials)[(long)p * blocks + block] = r;
  };
  for (int p = 0; p < a.n_pairs; ++p) {
    __syncthreads();      // the table is staged; the pair before has left its sums (two buffers: pair p + 1 fills the other one)
    if (tid == 0 && p > 0) write_partial(p - 1);
    const dd_seqq_pair P = a.pair[p];
    if (P.nch == 3)
      score_pair<3>(P, s, q, W, thr, k, a.exposure, wave_d[p & 1], wave_u[p & 1]);
    else
      score_pair<1>(P, s, q, W, thr, k, a.exposure, wave_d[p & 1], wave_u[p & 1]);
  }
  __syncthreads();
  if (tid == 0) write_partial(a.n_pairs - 1);
}

// records[pair] = the sum of the pair's `tiles` partial records (csrc/dd_frame_common.h: frame_finalize)
__global__ __launch_bounds__(STHREADS) void sequence_quality_finalize_kernel(const dd_seqq_record* __restrict__ partials, int tiles,
                                                                             dd_seqq_record* __restrict__ records) {
  frame_finalize<dd_seqq_record, SU, SD, false>(partials, tiles, records);
}

}  // namespace

extern "C" long dd_sequence_quality_scratch_bytes(int n_pairs, int H, int W) {
  return frame_scratch_bytes<ST, dd_seqq_record>("dd_sequence_quality_scratch_bytes", "n_pairs", n_pairs, DD_SEQQ_MAX_PAIRS, H, W);
}

extern "C" int dd_sequence_quality(const dd_seqq_pair* pairs, int n_pairs, int H, int W, const float* motion, int motion_ld, float sx, float sy,
                                   const float* thresholds, float exposure, void* records, void* scratch, dd_stream stream) {
  static_assert(sizeof(dd_seqq_record) == 72, "dd_seqq_record is 72 bytes (include/dd_hip.h, _lib.SequenceQualityRecord)");
  static_assert(sizeof(dd_seqq_pair) == 56, "include/dd_hip.h, _lib.SequenceQualityPair");
  DD_REQUIRE(pairs, "dd_sequence_quality: null pair table");
  DD_REQUIRE(n_pairs >= 1 && n_pairs <= DD_SEQQ_MAX_PAIRS, "dd_sequence_quality: n_pairs = %d (1 .. %d)", n_pairs, DD_SEQQ_MAX_PAIRS);
  if (int rc = frame_check_motion<ST>("dd_sequence_quality", H, W, motion, motion_ld, sx, sy)) return rc;
  DD_REQUIRE(thresholds && ((uintptr_t)thresholds & 3) == 0, "dd_sequence_quality: thresholds is null or not 4-byte aligned");
  DD_REQUIRE(isfinite(exposure), "dd_sequence_quality: the exposure is not finite");
  if (int rc = frame_check_buffers("dd_sequence_quality", records, scratch)) return rc;
  SequenceArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_pairs; ++i) {
    const dd_seqq_pair& p = pairs[i];
    DD_REQUIRE(p.pred && p.pred_previous && p.target && p.target_previous, "dd_sequence_quality: pair %d has a null pred / pred_previous / target / target_previous", i);
    DD_REQUIRE((((uintptr_t)p.pred | (uintptr_t)p.pred_previous | (uintptr_t)p.target | (uintptr_t)p.target_previous) & 3) == 0,
               "dd_sequence_quality: pair %d is not 4-byte aligned", i);
    DD_REQUIRE(p.nch == 1 || p.nch == 3, "dd_sequence_quality: pair %d has %d channels (1 or 3 expected)", i, p.nch);
    DD_REQUIRE(p.pred_ld >= p.nch && p.pred_previous_ld >= p.nch && p.target_ld >= p.nch && p.target_previous_ld >= p.nch,
               "dd_sequence_quality: pair %d has a pixel stride (ld) below its channels", i);
    a.pair[i] = p;
  }
  a.motion = motion; a.thresholds = thresholds; a.motion_ld = motion_ld; a.n_pairs = n_pairs;
  a.sx = sx; a.sy = sy; a.exposure = exposure;
  const int tx = (int)frame_tiles_of<ST>(W), ty = (int)frame_tiles_of<ST>(H);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sequence_quality_kernel, dim3((unsigned)tx, (unsigned)ty), dim3(STHREADS), 0, s, a, H, W, reinterpret_cast<dd_seqq_record*>(scratch));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(sequence_quality_finalize_kernel, dim3((unsigned)n_pairs), dim3(STHREADS), 0, s, reinterpret_cast<const dd_seqq_record*>(scratch), tx * ty,
                     reinterpret_cast<dd_seqq_record*>(records));
  DD_LAUNCH_CHECK();
  return DD_OK;
}
