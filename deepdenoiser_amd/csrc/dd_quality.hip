// Full-frame quality of denoised passes against their targets (include/dd_hip.h: dd_frame_quality): scene-referred error sums, the 8-bit
// display error and the single-scale SSIM of up to 32 image pairs of one frame size, from frames that already sit in device memory.
//
//   frame_quality_kernel   : a workgroup of 256 threads owns QT x QT pixels of one pair (blockIdx.z) and the SSIM windows whose top-left pixel
//                            lies there, so it stages the (QT + 10)^2 patch under those windows once:
//                            stage     every patch pixel is fetched from HBM once (12-byte loads where ld == nch == 3), tested for inf / NaN on the
//                                      bits, quantised against the host's threshold table (dd_png_quantise, csrc/dd_png_core.h) and kept in LDS
//                                      as bytes; the thread that stages an OWNED pixel adds its fp32 error terms to double accumulators
//                            rows      the 11-tap Gaussian along x of  x, y, x^2 + y^2, x y  of the integer bytes, in double (the products are
//                                      exact, so E[x^2] - mu^2 on a flat bright region loses nothing that a pivot would have to save), into LDS,
//                                      two quantities at a time
//                            columns   the 11 taps along y from LDS, the SSIM of the window, added over the channels
//                            The window's validity is a box count of the invalid flags through the same two passes, skipped by a workgroup whose
//                            patch is clean.  Partial sums: a shuffle tree inside a wave, the four waves in order -> one partial record per workgroup.
//   frame_quality_finalize_kernel : one workgroup per pair adds its partial records in a fixed order (integers exactly, the rest in double).
// No atomics at all: two runs give the same bits; a pair's record does not depend on blockIdx.z or on its neighbours in the launch.
#include "dd_frame_common.h"
#include "dd_png_core.h"

namespace {

constexpr int QT = DD_QUALITY_TILE;            // pixels (and window origins) per workgroup side
constexpr int QP = QT + 10;                    // patch side
constexpr int QS = 44;                         // bytes per patch row in LDS (QP rounded up to whole dwords)
constexpr int QI = QT + 1;                     // doubles per row of the row-pass results (odd: the row-pass stores of a wave spread over the banks)
constexpr int QTHREADS = FRAME_THREADS;
constexpr int QWAVES = FRAME_WAVES;
constexpr int QU = 3, QD = 5;                  // counts and sums of a dd_quality_record (then max_abs and reserved)
constexpr int QGROUP = 8;                      // consecutive windows of one patch row per row-pass thread
constexpr int QTABLE = DD_PREVIEW_THRESHOLDS;
constexpr int QITER = (QP * QP + QTHREADS - 1) / QTHREADS;      // patch pixels per thread
static_assert(QT == 32 && QTHREADS == 8 * QT, "the column pass maps a thread to one window column and four rows");
static_assert(frame_record_is<dd_quality_record, QU, QD, true>(offsetof(dd_quality_record, pixels_valid), offsetof(dd_quality_record, se),
                                                               offsetof(dd_quality_record, max_abs)), "dd_quality_record: three uint64 counts, five double sums, max_abs");
static_assert(QP * (QT / QGROUP) <= QTHREADS && QT / QGROUP * QGROUP + 12 <= QS, "one row-pass item per thread, five dwords per item");

struct QualityArgs {
  dd_quality_pair pair[DD_QUALITY_MAX_PAIRS];
  float* map[DD_QUALITY_MAX_PAIRS];
  double gauss[11];                            // normalised 1-D Gaussian, sigma 1.5 (the 2-D filter is its outer product)
};

// The pixel of a pair's image with its RUNTIME channel count (channels nch .. 2 read as 0).  Not dd_frame_common.h's load_pixel<NCH>: with the
// template behind a branch on nch this kernel, at 146 registers, spills 192 bytes per lane (hipcc's resource report).
__device__ __forceinline__ void load_pixel(const float* __restrict__ base, long q, int ld, int nch, float (&v)[3]) {
  v[1] = v[2] = 0.f;
  if (nch == 3 && ld == 3) {
    const Float3 w = *reinterpret_cast<const Float3*>(base + 3 * q);
    v[0] = w.x; v[1] = w.y; v[2] = w.z;
  } else {
    const float* __restrict__ s = base + q * ld;
    v[0] = s[0];
    if (nch == 3) { v[1] = s[1]; v[2] = s[2]; }
  }
}

__global__ __launch_bounds__(QTHREADS) void frame_quality_kernel(const QualityArgs a, int H, int W, const float* __restrict__ thresholds, float exposure,
                                                                 float epsilon, dd_quality_record* __restrict__ partials) {
  __shared__ float thr[QTABLE + 1];
  __shared__ __attribute__((aligned(16))) unsigned char bytes[2][3][QP * QS];      // [prediction | target][channel]
  __shared__ __attribute__((aligned(16))) unsigned char invalid[QP * QS];
  __shared__ unsigned char invalid_rows[QP * QT];                                   // invalid pixels under the 11 taps along x
  __shared__ double rows[2][QP * QI];      // the row pass of two quantities at a time
  __shared__ double wave_d[QD][QWAVES];
  __shared__ unsigned wave_u[QU][QWAVES];
  __shared__ float wave_f[QWAVES];

  const int tid = threadIdx.x;
  const dd_quality_pair P = a.pair[blockIdx.z];
  const int nch = P.nch, x0 = blockIdx.x * QT, y0 = blockIdx.y * QT;
  if (tid < QTABLE) thr[tid] = thresholds[tid];
  __syncthreads();

  // ---------------------------------------------------------------------------------------------- stage the patch, add the owned pixels up
  double se = 0.0, ae = 0.0, rse = 0.0, smape = 0.0;
  float max_abs = 0.f;
  unsigned pixels = 0u, ldr = 0u, bad_here = 0u;      // (ldr: at most 4 owned pixels per thread and 1024 per workgroup, 3 * 255^2 each: fits 32 bits)
  // every load of the thread's QITER patch pixels is issued before the first is used: one exposed HBM latency per workgroup, not QITER
  float pv[QITER][3], tv[QITER][3];
#pragma unroll
  for (int k = 0; k < QITER; ++k) {
    const int i = tid + k * QTHREADS, py = i / QP, px = i - py * QP, y = y0 + py, x = x0 + px;
    pv[k][0] = pv[k][1] = pv[k][2] = tv[k][0] = tv[k][1] = tv[k][2] = 0.f;
    if (i < QP * QP && y < H && x < W) {
      const long q = (long)y * W + x;
      load_pixel(P.pred, q, P.pred_ld, nch, pv[k]);
      load_pixel(P.target, q, P.target_ld, nch, tv[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < QITER; ++k) {
    const int i = tid + k * QTHREADS, py = i / QP, px = i - py * QP, y = y0 + py, x = x0 + px;
    if (i >= QP * QP) break;
    unsigned bp[3] = {0u, 0u, 0u}, bt[3] = {0u, 0u, 0u}, bad = 0u;
    if (y < H && x < W) {
      const float (&p)[3] = pv[k];
      const float (&t)[3] = tv[k];
      bad = (nonfinite(p[0]) || nonfinite(t[0]) || (nch == 3 && (nonfinite(p[1]) || nonfinite(p[2]) || nonfinite(t[1]) || nonfinite(t[2])))) ? 1u : 0u;
      if (!bad) {
        const bool owned = py < QT && px < QT;
        pixels += owned ? 1u : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma clang fp contract(off)
          if (c >= nch) break;
          bp[c] = dd_png_quantise(thr, p[c] * exposure);
          bt[c] = dd_png_quantise(thr, t[c] * exposure);
          if (owned) {
            const float d = p[c] - t[c], ad = fabsf(d), sq = d * d;
            se += (double)sq;
            ae += (double)ad;
            rse += (double)(sq / (t[c] * t[c] + epsilon));
            smape += (double)(ad / (fabsf(p[c]) + fabsf(t[c]) + epsilon));
            max_abs = fmaxf(max_abs, ad);
            const int db = (int)bp[c] - (int)bt[c];
            ldr += (unsigned)(db * db);
          }
        }
      }
    }
    const int o = py * QS + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bytes[0][c][o] = (unsigned char)bp[c];
      bytes[1][c][o] = (unsigned char)bt[c];
    }
    invalid[o] = (unsigned char)bad;
    bad_here |= bad;
  }
  const bool any_bad = __syncthreads_or((int)bad_here) != 0;      // (also the barrier between the stage and the row pass)

  // ---------------------------------------------------------------------------------------------- SSIM of the windows that start in this tile
  double ssim = 0.0;
  unsigned windows = 0u;
  if (y0 + 11 <= H && x0 + 11 <= W) {      // (uniform over the workgroup) the tile has at least one window
    const double C1 = 0.01 * 0.01 * 255.0 * 255.0, C2 = 0.03 * 0.03 * 255.0 * 255.0;      // on bytes instead of bytes / 255: the same quotient
    const int wx = tid & (QT - 1), wy0 = (tid / QT) * 4;      // column pass: one window column, four consecutive window rows
    const int rr = tid % QP, rg = tid / QP;                   // row pass: patch row rr, windows rg * 8 .. + 7 (threads below QP * 4)
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned bad_windows[4] = {0u, 0u, 0u, 0u};
    for (int c = 0; c < nch; ++c) {
      double acc[4][4];      // the window's four moments, filled two at a time: `rows` holds two quantities, so four workgroups fit a CU's LDS
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {      // h = 0: x, y (and the invalid flags);  h = 1: x^2 + y^2, x y
        if (c > 0 || h > 0) __syncthreads();      // the column pass before has read `rows`
        if (tid < QP * (QT / QGROUP)) {
          const unsigned* xr = reinterpret_cast<const unsigned*>(&bytes[0][c][rr * QS + rg * QGROUP]);
          const unsigned* yr = reinterpret_cast<const unsigned*>(&bytes[1][c][rr * QS + rg * QGROUP]);
          unsigned xw[5], yw[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) { xw[k] = xr[k]; yw[k] = yr[k]; }
          double racc[QGROUP][2];
#pragma unroll
          for (int k = 0; k < QGROUP; ++k) racc[k][0] = racc[k][1] = 0.0;
#pragma unroll
          for (int j = 0; j < QGROUP + 10; ++j) {
            const int xi = (int)((xw[j >> 2] >> (8 * (j & 3))) & 0xffu), yi = (int)((yw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            const double v0 = h == 0 ? (double)xi : (double)(xi * xi + yi * yi), v1 = h == 0 ? (double)yi : (double)(xi * yi);
#pragma unroll
            for (int k = 0; k < QGROUP; ++k) {
              const int tap = j - k;
              if (tap < 0 || tap > 10) continue;
              const double g = a.gauss[tap];
              racc[k][0] = fma(g, v0, racc[k][0]);
              racc[k][1] = fma(g, v1, racc[k][1]);
            }
          }
#pragma unroll
          for (int k = 0; k < QGROUP; ++k) {
            rows[0][rr * QI + rg * QGROUP + k] = racc[k][0];
            rows[1][rr * QI + rg * QGROUP + k] = racc[k][1];
          }
          if (h == 0 && c == 0 && any_bad) {
            const unsigned* ir = reinterpret_cast<const unsigned*>(&invalid[rr * QS + rg * QGROUP]);
            unsigned iw[5], cnt[QGROUP];
#pragma unroll
            for (int k = 0; k < 5; ++k) iw[k] = ir[k];
#pragma unroll
            for (int k = 0; k < QGROUP; ++k) cnt[k] = 0u;
#pragma unroll
            for (int j = 0; j < QGROUP + 10; ++j) {
              const unsigned f = (iw[j >> 2] >> (8 * (j & 3))) & 0xffu;
#pragma unroll
              for (int k = 0; k < QGROUP; ++k)
                if (j - k >= 0 && j - k <= 10) cnt[k] += f;
            }
#pragma unroll
            for (int k = 0; k < QGROUP; ++k) invalid_rows[rr * QT + rg * QGROUP + k] = (unsigned char)cnt[k];
          }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 14; ++j) {
          const double v0 = rows[0][(wy0 + j) * QI + wx], v1 = rows[1][(wy0 + j) * QI + wx];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int tap = j - k;
            if (tap < 0 || tap > 10) continue;
            const double g = a.gauss[tap];
            acc[k][2 * h] = fma(g, v0, acc[k][2 * h]);
            acc[k][2 * h + 1] = fma(g, v1, acc[k][2 * h + 1]);
          }
          if (h == 0 && c == 0 && any_bad) {
            const unsigned f = invalid_rows[(wy0 + j) * QT + wx];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (j - k >= 0 && j - k <= 10) bad_windows[k] += f;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double mx = acc[k][0], my = acc[k][1], mm = mx * my, m2 = mx * mx + my * my;
        s[k] += ((2.0 * mm + C1) * (2.0 * (acc[k][3] - mm) + C2)) / ((m2 + C1) * (acc[k][2] - m2 + C2));
      }
    }
    float* __restrict__ map = a.map[blockIdx.z];
    const int MW = W - 10;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int gy = y0 + wy0 + k, gx = x0 + wx;
      if (gy + 11 <= H && gx + 11 <= W) {
        const bool ok = bad_windows[k] == 0u;
        const double v = s[k] / (double)nch;
        if (ok) { ssim += v; ++windows; }
        if (map) map[(long)gy * MW + gx] = ok ? (float)v : __uint_as_float(0x7fc00000u);
      }
    }
  }

  // ---------------------------------------------------------------------------------------------- the workgroup's partial record
  se = wave_sum(se); ae = wave_sum(ae); rse = wave_sum(rse); smape = wave_sum(smape); ssim = wave_sum(ssim);
  pixels = wave_sum(pixels); windows = wave_sum(windows); ldr = wave_sum(ldr);
  max_abs = wave_max(max_abs);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    wave_d[0][w] = se; wave_d[1][w] = ae; wave_d[2][w] = rse; wave_d[3][w] = smape; wave_d[4][w] = ssim;
    wave_u[0][w] = pixels; wave_u[1][w] = windows; wave_u[2][w] = ldr;
    wave_f[w] = max_abs;
  }
  __syncthreads();
  if (tid == 0) {
    FrameSums<QU, QD, true> r;
    frame_wave_partial<QU, QD>(r.u, r.d, {wave_u[0], wave_u[1], wave_u[2]}, wave_d);
    r.mx = fmaxf(fmaxf(wave_f[0], wave_f[1]), fmaxf(wave_f[2], wave_f[3]));
    r.reserved = 0.f;
    reinterpret_cast<FrameSums<QU, QD, true>*>(partials)[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
  }
}

// records[pair] = the sum of the pair's `tiles` partial records (csrc/dd_frame_common.h: frame_finalize)
__global__ __launch_bounds__(QTHREADS) void frame_quality_finalize_kernel(const dd_quality_record* __restrict__ partials, int tiles,
                                                                          dd_quality_record* __restrict__ records) {
  frame_finalize<dd_quality_record, QU, QD, true>(partials, tiles, records);
}

}  // namespace

extern "C" long dd_frame_quality_scratch_bytes(int n_pairs, int H, int W) {
  return frame_scratch_bytes<QT, dd_quality_record>("dd_frame_quality_scratch_bytes", "n_pairs", n_pairs, DD_QUALITY_MAX_PAIRS, H, W);
}

extern "C" int dd_frame_quality(const dd_quality_pair* pairs, int n_pairs, int H, int W, const float* thresholds, float exposure, float epsilon,
                                float* const* ssim_maps, void* records, void* scratch, dd_stream stream) {
  static_assert(sizeof(dd_quality_record) == 72, "dd_quality_record is 72 bytes (include/dd_hip.h, _lib.QualityRecord)");
  DD_REQUIRE(pairs, "dd_frame_quality: null pair table");
  DD_REQUIRE(n_pairs >= 1 && n_pairs <= DD_QUALITY_MAX_PAIRS, "dd_frame_quality: n_pairs = %d (1 .. %d)", n_pairs, DD_QUALITY_MAX_PAIRS);
  DD_REQUIRE(H >= 1 && W >= 1, "dd_frame_quality: bad shape %d x %d", H, W);
  DD_REQUIRE(frame_tiles_of<QT>(H) <= 65535 && frame_tiles_of<QT>(W) <= 0x7fffffffl, "dd_frame_quality: %d x %d does not fit a grid", H, W);
  DD_REQUIRE(thresholds, "dd_frame_quality: no threshold table (thresholds is null)");
  DD_REQUIRE(((uintptr_t)thresholds & 3) == 0, "dd_frame_quality: thresholds must be 4-byte aligned");
  if (int rc = frame_check_buffers("dd_frame_quality", records, scratch)) return rc;
  DD_REQUIRE(epsilon > 0.f, "dd_frame_quality: epsilon must be positive");
  QualityArgs a;
  for (int i = 0; i < DD_QUALITY_MAX_PAIRS; ++i) {
    a.pair[i] = dd_quality_pair{nullptr, nullptr, 0, 0, 0};
    a.map[i] = nullptr;
  }
  for (int i = 0; i < n_pairs; ++i) {
    const dd_quality_pair& p = pairs[i];
    DD_REQUIRE(p.pred && p.target, "dd_frame_quality: pair %d has a null pred / target", i);
    DD_REQUIRE(((uintptr_t)p.pred & 3) == 0 && ((uintptr_t)p.target & 3) == 0, "dd_frame_quality: pair %d is not 4-byte aligned", i);
    DD_REQUIRE(p.nch == 1 || p.nch == 3, "dd_frame_quality: pair %d has %d channels (1 or 3 expected)", i, p.nch);
    DD_REQUIRE(p.pred_ld >= p.nch && p.target_ld >= p.nch, "dd_frame_quality: pair %d has a pixel stride (ld) below its channels", i);
    a.pair[i] = p;
    if (ssim_maps && H >= 11 && W >= 11) {
      DD_REQUIRE(((uintptr_t)ssim_maps[i] & 3) == 0, "dd_frame_quality: ssim_maps[%d] is not 4-byte aligned", i);
      a.map[i] = ssim_maps[i];
    }
  }
  double e[11], sum = 0.0;
  for (int i = 0; i < 11; ++i) { e[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += e[i]; }
  for (int i = 0; i < 11; ++i) a.gauss[i] = e[i] / sum;
  const int tx = (int)frame_tiles_of<QT>(W), ty = (int)frame_tiles_of<QT>(H);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(frame_quality_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)n_pairs), dim3(QTHREADS), 0, s, a, H, W, thresholds, exposure, epsilon,
                     reinterpret_cast<dd_quality_record*>(scratch));
  DD_LAUNCH_CHECK();
  hipLaunchKernelGGL(frame_quality_finalize_kernel, dim3((unsigned)n_pairs), dim3(QTHREADS), 0, s, reinterpret_cast<const dd_quality_record*>(scratch), tx * ty,
                     reinterpret_cast<dd_quality_record*>(records));
  DD_LAUNCH_CHECK();
  return DD_OK;
}
