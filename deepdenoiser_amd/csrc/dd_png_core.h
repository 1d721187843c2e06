// The PNG row coder shared by the device kernel (dd_png_encode.hip: png_pack_kernel) and a stand-alone host program (tests/png_core_main.cpp):
// everything that decides a BYTE of a filtered row lives here, as functions that compile for the host and for the device from the same text
// (like dd_deflate_core.h), so the two builds give the same bytes and the CPU build runs under sanitizers before the code runs on a GPU.
//
// The byte of a sample: v = sample * exposure (one fp32 multiply, never contracted), byte = the number of entries of the 255-entry threshold
// table (metrics.preview_thresholds: the host owns the sRGB transfer function, the device only compares) that are <= v.  -inf, negatives
// and -0.0 give 0, +inf gives 255; every comparison with a NaN is false, so a NaN gives 0: that is the gray rule, and an RGB pixel with a NaN
// in any channel becomes (255, 0, 255) as in the previews (dd_preview.hip).
//
// The filter of a row (RFC 2083 section 6): x the byte, a the byte `bpp` to the left, b the byte above, c the byte above a; bytes outside the
// row, and the row above the first, are 0.  Type 0 None x, 1 Sub x - a, 2 Up x - b, 3 Average x - floor((a + b) / 2), 4 Paeth x - the one of
// a, b, c nearest to a + b - c (ties: a, then b), all modulo 256.  The type of a row is the one with the smallest sum of |filtered byte read as
// signed 8-bit| over the row, ties to the lowest number: integer arithmetic, the same on every path.
//
// Lanes.  A row is worked on by `lanes` workers; worker `lane` takes the bytes (or pixels) lane, lane + lanes, ...  On the device the workers
// are the threads of the workgroup, on the CPU a loop.  The sums of the workers are added by the caller (in any order: integers).
#ifndef DD_PNG_CORE_H
#define DD_PNG_CORE_H

#if defined(__HIPCC__)
#define DD_PNG_DHD __host__ __device__ __forceinline__
#else
#define DD_PNG_DHD inline
#endif

#define DD_PNG_THRESHOLDS 255
#define DD_PNG_FILTERS 5

// the number of table entries <= v: a branch-free binary search (8 steps: 128 + 64 + ... + 1 = 255)
DD_PNG_DHD unsigned dd_png_quantise(const float* thr, float v) {
  unsigned lo = 0;
  for (unsigned step = 128; step > 0; step >>= 1)
    if (thr[lo + step - 1] <= v) lo += step;      // lo + step <= 255 always
  return lo;
}

// The bytes of the pixels lane, lane + lanes, ... of one row: row = the fp32 samples of the row ([W, C]), channel[k] the plane channel of
// byte k of a pixel, n = 1 (gray) or 3 (RGB) -> bytes[W * n].
DD_PNG_DHD void dd_png_quantise_row(const float* thr, const float* row, int W, int C, int n, const int* channel, float exposure, int lane, int lanes,
                                    unsigned char* bytes) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int x = lane; x < W; x += lanes) {
    const float* p = row + (long)x * C;
    if (n == 1) {
      bytes[x] = (unsigned char)dd_png_quantise(thr, p[channel[0]] * exposure);
    } else {
      const float r = p[channel[0]] * exposure, g = p[channel[1]] * exposure, b = p[channel[2]] * exposure;
      const bool nan = r != r || g != g || b != b;
      bytes[3 * x + 0] = (unsigned char)(nan ? 255u : dd_png_quantise(thr, r));
      bytes[3 * x + 1] = (unsigned char)(nan ? 0u : dd_png_quantise(thr, g));
      bytes[3 * x + 2] = (unsigned char)(nan ? 255u : dd_png_quantise(thr, b));
    }
  }
}

DD_PNG_DHD int dd_png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// byte i of the row under filter `type`; cur / up: the row's bytes and those of the row above (up == nullptr: zeros)
DD_PNG_DHD unsigned dd_png_filtered(int type, const unsigned char* cur, const unsigned char* up, int i, int bpp) {
  const int x = cur[i], a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
  const int predicted = type == 0 ? 0 : (type == 1 ? a : (type == 2 ? b : (type == 3 ? (a + b) >> 1 : dd_png_paeth(a, b, c))));
  return (unsigned)(x - predicted) & 0xffu;
}

// cost[t] += the sum over the bytes lane, lane + lanes, ... < nbytes of |filtered byte as signed 8-bit| under filter t
DD_PNG_DHD void dd_png_row_costs(const unsigned char* cur, const unsigned char* up, int nbytes, int bpp, int lane, int lanes, unsigned* cost) {
  for (int i = lane; i < nbytes; i += lanes) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < DD_PNG_FILTERS; ++t) {
      const unsigned f = dd_png_filtered(t, cur, up, i, bpp);
      cost[t] += f < 128u ? f : 256u - f;
    }
  }
}

// the type with the smallest sum, ties to the lowest number
DD_PNG_DHD int dd_png_pick(const unsigned* cost) {
  int best = 0;
  for (int t = 1; t < DD_PNG_FILTERS; ++t)
    if (cost[t] < cost[best]) best = t;
  return best;
}

// the filtered row: dst[0] the type byte (by lane 0), dst[1 + i] the filtered bytes lane, lane + lanes, ...
DD_PNG_DHD void dd_png_write_row(int type, const unsigned char* cur, const unsigned char* up, int nbytes, int bpp, int lane, int lanes, unsigned char* dst) {
  if (lane == 0) dst[0] = (unsigned char)type;
  for (int i = lane; i < nbytes; i += lanes) dst[1 + i] = (unsigned char)dd_png_filtered(type, cur, up, i, bpp);
}

#endif  // DD_PNG_CORE_H
