// Image summaries: 8-bit display previews of source | prediction | target | difference, rendered where the tensors are
// (include/dd_hip.h: dd_loss_previews).  The reference writes no image summaries; this is what tf.summary.image would be given.
//
//   previews : store-shaped.  A thread owns PV_PIX consecutive pixels of one panel row of one mosaic: it forms their values with the
//              helpers of dd_loss_common.h (the raw passes are one more SIDE next to predictions and targets), quantises every channel
//              against the host's threshold table and packs the 3-byte pixels into three dwords.  Where the 12 bytes start on a 4-byte
//              boundary and the panel row has all four pixels they leave as whole dwords; the tail of a row whose length is no multiple
//              of 4 pixels, and rows that start off a boundary, leave as bytes.  Plain vector stores, no atomics, every output byte has
//              exactly one writer: two runs give the same bits.
//   quantise : byte = number of table entries <= v, a branch-free binary search (8 steps: 128 + 64 + ... + 1 = 255) over the table in
//              LDS.  The device never evaluates a transfer function; the table clamps by construction (+inf -> 255, -inf -> 0), and every
//              comparison with a NaN is false, so NaN is found separately: one NaN channel makes the whole pixel (255, 0, 255).
#include "dd_common.h"
#include "dd_loss_common.h"

namespace {

constexpr int PV_PIX = 4;                           // pixels per thread: 12 bytes = 3 dwords
constexpr int PV_TABLE = DD_PREVIEW_THRESHOLDS;     // 255
constexpr int PV_PANELS = 4;

struct PreviewSel {
  const float* source[DD_MAX_FEATURES];             // raw noisy passes (NULL without the source panel)
  int source_ld[DD_MAX_FEATURES];
  int images[DD_PREVIEW_MAX_IMAGES];
  unsigned char slots[DD_METRIC_SOURCES];
  unsigned char panel[PV_PANELS];                   // panel index -> bit number (0 source, 1 prediction, 2 target, 3 difference)
  int n_images, n_slots, n_panels;
};

// number of table entries <= v (0 for a NaN)
__device__ __forceinline__ unsigned quantise(const float* thr, float v) {
  unsigned lo = 0;
#pragma unroll
  for (unsigned step = 128; step > 0; step >>= 1)
    if (thr[lo + step - 1] <= v) lo += step;        // lo + step <= 255 always
  return lo;
}

// the slot's value on one side at pixel i
__device__ __forceinline__ void slot_value(const dd_loss_desc& d, const LossSide s, int slot, long i, float (&v)[3]) {
  const LossSide sd[1] = {s};
  SideVal<1> a;
  if (slot < DD_MAX_FEATURES) a = feature_sides<1>(d, sd, slot, i);
  else if (slot < DD_MAX_FEATURES + DD_MAX_COMBINED) a = combined_sides<1>(d, sd, slot - DD_MAX_FEATURES, i);
  else a = image_sides<1>(d, sd, i);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = a.s[0][c];
}

// |channel-summed LossDifference(p, t)| * gain, one rounding per operation
__device__ __forceinline__ float difference_value(int kind, float eps, const float (&p)[3], const float (&t)[3], int nch, float gain) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if (ch >= nch) break;
    float l, dl;
    loss_term(kind, eps, p[ch], t[ch], &l, &dl);
    s += l;
  }
  return fabsf(s) * gain;
}

__global__ __launch_bounds__(256) void loss_previews_kernel(const dd_loss_desc d, const PreviewSel sel, int B, int H, int W, int groups, long total,
                                                            const float* __restrict__ thresholds, float exposure, float error_gain,
                                                            unsigned char* __restrict__ out) {
  __shared__ float thr[PV_TABLE + 1];
  if (threadIdx.x < PV_TABLE) thr[threadIdx.x] = thresholds[threadIdx.x];
  __syncthreads();
  const long tid = (long)blockIdx.x * 256 + threadIdx.x;
  if (tid >= total) return;
  // tid = (((slot * n_images + r) * H + y) * n_panels + panel) * groups + g
  const int g = (int)(tid % groups);
  long rest = tid / groups;
  const int pn = (int)(rest % sel.n_panels);
  rest /= sel.n_panels;
  const int y = (int)(rest % H);
  rest /= H;                                          // = slot index * n_images + r: the mosaic's image row
  const int r = (int)(rest % sel.n_images), si = (int)(rest / sel.n_images);
  const int slot = sel.slots[si], what = sel.panel[pn], b = sel.images[r];
  const int x0 = g * PV_PIX, npix = min(PV_PIX, W - x0);
  const long pix0 = ((long)b * H + y) * W + x0;
  const int nch = (slot < DD_MAX_FEATURES && d.nch[slot] == 1) ? 1 : 3;
  const LossSide source_side = {sel.source, sel.source_ld};
  const LossSide side = what == 0 ? source_side : (what == 1 ? pred_side(d) : target_side(d));      // (the difference panel reads both)

  unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < PV_PIX; ++k) {
    if (k >= npix) break;
    float v[3];
    if (what < 3) {
#pragma clang fp contract(off)
      slot_value(d, side, slot, pix0 + k, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = v[c] * exposure;
    } else {
      float p[3], t[3];
      slot_value(d, pred_side(d), slot, pix0 + k, p);
      slot_value(d, target_side(d), slot, pix0 + k, t);
      v[0] = v[1] = v[2] = difference_value(d.kind, d.epsilon, p, t, nch, error_gain);
    }
    unsigned q[3];
    if (v[0] != v[0] || v[1] != v[1] || v[2] != v[2]) {      // a NaN channel: the whole pixel is magenta
      q[0] = 255u; q[1] = 0u; q[2] = 255u;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] = quantise(thr, v[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int byte = 3 * k + c;                      // (compile-time after unrolling: no indexed register array)
      word[byte >> 2] |= q[c] << (8 * (byte & 3));
    }
  }
  // the thread's bytes in the mosaic: row (r * H + y) of mosaic si, panel pn, from pixel x0
  const long row_bytes = 3l * sel.n_panels * W;
  unsigned char* dst = out + (rest * H + y) * row_bytes + 3l * pn * W + 3l * x0;
  if (npix == PV_PIX && ((uintptr_t)dst & 3) == 0) {
    unsigned* dw = reinterpret_cast<unsigned*>(dst);
    dw[0] = word[0]; dw[1] = word[1]; dw[2] = word[2];
  } else {
#pragma unroll
    for (int j = 0; j < 3 * PV_PIX; ++j)
      if (j < 3 * npix) dst[j] = (unsigned char)(word[j >> 2] >> (8 * (j & 3)));
  }
}

}  // namespace

extern "C" int dd_loss_previews(const dd_loss_desc* desc, const float* const* source, const int* source_ld, int B, int H, int W, const int* images,
                                int n_images, const int* slots, int n_slots, int panels, const float* thresholds, float exposure, float error_gain,
                                unsigned char* out, dd_stream stream) {
  DD_REQUIRE(desc && images && slots && out, "dd_loss_previews: null descriptor / images / slots / out");
  DD_REQUIRE(thresholds, "dd_loss_previews: no threshold table (thresholds is null)");
  DD_REQUIRE(((uintptr_t)thresholds & 3) == 0, "dd_loss_previews: thresholds must be 4-byte aligned");
  DD_REQUIRE(B > 0 && H > 0 && W > 0, "dd_loss_previews: bad shape %d x %d x %d", B, H, W);
  DD_REQUIRE(n_images >= 1 && n_images <= DD_PREVIEW_MAX_IMAGES, "dd_loss_previews: n_images = %d (1 .. %d)", n_images, DD_PREVIEW_MAX_IMAGES);
  DD_REQUIRE(n_slots >= 1 && n_slots <= DD_METRIC_SOURCES, "dd_loss_previews: n_slots = %d (1 .. %d)", n_slots, DD_METRIC_SOURCES);
  DD_REQUIRE(panels > 0 && panels < (1 << PV_PANELS), "dd_loss_previews: panels = %d (a non-empty mask of 1 source, 2 prediction, 4 target, 8 difference)", panels);
  DD_REQUIRE(!(panels & DD_PREVIEW_SOURCE) || (source && source_ld), "dd_loss_previews: the source panel is asked for but source / source_ld is null");
  DD_REQUIRE(desc->n_features > 0 && desc->n_features <= DD_MAX_FEATURES && desc->n_combined >= 0 && desc->n_combined <= DD_MAX_COMBINED,
             "dd_loss_previews: n_features / n_combined out of range");
  DD_REQUIRE(desc->n_image_combined >= 0 && desc->n_image_combined <= DD_MAX_COMBINED && desc->n_image_features >= 0 &&
                 desc->n_image_features <= DD_MAX_FEATURES, "dd_loss_previews: image member counts out of range");
  DD_REQUIRE(!(panels & DD_PREVIEW_DIFFERENCE) || (desc->kind >= 1 && desc->kind <= 5), "dd_loss_previews: unknown loss kind %d", desc->kind);
  PreviewSel sel;
  for (int f = 0; f < DD_MAX_FEATURES; ++f) { sel.source[f] = nullptr; sel.source_ld[f] = 0; }
  for (int f = 0; f < desc->n_features; ++f) {
    DD_REQUIRE(desc->pred[f] && desc->target[f], "dd_loss_previews: feature %d has a null pred / target", f);
    DD_REQUIRE(desc->nch[f] == 1 || desc->nch[f] == 3, "dd_loss_previews: feature %d has %d channels (1 or 3 expected)", f, desc->nch[f]);
    DD_REQUIRE(desc->pred_ld[f] >= desc->nch[f] && desc->target_ld[f] >= desc->nch[f], "dd_loss_previews: feature %d has a pixel stride below its channels", f);
    DD_REQUIRE(((uintptr_t)desc->pred[f] & 3) == 0 && ((uintptr_t)desc->target[f] & 3) == 0, "dd_loss_previews: feature %d is not 4-byte aligned", f);
    if (panels & DD_PREVIEW_SOURCE) {
      DD_REQUIRE(source[f] && ((uintptr_t)source[f] & 3) == 0, "dd_loss_previews: source[%d] is null or not 4-byte aligned", f);
      DD_REQUIRE(source_ld[f] >= desc->nch[f], "dd_loss_previews: source[%d] has a pixel stride below its channels", f);
      sel.source[f] = source[f];
      sel.source_ld[f] = source_ld[f];
    }
  }
  for (int k = 0; k < desc->n_combined; ++k)
    for (int c = 0; c < 3; ++c)
      DD_REQUIRE(desc->comb[k][c] >= 0 && desc->comb[k][c] < desc->n_features, "dd_loss_previews: comb[%d][%d] is not a feature index", k, c);
  for (int i = 0; i < desc->n_image_combined; ++i)
    DD_REQUIRE(desc->image_combined[i] >= 0 && desc->image_combined[i] < desc->n_combined, "dd_loss_previews: image_combined[%d] is not a combined index", i);
  for (int i = 0; i < desc->n_image_features; ++i)
    DD_REQUIRE(desc->image_features[i] >= 0 && desc->image_features[i] < desc->n_features, "dd_loss_previews: image_features[%d] is not a feature index", i);
  for (int r = 0; r < n_images; ++r) {
    DD_REQUIRE(images[r] >= 0 && images[r] < B, "dd_loss_previews: images[%d] = %d is not a batch index (B = %d)", r, images[r], B);
    sel.images[r] = images[r];
  }
  for (int s = 0; s < n_slots; ++s) {
    const int slot = slots[s];
    const bool is_f = slot >= 0 && slot < desc->n_features, is_c = slot >= DD_MAX_FEATURES && slot < DD_MAX_FEATURES + desc->n_combined;
    const bool is_i = slot == DD_MAX_FEATURES + DD_MAX_COMBINED && (desc->n_image_combined > 0 || desc->n_image_features > 0);
    DD_REQUIRE(is_f || is_c || is_i, "dd_loss_previews: slots[%d] names slot %d, which the descriptor does not have", s, slot);
    sel.slots[s] = (unsigned char)slot;
  }
  sel.n_images = n_images;
  sel.n_slots = n_slots;
  sel.n_panels = 0;
  for (int bit = 0; bit < PV_PANELS; ++bit)
    if (panels & (1 << bit)) sel.panel[sel.n_panels++] = (unsigned char)bit;
  const int groups = (W + PV_PIX - 1) / PV_PIX;
  const long total = (long)n_slots * n_images * H * sel.n_panels * groups;
  const long blocks = (total + 255) / 256;
  DD_REQUIRE(blocks <= 0x7fffffffl, "dd_loss_previews: %ld workgroups do not fit a grid", blocks);
  hipLaunchKernelGGL(loss_previews_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *desc, sel, B, H, W, groups, total,
                     thresholds, exposure, error_gain, out);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
