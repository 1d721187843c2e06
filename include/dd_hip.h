/*
 * dd_hip.h -- C ABI of libdd_hip.so: hand-written CDNA4 (gfx950) HIP kernels for the conv hot
 * path of DeepBlender/DeepDenoiser.
 *
 * The reference has no FFI/plugin interface (it is pure Python on TensorFlow 1.x); its seams are
 * Python call signatures.  Each entry point below names the reference op-level seam it replaces
 * (file:line relative to /root/reference).  Conventions:
 *   - caller (PyTorch host) owns every buffer; the library never allocates or frees device memory
 *     and keeps no global state; all work is enqueued on the passed hipStream_t; no implicit sync;
 *   - activations are NHWC; a tensor is (pointer, ld) where ld = channel stride of one pixel in
 *     ELEMENTS (so concat buffers are written in place at a channel offset);
 *   - master weights / gradients / optimizer state are fp32 in TensorFlow variable layout:
 *     conv kernel HWIO [kh,kw,C_in,C_out]; transpose-conv kernel [kh,kw,C_out,C_in];
 *   - `dtype` selects the storage type of activations and packed weights: DD_F32 (parity path,
 *     exact-f32 MFMA), DD_BF16 (training throughput path, bf16 MFMA with fp32 accumulate) or
 *     DD_F16 (inference path of BASELINE cfg-5: fp16 MFMA, fp32 accumulate; range +-65504);
 *   - return 0 on success, negative dd_status otherwise; dd_last_error() gives the message of the
 *     calling thread's last failure.  No exceptions cross the ABI.
 */
#ifndef DD_HIP_H
#define DD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dd_stream; /* hipStream_t */

enum dd_dtype { DD_F32 = 0, DD_BF16 = 1, DD_F16 = 2 };

enum dd_status {
  DD_OK = 0,
  DD_ERR_INVALID = -1,  /* bad argument / unsupported shape */
  DD_ERR_LAUNCH = -2    /* HIP launch error */
};

/* flags of dd_conv_igemm / dd_conv_wgrad */
enum dd_conv_flags {
  DD_IN_RELU = 1,       /* operand is relu(x) (pre-activation convs: Tiramisu.py:33, MultiScalePrediction.py:87) */
  DD_OUT_RELU = 2,      /* y = relu(.) (tf.layers activation=tf.nn.relu) */
  DD_ACCUM = 4,         /* y += result (gradient accumulation for multi-consumer tensors) */
  DD_PIXSHUF = 8,       /* 2x2/s2 transpose-conv forward: n=(a,b,co) scattered to (2y+a,2x+b,co) */
  DD_GATHER2X2 = 16     /* 2x2/s2 gather: tap (a,b) reads input pixel (2y+a,2x+b) (transpose-conv dgrad/wgrad) */
};

const char* dd_version(void);
const char* dd_last_error(void);

/* ---- weight packing: fp32 master (TF layout) -> MFMA operand layout [taps][n_pad][k_pad] of `dtype`.
 * dst[t][n][k] = src[tsrc*s_tap + n*s_n + k*s_k], tsrc = tap_flip ? taps-1-t : t; zero padded. */
int dd_pack_weights(const float* src, void* dst, int dtype, int taps, int n, int k, int n_pad, int k_pad,
                    long s_tap, long s_n, long s_k, int tap_flip, dd_stream stream);

/* all layers in ONE launch: `table` is a device array of n records */
/* dst_ld / dst_tap_stride (elements; 0 = k_pad / n_pad * k_pad): the record fills the [n_pad][k_pad] corner of every tap of a WIDER image
 * ([taps][n_pad][dst_ld]) -- several records stack their reductions side by side in one operand (the gather-form data gradient of dd_conv3x3_ks) */
typedef struct { const float* src; void* dst; int taps, n, k, n_pad, k_pad, tap_flip; long s_tap, s_n, s_k; long dst_ld, dst_tap_stride; } dd_pack_desc;
int dd_pack_weights_batched(const dd_pack_desc* table, int n_layers, int dtype, dd_stream stream);

/* ---- implicit-GEMM convolution on MFMA (forward and data-gradient of every conv-like layer).
 * Replaces tf.layers.conv2d 3x3/1x1 SAME (UNet.py:29-31; Tiramisu.py:35-37,50-52,77-79;
 * Architecture.py:238-243; MultiScalePrediction.py:64-66,73-75,88-90), tf.layers.conv2d_transpose
 * 2x2/s2 (UNet.py:56-58) and, with flipped/transposed packed weights, their TF-autodiff input gradients.
 *   y[b,p,n] = epi( sum_{t,k} in(x)[b, map_t(p), k] * wp[t][n][k] + bias[n] + res[b,p,n] )
 * taps: 9 (3x3, pad 1), 1, or 4 with DD_GATHER2X2.  epi: optional relu, then *(mask>0), then +y if DD_ACCUM. */
typedef struct {
  const void* x; int ldx; int cin;     /* input [B,Hin,Win,*]; cin = valid channels (multiple of 16 bytes) */
  const void* wp; int k_pad; int n_pad;/* packed weights [taps][n_pad][k_pad] */
  const float* bias; int nbias;        /* fp32 bias and its length (nbias <= n), or NULL */
  const void* res; int ldres;          /* residual added before activation, or NULL */
  const void* mask; int ldmask;        /* y *= (mask > 0), or NULL (ReLU backward fused into the producer) */
  void* y; int ldy; int n;             /* output channels actually stored (n <= n_pad, n % 4 == 0; DD_PIXSHUF: cout = n / 4 a multiple of 16 bytes) */
  int B, H, W;                         /* GEMM-row pixel grid: output grid, except DD_PIXSHUF where it is the input grid */
  int taps; int flags; int dtype;
} dd_conv_args;
int dd_conv_igemm(const dd_conv_args* a, dd_stream stream);
/* Number of dd_conv_igemm calls this process routed to the wide 1x1 GEMM kernel (csrc/dd_conv_pw.hip: taps == 1, 2-byte storage, more than
 * 64 output channels, no residual operand, at least DD_CONV_PW_MIN_PIXELS = 32 768 pixels; DD_CONV_PW=0 turns the route off).  Tests use it
 * to assert that the kernel they mean to check is the one that ran. */
long dd_conv_pw_count(void);
long dd_wgrad_pw_count(void);   /* ... and dd_conv_wgrad calls routed to its weight-gradient counterpart (taps == 1, m or n above 64 channels) */
/* The same for EVERY kernel dd_conv_igemm, dd_conv3x3_ks and dd_conv_wgrad may route a call to: a host-side count per route, incremented next
 * to the launch it counts (no kernel, launch geometry or dispatch rule depends on it).  dd_conv_route_count(route) is the number of launches
 * this process sent down that route; -1 for a route it does not know.  Tests name the route a case must take and assert that exactly that
 * counter moved. */
enum dd_conv_route {
  DD_ROUTE_IGEMM_RESIDENT = 0,  /* conv_igemm_kernel, weights resident in LDS (csrc/dd_conv_igemm.hip) */
  DD_ROUTE_IGEMM_STREAMED,      /* conv_igemm_kernel, weights streamed slab by slab */
  DD_ROUTE_IGEMM_WS,            /* conv_igemm_ws_kernel (wave-specialised, 2-byte storage) */
  DD_ROUTE_RW_6_2,              /* conv_rw_kernel: 65..96 input channels, 6 compute + 2 I/O waves, any epilogue (csrc/dd_conv_rw.hip) */
  DD_ROUTE_RW12,                /* conv_rw8_kernel<KC = 3, 12 waves>: 65..96 input channels, bias / ReLU */
  DD_ROUTE_RW12_MASK,           /* ... with the ReLU-backward mask tile */
  DD_ROUTE_RW12_RES,            /* ... with a residual operand */
  DD_ROUTE_RW8_KC2,             /* conv_rw8_kernel<KC = 2>: 17..64 input channels */
  DD_ROUTE_RW8_KC4,             /* conv_rw8_kernel<KC = 4>: 97..128 input channels */
  DD_ROUTE_RW8_KC4_MASK,        /* ... with the ReLU-backward mask tile */
  DD_ROUTE_PW,                  /* conv_pw_kernel from dd_conv_igemm (csrc/dd_conv_pw.hip) */
  DD_ROUTE_KS,                  /* conv_ks_kernel (csrc/dd_conv_ks.hip) */
  DD_ROUTE_KS_PW_TAPS,          /* dd_conv3x3_ks routed to conv_pw_kernel's tap form (dd_conv_pw_taps_launch) */
  DD_ROUTE_WGRAD_DMA,           /* wgrad_dma_kernel, plain form (csrc/dd_conv_wgrad.hip) */
  DD_ROUTE_WGRAD_REG,           /* wgrad_kernel (register-staged) */
  DD_ROUTE_WGRAD_PW,            /* wgrad_pw_kernel from dd_conv_wgrad (csrc/dd_conv_pw.hip) */
  DD_ROUTE_WGRAD_STACKED,       /* wgrad_dma_kernel, stacked dense-block form */
  /* sub-counts: launches ALREADY counted under a route above that took a narrower instantiation of its kernel */
  DD_ROUTE_RW8_K32,             /* of DD_ROUTE_RW8_KC2: conv_rw8_kernel<KC = 1>, 17..32 input channels in a 32-channel weight image (DD_CONV_RW8_K32=0: none) */
  DD_ROUTE_COUNT
};
long dd_conv_route_count(int route);

/* ---- weight gradient on MFMA: out[t][m][n] += sum_{b,p} in(P)[b,map_t(p),m] * Q[b,p,n]   (fp32 atomics)
 * conv2d:            P = layer input x, Q = pre-activation output gradient -> out = dKernel HWIO
 * conv2d_transpose:  P = output gradient (fine grid, DD_GATHER2X2), Q = layer input -> out = dKernel [a,b,co,ci]
 * Replaces the TF-autodiff filter gradients behind AdamOptimizer.minimize (Training.py:701-702). */
typedef struct {
  const void* p; int ldp; int m;       /* P operand and its logical channel count (= out dim m) */
  const void* q; int ldq; int n;       /* Q operand and its logical channel count (= out dim n); channels up to the next
                                          multiple of 16 bytes must be readable and zero in both operands */
  float* out;                          /* [taps][m][n] fp32, accumulated atomically (zero it first) */
  float* bias_out; int bias_mode;      /* fused bias gradient (fp32 atomics): 0 none, 1 = column sums of Q -> bias_out[n] (conv2d),
                                          2 = column sums of P -> bias_out[m] (conv2d_transpose) */
  int B, H, W;                         /* grid of Q (the reduction pixels) */
  int taps; int flags; int dtype;
  int ksplit;                          /* number of reduction splits (0 = choose) */
  /* Stacked form (round 5; taps = 9, 2-byte storage): the weight gradients of ALL convs of a Tiramisu dense block (Tiramisu.py:26-41) in one
   * launch.  Conv j reads the prefix [0, stack_m0 + j * stack_width) of the block's buffer and appends stack_width channels, so the output
   * gradients of the stack_blocks convs are ONE contiguous channel range: Q = that range (n = stack_blocks * stack_width), P = the longest
   * prefix (m = stack_m0 + (stack_blocks - 1) * stack_width).  Column block j of the product, rows below its conv's own input width, is conv j's
   * gradient: stack_out[j] [taps][stack_m0 + j * stack_width][stack_width] and, with bias_mode = 1, stack_bias[j] [stack_width] (fp32 atomics);
   * out / bias_out are not used.  stack_blocks = 0: the plain form above. */
  int stack_blocks; int stack_width; int stack_m0;
  float* stack_out[8]; float* stack_bias[8];
} dd_wgrad_args;
int dd_conv_wgrad(const dd_wgrad_args* a, dd_stream stream);

/* ---- fused backward of a 3x3 SAME conv2d (stride 1): the data gradient (Conv2DBackpropInput + the ReluGrad of the layer's input) AND the
 * weight / bias gradients (Conv2DBackpropFilter, BiasAddGrad) that TensorFlow's autodiff emits for tf.layers.conv2d (Training.py:701-702 over
 * UNet.py:38-48), from ONE pass over dy and x (dd_conv_igemm + dd_conv_wgrad fetch each of them twice).  bf16 / f16 storage.  With a data
 * gradient: cout <= 64 in one launch (64 input channels per workgroup column), 65 <= cout <= 96 in one launch of the kernel that gives a
 * workgroup a 32-channel third of the input against all output channels (round 6: the U-Net's 64 x 64 level, UNet.py:25-36); wider layers run
 * as one launch per 64 output channels, the later ones accumulating into dx.
 *   dx[p][ci] = (use_mask ? x[p][ci] > 0 : 1) * sum_{t,co} wd[t][ci][co] * dy[p + off(t)][co]      (accumulate != 0: added to the existing dx)
 *   dw[t][ci][co] += sum_p x[p + off(t)][ci] * dy[p][co]     (TensorFlow kernel layout [3][3][cin][cout], fp32 atomics: zero it first)
 *   db[co] += sum_p dy[p][co]                                  (optional) */
typedef struct {
  const void* dy; int ld_dy; int cout; /* gradient of the layer's output [B,H,W,ld_dy]; channels up to the next multiple of 8 readable and zero */
  const void* x; int ld_x; int cin;    /* the layer's input [B,H,W,ld_x] (weight-gradient operand and ReLU mask of dx) */
  const void* wd; int n_pad; int k_pad;/* data-gradient weights as dd_pack_weights lays them out for dd_conv_igemm: [9][n_pad (ci)][k_pad (co)] */
  void* dx; int ld_dx;                 /* [B,H,W,ld_dx]; NULL (then wd may be NULL too, and cout may exceed 64): only dw / db are computed */
  float* dw; float* db;                /* db may be NULL */
  int B, H, W;
  int use_mask; int accumulate; int dtype;
} dd_conv_bwd_args;
int dd_conv3x3_bwd(const dd_conv_bwd_args* a, dd_stream stream);
/* the weight / bias gradients (dx = NULL) of n <= 4 layers on the SAME [B, H, W] grid as one launch (round 5: the 128-channel layers of the U-Net's
 * coarsest level -- each problem gets a share of the workgroups with more tiles apiece, i.e. fewer fp32 atomics per problem and n - 1 launch
 * boundaries fewer).  a: HOST array of n descriptors. */
int dd_conv3x3_bwd_multi(const dd_conv_bwd_args* a, int n, dd_stream stream);

/* ---- 2x2 / stride-2 transposed convolution (tf.layers.conv2d_transpose(filters, 2, strides=2), UNet.py:54-59) as streaming kernels: the
 * forward (+ bias, ReLU), and the data + weight + bias gradients of TensorFlow's autodiff (Training.py:701-702) in ONE launch.  bf16 / f16
 * storage, cin <= 128, cout a multiple of 16 (<= 96 forward, <= 128 backward: 65..96 one launch over two 64-channel slices, more as consecutive launches over blocks of 64; dx is rounded per block of 64 either way).  x [B,H,W,ld_x], y / dy [B,2H,2W,ld_y];
 * kernel K[a][b][co][ci] (TensorFlow layout [2][2][cout][cin]):
 *   forward : y[2i+a][2j+b][co] = act(bias[co] + sum_ci x[i][j][ci] K[a][b][co][ci]);  w = dd_pack_weights layout [4*cout -> n_pad][k_pad (ci)]
 *   backward: dx[i][j][ci] = (use_mask ? x > 0 : 1) * sum_{a,b,co} dy[2i+a][2j+b][co] K[a][b][co][ci]   (accumulate: added to dx);
 *             dw[a][b][co][ci] += sum_{i,j} dy[2i+a][2j+b][co] x[i][j][ci];  db[co] += sum dy (db may be NULL); fp32 atomics: zero them first;
 *             w = the data-gradient pack [4][n_pad (ci)][k_pad (co)] */
typedef struct {
  const void* x; int ld_x; int cin;
  void* y; int ld_y; int cout;         /* forward: output; backward: dy (read only) */
  const void* w; int n_pad; int k_pad;
  const float* bias; int relu;         /* forward only */
  void* dx; int ld_dx; float* dw; float* db; int use_mask; int accumulate;      /* backward only */
  int B, H, W;                         /* INPUT grid */
  int dtype;
} dd_convt_args;
int dd_convt2x2_fwd(const dd_convt_args* a, dd_stream stream);
int dd_convt2x2_bwd(const dd_convt_args* a, dd_stream stream);
/* Number of dd_convt2x2_bwd calls this process ran as ONE launch of the two-slice kernel (65 <= cout <= 96; DD_CONVT_BWD_WIDE=0: none, those
 * layers run as two launches).  dx is bit-identical either way, so tests read the path here. */
long dd_convt_bwd_wide_count(void);

/* ---- K-streamed 3x3 convolution for deep reductions and few output channels: the dense blocks of the Tiramisu backbone
 * (tf.layers.conv2d over the growing concat, Tiramisu.py:26-41: K = 9 x up to 1 088 channels, 16 ... 128 new channels) and its 3x3 / stride-2
 * transposed convolution (tf.layers.conv2d_transpose(filters, 3, strides=2, padding='same'), Tiramisu.py:60-65).  bf16 / f16 storage.
 *   mode 0: y[p][n0 + c] = act(bias[n0 + c] + sum_{t,ci} w[t][n0 + c][ci] * in(x[p + off(t)][ci])),  c < n,  in = relu if DD_IN_RELU;
 *           w = the dd_pack_weights image [9][n_pad][k_pad] dd_conv_igemm takes, x [B,H,W,ldx], y [B,H,W,ldy] (a channel view of a concat buffer).
 *   mode 1..4: output parity (py, px) = ((mode-1)/2, (mode-1)%2) of the transposed conv (o = 2i + a, rows / columns 2H, 2W dropped):
 *           y[2i+py][2j+px][n0 + c] = act(bias + sum over the taps a = py, b = px (mod 2) of x[i - a/2][j - b/2][ci] K[a][b][n0 + c][ci]),
 *           y [B,2H,2W,ldy]; w = the image dd_pack_weights builds for the zero-stuffed form of the same layer ([9][n_pad][k_pad], taps flipped):
 *           the four parities together ARE the layer, with the 9 real taps instead of 36;
 *   mode 5: all four parities in one launch.
 * One call covers output channels [n0, n0 + n) (mode 5: n <= 64 + 63): whole blocks of 64 channels and the remainder (32 / 16-channel tiles: a
 * 96-channel layer = 64 + 32), and the parities, run as sub-problems of ONE grid (blockIdx.y); the input is re-read per block, from L2.
 * DD_ACCUM (mode 0) is the data gradient of a Tiramisu dense block in GATHER form (TF autodiff of Tiramisu.py:26-41 behind Training.py:701-702):
 * the gradient of a channel range of the block's buffer receives the contributions of ALL later convs of the block in one launch -- their output
 * gradients are one contiguous channel range of the gradient buffer (= x, the reduction), wp the stacked transposed / flipped kernels
 * (dd_pack_weights_batched with dst_ld) -- masked by the ReLU the consumers apply on read, added to what is already stored, rounded once. */
typedef struct {
  const void* x; int ldx; int cin;
  const void* wp; int n_pad; int k_pad;
  const float* bias; int nbias;        /* bias[c] for c < nbias; NULL: none */
  void* y; int ldy;
  int n0; int n;
  int B, H, W;                         /* INPUT grid */
  int mode; int flags; int dtype;      /* flags: DD_IN_RELU (mode 0 only) | DD_OUT_RELU, or DD_ACCUM alone (gather-form data gradient, below) */
  const void* mask; int ldmask;        /* DD_ACCUM: y[p][n0+c] += (mask[p][n0+c] > 0) * sum  -- no bias, no activation, rounded once */
} dd_conv_ks_args;
int dd_conv3x3_ks(const dd_conv_ks_args* a, dd_stream stream);

/* column sums: out[c] += sum_rows x[row*ld + c]  (bias gradients; embedding-row gradients) */
int dd_colsum(const void* x, int ld, int c, long rows, float* out, int dtype, dd_stream stream);
/* the same over n_segments (<= 64) consecutive segments of rows_per_segment rows in one launch: out[out_row[s]*out_ld + ch] += the sum over
 * segment s (the embedding-row gradients of FeatureFlags.feature_flags, FeatureFlags.py:57-67: one row per tuple, tiled over the tuple's images).
 * out_row is a HOST table; c <= 8 16-byte vectors of the storage type (64 bf16 / fp16, 32 f32 channels), x 16-byte aligned, ld a multiple of a vector. */
int dd_colsum_segments(const void* x, int ld, int c, long rows_per_segment, int n_segments, float* out, int out_ld, const int* out_row,
                       int dtype, dd_stream stream);

/* ---- max pooling, TF SAME (UNet.py:42-44 3x3/s2; Tiramisu.py:55-57 2x2/s2); idx = window argmax (uint8).
 * relu_mask != 0: x is a ReLU output whose backward mask (x > 0) is folded into idx (255 = the window maximum is not positive, no
 * gradient), so dd_maxpool_bwd can be called with mask == NULL.  idx == NULL: forward only (inference), no argmax plane is stored.
 * idx code: a * pool + b for cell (a, b) of the window, padded cells counted; the FIRST maximum in row-major window order wins (as TF).
 * 16-byte vectors: C and every ld multiples of 8 (bf16 / fp16) or 4 (f32), x, y, dy, dx, mask 16-byte aligned, idx 8- / 4-byte aligned;
 * anything else returns -1 before a launch. */
int dd_maxpool_fwd(const void* x, int ldx, void* y, int ldy, uint8_t* idx, int C, int B, int H, int W,
                   int pool, int stride, int relu_mask, int dtype, dd_stream stream);
/* dx (+)= scatter(dy) masked by (mask>0) if mask != NULL */
int dd_maxpool_bwd(const void* dy, int lddy, const uint8_t* idx, void* dx, int lddx, const void* mask, int ldmask,
                   int C, int B, int H, int W, int pool, int stride, int accumulate, int dtype, dd_stream stream);

/* ---- f x f average pooling, stride f, fp32 (MultiScalePrediction.scale_down, MultiScalePrediction.py:11-13) */
int dd_avgpool(const float* x, int ldx, float* y, int ldy, int C, int B, int H, int W, int f, dd_stream stream);

/* ---- input pipeline (FeatureStandardization.standardize Architecture.py:39-46; FeatureEngineering.variance
 * FeatureEngineering.py:57-70): src [B,H,W,cs] fp32 (cs in {1,3}) -> dst [B,H,W,ldd] fp32 =
 * {3 standardized channels (1-ch sources replicated, SourceEncoder.py:49-51), local variance (1 channel, or cs if not compressed)}. */
typedef struct {
  int use_log1p; float mean; float inv_std;      /* standardize */
  int use_variance; int variance_before; int mode_neighbor; int relative; int compress; float epsilon;
} dd_feature_params;
int dd_prepare_feature(const float* src, int cs, float* dst, int ldd, const dd_feature_params* fp, int B, int H, int W, dd_stream stream);

/* channel gather/concat into the network input (SourceEncoder.prepare_neural_network_input, SourceEncoder.py:29-79,
 * incl. the embedding broadcast of FeatureFlags.feature_flags, FeatureFlags.py:50-69).
 * table: n_tuples x n_entries device records; dst [n_tuples*B,H,W,ld] of dtype, channels >= used ones zeroed up to c_pad. */
typedef struct { const float* src; int pixel_stride; int batch_stride_pixels; int nch; int dst_ch; } dd_gather_entry;
int dd_gather_input(const dd_gather_entry* table, int n_tuples, int n_entries, void* dst, int ld, int c_pad,
                    int B, int H, int W, int dtype, dd_stream stream);

/* prepare + gather in ONE launch (bf16 / fp16 / f32): every entry of a tuple is computed from the raw pass and written straight into the
 * network input; no fp32 staging plane.  kind 0: a render pass (src [B,H,W,cs] fp32, standardised per `fp`, local variance appended: nch = 3 +
 * variance channels); kind 1: a vector of nch floats broadcast over the image (the embedding row of FeatureFlags.feature_flags,
 * FeatureFlags.py:50-69); kind 2: a plane [B,H,W,nch] copied as it is (one-hot flags).  std_out (kind 0, optional): the entry's standardised
 * channels in fp32 [B,H,W,ld_std] -- the source KernelPredictor filters (Architecture.py:262-265). */
typedef struct { const float* src; int cs; int kind; dd_feature_params fp; int nch; int dst_ch; float* std_out; int ld_std; } dd_assemble_entry;
int dd_assemble_input(const dd_assemble_entry* table, int n_tuples, int n_entries, void* dst, int ld, int c_pad,
                      int B, int H, int W, int dtype, dd_stream stream);
/* The same launch for full-frame inference (Prediction.py:380-427: every tile is an H x W window of the frame): the kind-0 entries' src are
 * whole frames [frame_h, frame_w, cs] fp32 and image b of the batch is the window at (origins_yx[2b], origins_yx[2b+1]) (device table,
 * [B][2] int32, the tile plan's origins) -- read in place, mirrored at the WINDOW's border exactly as a copied tile would be.  Replaces one
 * dd_extract_tiles per render pass and the tile copies it wrote.  kind-1 / kind-2 entries as in dd_assemble_input. */
int dd_assemble_input_frames(const dd_assemble_entry* table, int n_tuples, int n_entries, void* dst, int ld, int c_pad,
                             int B, int H, int W, int dtype, const int* origins_yx, int frame_h, int frame_w, dd_stream stream);

/* ---- kernel prediction (KernelPrediction.kernel_prediction, KernelPrediction.py:11-63): softmax over k*k logits,
 * symmetric pad, per-pixel k x k filter of the 3-channel source.
 * All four entries REFUSE (DD_ERR_INVALID, dd_last_error names the reason, nothing is launched): ksize other than 3, 5, 7; a dtype that
 * is none of DD_F32 / DD_BF16 / DD_F16; B, H or W <= 0; H or W below the pad (ksize - 1) / 2 -- the symmetric index mirrors once, so a
 * smaller image would be read outside itself, and TensorFlow's SYMMETRIC pad rejects such shapes as well; B * H * W >= 2^31;
 * ldsrc, ldo (and, backward, lddo) < 3; ldl (ldw) < k*k; backward: dl_pad > lddl or dl_pad < k*k (channels 0..k*k-1 of a d logits
 * row are always written, k*k..dl_pad-1 are set to +0, anything beyond dl_pad is left alone); null pointers. */
int dd_kpcn_fwd(const float* src, int ldsrc, const void* logits, int ldl, float* out, int ldo,
                int B, int H, int W, int ksize, int dtype, dd_stream stream);
int dd_kpcn_bwd(const float* src, int ldsrc, const void* logits, int ldl, const float* dout, int lddo,
                void* dlogits, int lddl, int dl_pad, int B, int H, int W, int ksize, int dtype, dd_stream stream);
/* The same with the logits computed IN the kernel, in fp32, from the input of AdjustNumberOfChannels' second 1x1 layer (Architecture.py:237-244):
 * logits[t] = bb[t] + sum_k hid[k] * wb[k * ldw + t], hid [B,H,W,ldh] of dtype (kh channels, post-ReLU), wb / bb the fp32 master variables
 * (TensorFlow layout [kh][ldw]; a COMBINED tuple's member j passes wb + j*k*k, bb + j*k*k).  What the layer-wise head of the half-precision
 * programs uses: a logit of magnitude 50 rounded to bf16 moves its softmax weight by up to 13 %.  The backward writes d logits (dtype) for the
 * weight / data gradient launches of that layer, exactly as dd_kpcn_bwd does. */
int dd_kpcn_hidden_fwd(const float* src, int ldsrc, const void* hid, int ldh, int kh, const float* wb, int ldw, const float* bb,
                       float* out, int ldo, int B, int H, int W, int ksize, int dtype, dd_stream stream);
int dd_kpcn_hidden_bwd(const float* src, int ldsrc, const void* hid, int ldh, int kh, const float* wb, int ldw, const float* bb,
                       const float* dout, int lddo, void* dlogits, int lddl, int dl_pad, int B, int H, int W, int ksize, int dtype, dd_stream stream);

/* ---- the whole kernel-prediction head of one scale as ONE launch each way: AdjustNumberOfChannels.predict (Architecture.py:237-244:
 * 1x1 conv C -> K + ReLU, 1x1 conv K -> K) + KernelPredictor.predict / KernelPrediction.kernel_prediction (Architecture.py:260-289,
 * KernelPrediction.py:11-63) with K = ksize * ksize (one tuple member), and their TF-autodiff gradients.  bf16 / fp16 storage only.
 * Weights are the fp32 master variables in TensorFlow layout (wa [C][K], wb [K][K]).  The backward recomputes hid / logits from x, so
 * the forward stores nothing; dx (storage type) is masked by x > 0 (x is a ReLU output) and optionally accumulated into; the weight /
 * bias gradients are ADDED to their fp32 arena slots.  x 16-byte aligned with ldx % 8 == 0, dx 8-byte aligned with ld_dx % 4 == 0;
 * H, W >= (ksize - 1) / 2; N * H * W < 2^31 and H * W * ldsrc < 2^32 (pixels and tap offsets are 32-bit in the kernels). */
typedef struct {
  const void* x; int ldx; int C;           /* backbone output of this scale [N,H,W,ldx], C valid channels (C % 8 == 0, C <= 128) */
  const float* src; int ldsrc;             /* 3-channel source at this scale [N,H,W,ldsrc] fp32 */
  const float* wa; const float* ba; const float* wb; const float* bb;
  float* out; int ld_out;                  /* forward: prediction [N,H,W,ld_out] fp32 (3 channels) */
  const float* dout; int ld_dout;          /* backward: dL/d(out) fp32 */
  void* dx; int ld_dx; int accumulate_dx;  /* backward: dL/dx (storage type) */
  float* dwa; float* dba; float* dwb; float* dbb;
  int N, H, W, ksize, dtype;
} dd_head_args;
int dd_kpcn_head_fwd(const dd_head_args* a, dd_stream stream);
int dd_kpcn_head_bwd(const dd_head_args* a, dd_stream stream);
/* the backward of n <= 3 scales' heads (HOST array; one storage type and kernel size) as ONE launch: the scales are independent and the coarse
 * ones are mostly fixed cost (weight staging, the flush); side by side they share the device in proportion to their pixel counts (round 5) */
int dd_kpcn_head_bwd_multi(const dd_head_args* a, int n, dd_stream stream);

/* ---- multiscale compose (MultiScalePrediction.compose_scales, MultiScalePrediction.py:36-54) */
/* net input = concat(nearest_x2(small), fine), zero padded to c_pad channels */
int dd_compose_pack(const float* small, int lds, const float* fine, int ldf, void* dst, int ld, int c_pad,
                    int B, int H, int W, int dtype, dd_stream stream);
/* out = fine - w*up(avg2(fine)) + w*up(small), w = sigmoid(wl)  (wl = relu'd 1-channel net output) */
int dd_compose_blend_fwd(const float* small, int lds, const float* fine, int ldf, const void* wl, int ldw,
                         float* out, int ldo, int B, int H, int W, int dtype, dd_stream stream);
/* backward of the blend: dfine (overwritten), dsmall (overwritten or accumulated) and dwl (gradient at the pre-relu net output) */
int dd_compose_blend_bwd(const float* dout, int lddo, const float* small, int lds, const float* fine, int ldf,
                         const void* wl, int ldw, float* dsmall, int ldds, int accumulate_small, float* dfine, int lddf,
                         void* dwl, int lddw, int dw_pad, int B, int H, int W, int dtype, dd_stream stream);
/* backward of compose_pack: dsmall += sum_2x2 dnet[0:3]; dfine += dnet[3:6] */
int dd_compose_unpack_bwd(const void* dnet, int ld, float* dsmall, int ldds, float* dfine, int lddf,
                          int B, int H, int W, int dtype, dd_stream stream);

/* ---- the whole compose net of one scale transition as ONE launch (MultiScalePrediction.compose_scales, MultiScalePrediction.py:36-93):
 * out = fine - w * up(avg_pool2(fine)) + w * up(small),  w = sigmoid(relu(1x1(a3))),  a3 = two residual blocks over relu(1x1([up(small) | fine])).
 * Weights are the fp32 master variables of scope 'reused_compose_scales' in TensorFlow layout (conv2d: [6][24]; conv2d_1..4: HWIO
 * [3][3][24][24]; conv2d_5: [24][1]).  bf16 / fp16 storage only (f32 runs layer by layer through dd_conv_igemm).
 * Training: the activations the layer-wise backward reads are stored when their pointers are non-NULL -- netin (the packed 6-channel
 * input, ld >= 8), act[0..4] = a1, relu(r1), a2, relu(r3), a3 (24 channels, ld >= 24, ld % 8 == 0), wl = relu(1x1(a3)) (1 channel). */
typedef struct {
  const float* small; int ld_small;        /* [N, H/2, W/2, ld] fp32 */
  const float* fine; int ld_fine;          /* [N, H, W, ld] fp32 */
  float* out; int ld_out;                  /* [N, H, W, ld] fp32 */
  const float* w_in; const float* b_in;
  const float* w_res[4]; const float* b_res[4];
  const float* w_out; const float* b_out;
  void* save_netin; int ld_netin;
  void* save_act[5]; int ld_act[5];
  void* save_wl; int ld_wl;
  int N, H, W, dtype;
} dd_compose_args;
int dd_compose_net_fwd(const dd_compose_args* a, dd_stream stream);
/* Geometry dd_compose_net_fwd's row-streaming kernel (csrc/dd_compose_stream.hip) uses for an [N, H, W] launch on `cus` compute units:
 * out8 = {frame width, rows per step, 32-pixel tasks per row, column strips, strip output width, band height, bands per image,
 * virtual rows per band}.  Host-only (no device work); for tests and tools. */
int dd_compose_stream_plan(int N, int H, int W, int cus, int* out8);

/* Backward of dd_compose_net_fwd in ONE launch (TF autodiff of the same lines behind Training.py:701-702): d_fine is written, d_small is
 * written or accumulated into, every weight / bias gradient is ADDED to its fp32 arena slot (TensorFlow variable layout) with one
 * atomic per element per workgroup.  act[0..4], wl: the tensors the forward stored.  dout: dL/d(out), fp32. */
typedef struct {
  const float* small; int ld_small;
  const float* fine; int ld_fine;
  const float* dout; int ld_dout;
  const void* act[5]; int ld_act[5];
  const void* wl; int ld_wl;
  const float* w_in; const float* w_res[4]; const float* w_out;
  float* d_small; int ld_dsmall; int accumulate_small;
  float* d_fine; int ld_dfine;
  float* dw_in; float* db_in; float* dw_res[4]; float* db_res[4]; float* dw_out; float* db_out;
  int N, H, W, dtype;
  void* scratch; long scratch_bytes;       /* optional: >= dd_compose_bwd_scratch_bytes(N, H, W) bytes, 16-byte aligned (see below) */
} dd_compose_bwd_args;
int dd_compose_net_bwd(const dd_compose_bwd_args* a, dd_stream stream);
/* With `scratch` the backward runs as two row-streaming launches (csrc/dd_compose_stream_bwd.hip): the data-gradient chain, which parks the
 * four 24-channel gradient tensors and dz6 in scratch, then the weight gradients, which read every stored activation and parked gradient once.
 * Needs act[] rows of exactly 24 channels (ld_act == 24).  Without scratch (NULL): the 16x16-tile kernel of csrc/dd_compose.hip. */
long dd_compose_bwd_scratch_bytes(int N, int H, int W);

/* ---- inverse standardization (Architecture.py:48-55, Utilities.py:6-7), in place capable */
int dd_invert_std_fwd(const float* x, float* y, long n, int use_log1p, float mean, float std, dd_stream stream);
/* dx = dy * d(invert)/dx evaluated at the standardized value x */
int dd_invert_std_bwd(const float* x, const float* dy, float* dx, long n, int use_log1p, float mean, float std, dd_stream stream);

/* ---- loss head (LossDifference.difference LossDifference.py:15-35; BaseFeatureTraining.mean / variation_mean / loss
 * Training.py:126-129,141-176,210-243,304-348; Combined*FeatureTraining.initialize Training.py:420-437,475-495): per-pixel evaluation of
 * every feature loss, combined-feature loss (color*(direct+indirect)) and combined-image loss at one scale, fused with its own backward.
 * Each of the three levels has a MEAN term (difference of the values) and a VARIATION term (difference of the horizontal and vertical
 * finite differences x[.,j+1]-x[.,j], x[i+1,.]-x[i,.], averaged over all B*(H*(W-1)+(H-1)*W) pairs). */
#define DD_MAX_FEATURES 32
#define DD_MAX_COMBINED 8
typedef struct {
  int n_features;
  const float* pred[DD_MAX_FEATURES];    /* [B,H,W,pred_ld] internal prediction (1-channel passes use channel 0) */
  const float* target[DD_MAX_FEATURES];  /* [B,H,W,target_ld], first nch channels used */
  float* dpred[DD_MAX_FEATURES];         /* [B,H,W,3]; of a feature that carries a weight (its own, or through a combined / image term), or
                                            pred_std: overwritten, all 3 channels.  Of a feature that carries NO weight: left untouched by the
                                            flat-stream kernel and zeroed by the other two -- callers must not rely on either */
  int target_ld[DD_MAX_FEATURES];        /* pixel stride of target */
  int pred_ld[DD_MAX_FEATURES];          /* pixel stride of pred (3, or 4 when a source is echoed) */
  int nch[DD_MAX_FEATURES];
  float weight[DD_MAX_FEATURES];         /* mean-term weight incl. scale factor; the 1/(B*H*W) mean is applied inside */
  float var_weight[DD_MAX_FEATURES];     /* variation-term weight incl. scale factor */
  float masked_weight[DD_MAX_FEATURES];  /* masked-mean weight incl. scale factor (BaseFeatureTraining.masked_mean, Training.py:131-137) */
  int mask_feature[DD_MAX_FEATURES];     /* feature whose TARGET defines the mask (Conv2dUtilities.non_zero_mask of the corresponding colour pass) */
  int n_combined;
  int comb[DD_MAX_COMBINED][3];          /* feature indices of color, direct, indirect */
  float comb_weight[DD_MAX_COMBINED];
  float comb_var_weight[DD_MAX_COMBINED];
  float comb_masked_weight[DD_MAX_COMBINED];
  int comb_mask_feature[DD_MAX_COMBINED];
  int n_image_combined; int image_combined[DD_MAX_COMBINED];   /* indices into comb[] */
  int n_image_features; int image_features[DD_MAX_FEATURES];   /* indices into features */
  float image_weight;
  float image_var_weight;
  int kind;                              /* 1 DIFFERENCE, 2 ABSOLUTE, 3 SMOOTH_ABSOLUTE, 4 SQUARED, 5 SMAPE */
  float epsilon;
  const float* mask_sums;                /* device, [DD_MAX_FEATURES + DD_MAX_COMBINED]: sum of each source's mask over the batch (dd_loss_mask_sums);
                                            may be NULL when no masked weight is set */
  /* Optional fusion of FeaturePrediction.prediction_invert_standardization (Architecture.py:134-138, :47-55; Utilities.py:3-7) into the loss
   * launch, per feature; for every descriptor WITHOUT variation terms (features-only ones take the flat-stream kernel, descriptors with
   * combined / image / masked terms the per-pixel kernel; with a variation term dd_loss_head rejects pred_std: run dd_invert_std_fwd / _bwd
   * around it).  With pred_std[f] != NULL the launch reads the STANDARDIZED prediction x from
   * pred_std[f], stores p = sign(z) expm1|z| (inv_log1p) or z, z = x inv_std + inv_mean, to pred_inv[f] (what dd_invert_std_fwd stores),
   * and writes dL/dx (what dd_invert_std_bwd stores) to dpred[f] instead of dL/dp; pred[f] is not read. */
  const float* pred_std[DD_MAX_FEATURES];
  float* pred_inv[DD_MAX_FEATURES];
  int inv_log1p[DD_MAX_FEATURES];
  float inv_mean[DD_MAX_FEATURES];
  float inv_std[DD_MAX_FEATURES];
} dd_loss_desc;
/* mask_sums[src] = sum over [B,H,W] of sign(sum_c |target_c|) of the source's mask feature, for every source with a masked weight
 * (features first, then combined at DD_MAX_FEATURES + k).  The masked mean divides by this BATCH-global count (Training.py:131-137). */
int dd_loss_mask_sums(const dd_loss_desc* desc, int B, int H, int W, float* mask_sums, dd_stream stream);
/* loss_out[0] += total weighted loss of this scale; dpred written (see dd_loss_desc.dpred for features without a weight). desc is a HOST
 * struct (copied by value). */
int dd_loss_head(const dd_loss_desc* desc, int B, int H, int W, float* loss_out, float grad_scale, dd_stream stream);
/* dd_loss_head with the factor of dL/dprediction read from device memory when the kernel RUNS (*grad_scale_dev, in practice the `scale` word of
 * a dd_scaler_state): a captured hipGraph picks the current loss scale up on every replay.  Same kernels and the same multiply as the
 * by-value entry: dpred is bit-identical to dd_loss_head(..., the value at *grad_scale_dev, ...).  No host sync. */
int dd_loss_head_dscale(const dd_loss_desc* desc, int B, int H, int W, float* loss_out, const float* grad_scale_dev, dd_stream stream);
/* dd_loss_head launches so far, per kernel: path 0 the flat-stream kernel (features-only descriptors), 1 the per-pixel kernel (no variation
 * term), 2 the older kernel (everything else; DD_LOSS_SIMPLE=0 / DD_LOSS_GENERAL=0 send the first two here).  Host-side counter for tests, as
 * dd_conv_pw_count; -1 for any other path. */
long dd_loss_head_path_count(int path);

/* ---- MS-SSIM loss term (BaseFeatureTraining.ms_ssim Training.py:178-204, added ONCE with ms_ssim_weight alone at Training.py:231-232: no
 * multi-scale scale factor, always on predicted[0] / target[0]; tf.image.ssim_multiscale with max_val 1 and the THREE power factors
 * (0.0448, 0.2856, 0.3001), filter 11 x 11, sigma 1.5, k1 0.01, k2 0.03):
 *   term = weight * (1 - mean over images of MS),   MS = mean over channels of relu(cs_0)^0.0448 relu(cs_1)^0.2856 relu(ssim_2)^0.3001,
 * level k > 0 = the 2x2 / stride-2 average pool of level k-1, cs_k / ssim_k the means over the (h-10)(w-10) VALID filter positions.
 * The descriptor names the SOURCES of one scale-0 evaluation: a feature (FeatureTraining Training.py:374-392), a combined feature
 * color * (direct + indirect) (CombinedFeatureTraining.initialize Training.py:420-437) and the combined image = sum of its members
 * (CombinedImageFeatureTraining.initialize Training.py:475-495); every source with a positive weight is evaluated.  All tensors fp32 NHWC,
 * all arithmetic fp32.  Every used feature needs nch == 3 (Training.py:187-190 transposes anything else into an image 1 pixel high).
 * Every reduction has a fixed order (no atomics): loss and gradient are bit-identical from run to run.
 * Where relu clamps a factor (cs_k <= 0, an anti-correlated pair) MS of that image and channel is 0 as in TensorFlow; TensorFlow's own
 * gradient there is 0 * inf, OURS IS DEFINED AS 0 for that image and channel (finite).  A NaN in pred or target is NOT clamped away: it
 * reaches MS, loss_out and the gradient of that image and channel as in TensorFlow (a diverged run shows in the loss).
 * H and W must be multiples of 4 with min(H, W) / 4 >= 11 (TF refuses a level smaller than its filter; odd levels would need its symmetric pad). */
typedef struct {
  int n_features;
  const float* pred[DD_MAX_FEATURES];    /* [B,H,W,pred_ld], as dd_loss_desc */
  const float* target[DD_MAX_FEATURES];  /* [B,H,W,target_ld] */
  float* dpred[DD_MAX_FEATURES];         /* [B,H,W,3], ADDED to by dd_loss_msssim_bwd; NULL: no gradient wanted (a generated pass) */
  int target_ld[DD_MAX_FEATURES];
  int pred_ld[DD_MAX_FEATURES];
  int nch[DD_MAX_FEATURES];
  float ssim_weight[DD_MAX_FEATURES];    /* ms_ssim weight of the feature's own term; 0: none */
  int n_combined;
  int comb[DD_MAX_COMBINED][3];          /* feature indices of color, direct, indirect */
  float comb_ssim_weight[DD_MAX_COMBINED];
  int n_image_combined; int image_combined[DD_MAX_COMBINED];   /* indices into comb[] */
  int n_image_features; int image_features[DD_MAX_FEATURES];   /* indices into features */
  float image_ssim_weight;
} dd_loss_msssim_desc;
/* bytes of the scratch buffer (pooled levels, coarse gradients, per-tile partial sums, coefficients) for n_sources = the number of sources
 * with a positive weight; negative dd_status on a bad shape */
long dd_loss_msssim_scratch_bytes(int B, int H, int W, int n_sources);
/* loss_out[0] += sum of the weighted terms; leaves in scratch what dd_loss_msssim_bwd needs.  desc is a HOST struct.  No host sync. */
int dd_loss_msssim_fwd(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float* loss_out, dd_stream stream);
/* dpred += grad_scale * d term / d pred, routed through the combined product (d color += g (direct + indirect), d direct += g color,
 * d indirect += g color) and the image sum.  Same desc / scratch as the forward it follows on the same stream. */
int dd_loss_msssim_bwd(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float grad_scale, dd_stream stream);
/* dd_loss_msssim_bwd with grad_scale read from device memory when the kernels run (see dd_loss_head_dscale); bit-identical to the by-value entry. */
int dd_loss_msssim_bwd_dscale(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, const float* grad_scale_dev, dd_stream stream);
/* Tracked ms_ssim (track_ms_ssim of the statistics sections; add_tracked_metrics_to_dictionary Training.py:293-294 -> ms_ssim :178-204): the
 * forward kernels of dd_loss_msssim_fwd on the same scratch layout, but instead of adding a weighted term to a loss they leave
 *   ms_out[s * B + b] = MS of source s and image b (the mean over the 3 channels of the three-factor product)
 * for the sources with a POSITIVE weight in desc (the weight only selects: its value is not used), listed as features in index order, then
 * combined features, then the image.  The tracked scalar is 1 - mean over images of MS (Training.py:203).  dpred is not touched; the
 * scratch must not be the one a pending dd_loss_msssim_bwd still reads.  No host sync. */
int dd_loss_msssim_values(const dd_loss_msssim_desc* desc, int B, int H, int W, float* scratch, float* ms_out, dd_stream stream);

/* ---- tracked metrics (statistics / statistics_masked of Training.json: BaseFeatureTraining.add_tracked_metrics_to_dictionary
 * Training.py:283-302, add_tracked_summaries :246-265) of ONE scale.  Reads the sources of a dd_loss_desc -- pred / target, pred_ld /
 * target_ld, nch (1 or 3), comb, image_combined / image_features, mask_feature / comb_mask_feature, kind, epsilon; weights, dpred, mask_sums
 * and the pred_std fusion fields are ignored, pred[] must hold the final predictions -- and writes, for every source and EVERY IMAGE b,
 *   table[(slot * B + b) * 4 + 0] = sum over the image's pixels of the channel-summed LossDifference            (difference, Training.py:116-129)
 *   table[(slot * B + b) * 4 + 1] = sum over its H(W-1) horizontal and (H-1)W vertical pairs of the variation difference  (:139-176, :304-348)
 *   table[(slot * B + b) * 4 + 2] = sum of difference * mask                                                    (:121-124, :131-137)
 *   table[(slot * B + b) * 4 + 3] = sum of mask = non-zero mask of the target of mask_feature (0 when that is -1)   (:379-392, :434-437)
 * slot = f for feature f, DD_MAX_FEATURES + k for combined feature k, DD_MAX_FEATURES + DD_MAX_COMBINED for the combined image; rows of
 * sources the descriptor does not have are written as zeros.  table: DD_METRIC_SOURCES * B * 4 floats, 16-byte aligned, as is scratch
 * (>= dd_loss_metrics_scratch_bytes).  Per-image rows let the host leave the repeated examples of a padded batch out.  All arithmetic fp32;
 * every sum has a fixed order (no atomics): two runs give the same bits.  desc is a HOST struct (copied by value).  No host sync. */
#define DD_METRIC_SOURCES (DD_MAX_FEATURES + DD_MAX_COMBINED + 1)
long dd_loss_metrics_scratch_bytes(int B, int H, int W);
int dd_loss_metrics(const dd_loss_desc* desc, int B, int H, int W, float* scratch, float* table, dd_stream stream);

/* ---- TensorBoard histograms of the tracked differences (track_difference_histogram / track_variation_difference_histogram of the statistics
 * sections: BaseFeatureTraining.add_tracked_histograms, Training.py:267-281; tf.summary.histogram -> tensorflow/core/lib/histogram/histogram.cc)
 * (csrc/dd_histogram.hip).  A histogram RECORD is DD_HISTOGRAM_RECORD_BYTES(nb) bytes of device memory, 8-byte aligned:
 *   uint32 counts[nb]                                   bucket b counts limits[b-1] <= x < limits[b]  (Histogram::Add: upper_bound)
 *   at DD_HISTOGRAM_STATS_OFFSET(nb):  double min, max, sum, sum_squares;  uint64 num, nonfinite
 * limits: nb doubles in DEVICE memory, strictly increasing, the last one above every fp32 -- the table the host later writes as bucket_limit
 * (TensorFlow's default: 1551 entries); the device compares against it and never rebuilds it.  A NaN or +-inf value increments nonfinite and
 * touches nothing else.  An empty histogram has min = DBL_MAX, max = -DBL_MAX.  Counts are integer atomics, sum / sum_squares are added in
 * double in a fixed order, min / max do not depend on order: two runs give the same bits.  Records are OVERWRITTEN.  No host sync.  Counts are 32-bit: one call takes fewer
 * than 2^32 values (dd_loss_histograms: 2 B H W < 2^32).  The bucket search starts from a guess made for TensorFlow's default table and ends
 * in a binary search for any other table: exact for both, a few comparisons per value only for the default one. */
#define DD_HISTOGRAM_MAX_BUCKETS 4096
#define DD_HISTOGRAM_STATS_OFFSET(nb) ((((long)(nb) + 1) / 2) * 8)
#define DD_HISTOGRAM_RECORD_BYTES(nb) (DD_HISTOGRAM_STATS_OFFSET(nb) + 48)
#define DD_HISTOGRAM_VALUES_SCRATCH_BYTES 20480
#define DD_HISTOGRAM_MAX_CHUNKS 32
/* The binning primitive (what tf.summary.histogram does with the flat tensor it is given, Training.py:274): record = histogram of
 * values[0 .. n), n > 0 fp32 values, 4-byte aligned.  scratch: DD_HISTOGRAM_VALUES_SCRATCH_BYTES, 8-byte aligned. */
int dd_histogram_values(const float* values, long n, const double* limits, int nb, void* record, void* scratch, dd_stream stream);
/* The tracked histograms of ONE scale, from the sources of a dd_loss_desc read exactly as dd_loss_metrics reads them.  selection: HOST array
 * of n_records (slot, kind) pairs, slot as in the dd_loss_metrics table; record r (records + r * DD_HISTOGRAM_RECORD_BYTES(nb)) receives
 *   DD_HISTOGRAM_DIFFERENCE            the channel-summed LossDifference of every pixel, B*H*W values                     (Training.py:116-119, :274)
 *   DD_HISTOGRAM_VARIATION_DIFFERENCE  the H(W-1) horizontal and (H-1)W vertical pair differences of every image          (:139-176, :276)
 *   DD_HISTOGRAM_MASKED_DIFFERENCE     difference * non-zero mask of mask_feature's target, B*H*W values, zeros included  (:121-124, :279)
 * A masked difference needs mask_feature / comb_mask_feature >= 0 (the image has none); a pair may be selected once.  scratch:
 * >= dd_loss_histograms_scratch_bytes, 8-byte aligned.  Values are formed in fp32 like dd_loss_metrics'.  desc is a HOST struct (copied by
 * value). */
#define DD_HISTOGRAM_DIFFERENCE 0
#define DD_HISTOGRAM_VARIATION_DIFFERENCE 1
#define DD_HISTOGRAM_MASKED_DIFFERENCE 2
long dd_loss_histograms_scratch_bytes(int B, int H, int W, int n_records);
int dd_loss_histograms(const dd_loss_desc* desc, int B, int H, int W, const int* selection, int n_records, const double* limits, int nb,
                       void* records, void* scratch, dd_stream stream);

/* ---- image summaries: 8-bit previews of source | prediction | target | difference of ONE scale, rendered on the device
 * (csrc/dd_preview.hip; the reference writes no image summaries).  Reads the sources of a dd_loss_desc as dd_loss_metrics reads them -- pred /
 * target, pred_ld / target_ld, nch (1 or 3), comb, image_combined / image_features, kind, epsilon; weights, dpred, masks and the pred_std
 * fusion fields are ignored -- plus `source`: per feature the raw noisy pass [B,H,W,source_ld[f]], its first nch[f] channels used (HOST arrays
 * of n_features entries; may be NULL without the source panel).
 *   images : HOST, n_images batch indices 0 <= b < B (1 .. DD_PREVIEW_MAX_IMAGES, repeats allowed)
 *   slots  : HOST, n_slots source slots as in the dd_loss_metrics table (1 .. DD_METRIC_SOURCES)
 *   panels : bit mask of DD_PREVIEW_SOURCE / PREDICTION / TARGET / DIFFERENCE, P = the number of set bits
 * out: n_slots mosaics, each [n_images * H, P * W, 3] uint8 RGB: image row r is batch image images[r], panels run left to right in bit order.
 * A source / prediction / target panel pixel is the slot's value formed from that set of tensors (a feature's own channels, a 1-channel pass
 * replicated to gray; combined = color * (direct + indirect); image = sum of its members: the helpers of the loss kernels, one fp32 rounding
 * per operation), multiplied once by `exposure`.  The difference panel is gray: |channel-summed LossDifference(pred, target)| * error_gain.
 * A byte is the number of entries of `thresholds` (DEVICE, DD_PREVIEW_THRESHOLDS fp32, strictly increasing) that are <= the value: the host
 * owns the transfer function, the device only compares.  +inf gives 255, -inf 0; a NaN in any channel makes the pixel (255, 0, 255).
 * One launch, plain stores, every byte of the mosaics written exactly once and no other: two runs give the same bits.  A bad argument (a slot
 * the descriptor does not have, n_images / n_slots out of range, panels == 0, a NULL source with the source bit set, a NULL table) returns a
 * negative status without a launch.  desc is a HOST struct (copied by value).  No host sync. */
#define DD_PREVIEW_MAX_IMAGES 16
#define DD_PREVIEW_THRESHOLDS 255
#define DD_PREVIEW_SOURCE 1
#define DD_PREVIEW_PREDICTION 2
#define DD_PREVIEW_TARGET 4
#define DD_PREVIEW_DIFFERENCE 8
int dd_loss_previews(const dd_loss_desc* desc, const float* const* source, const int* source_ld, int B, int H, int W, const int* images, int n_images,
                     const int* slots, int n_slots, int panels, const float* thresholds, float exposure, float error_gain, unsigned char* out,
                     dd_stream stream);

/* ---- Adam, TensorFlow formulation (tf.train.AdamOptimizer, Training.py:701-702), flat arenas */
int dd_adam_step(float* params, const float* grads, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                 float eps, float grad_scale, dd_stream stream);

/* ---- dynamic loss scaling on the device (csrc/dd_loss_scale.hip).  One record of DEVICE memory per optimizer: the loss launches multiply
 * dL/dprediction by `scale` (dd_loss_head_dscale / dd_loss_msssim_bwd_dscale take &st->scale), and a step is
 *   dd_grads_nonfinite -> dd_adam_step_scaled -> dd_scaler_update
 * on one stream: the decision to skip an overflowed step, the scale and the Adam step counter never visit the host.  The host initialises the
 * record (scale > 0, the rest 0, or the values of a checkpoint) and may read it back whenever it is willing to wait. */
typedef struct {
  float scale;            /* current loss scale */
  int good_steps;         /* applied steps since the scale last changed */
  int found_nonfinite;    /* set by dd_grads_nonfinite, cleared by dd_scaler_update */
  int adam_t;             /* applied optimizer steps: the t of lr_t; skipped steps do not count */
  int skipped_total;      /* steps skipped because a gradient was inf / NaN */
} dd_scaler_state;
/* st->found_nonfinite |= (any of grads[0 .. n) is inf or NaN); a flag that is set stays set.  grads 16-byte aligned.  One read of the arena, no
 * write at all when every value is finite. */
int dd_grads_nonfinite(const float* grads, long n, dd_scaler_state* st, dd_stream stream);
/* dd_adam_step behind the device-side decision: writes NOTHING when st->found_nonfinite is set; otherwise the gradient is
 * grads * grad_scale / st->scale and lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) with t = st->adam_t + 1, derived on the device in double
 * (hence lr and the betas as doubles: the value the host formula of dd_adam_step's callers would give). */
int dd_adam_step_scaled(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1, double beta2,
                        float eps, float grad_scale, const dd_scaler_state* st, dd_stream stream);
/* after dd_adam_step_scaled, one thread.  Flag set: scale = max(scale * backoff, min_scale), good_steps = 0, ++skipped_total.  Flag clear:
 * ++adam_t, ++good_steps, and when good_steps == growth_interval: scale = min(scale * growth, max_scale), good_steps = 0.  The flag is
 * cleared.  Conventional values: growth 2, backoff 0.5, growth_interval 2000, min_scale 1, max_scale 2^24. */
int dd_scaler_update(dd_scaler_state* st, float growth, float backoff, int growth_interval, float min_scale, float max_scale, dd_stream stream);

/* ---- gradient clipping by global norm with per-variable norms (csrc/dd_grad_norm.hip; replaces tf.clip_by_global_norm).  One segmented,
 * fixed-order reduction over the flat gradient arena and, at the same indices, the value arena: two launches on the caller's stream, no
 * floating-point atomics, so the same bytes give the same bytes on every run and on every rank.
 * The host cuts every variable into chunks (deepdenoiser_amd/grad_clip.py, plan_chunks): at most DD_GRAD_CHUNK elements each, never across
 * two variables, never over the padding words between variables (which are excluded from every sum and may hold anything), sorted by
 * variable and, inside one, by offset; var_first[v] ... var_first[v + 1] are the chunks of variable v (n_vars + 1 entries). */
#define DD_GRAD_CHUNK 4096
#define DD_GRAD_PARTIAL_BYTES 24        /* scratch of the first launch per chunk */
typedef struct {
  long offset;            /* first element of the chunk in both arenas */
  int length;             /* 1 ... DD_GRAD_CHUNK elements */
  int variable;           /* index of the variable the chunk belongs to */
} dd_grad_chunk;
typedef struct {
  double grad_sq;         /* sum of squares of the variable's finite STORED gradient elements (before grad_factor) */
  double weight_sq;       /* sum of squares of the variable's values */
  unsigned nonfinite;     /* gradient elements that are inf / NaN; they add to no sum */
  unsigned reserved;      /* 0 */
} dd_grad_var_norms;
typedef struct {
  float grad_norm;                /* |grad_factor| * sqrt(sum of grad_sq): the norm of the true gradient; +inf when any element is inf / NaN */
  float coef;                     /* clip_norm / max(grad_norm, clip_norm); exactly 1 when clip_norm <= 0 or any element is inf / NaN */
  float grad_factor;              /* what the Adam launch multiplies the stored gradients by: grad_scale, or grad_scale / st->scale */
  unsigned nonfinite_variables;   /* variables with at least one inf / NaN gradient element */
  unsigned nonfinite_total;       /* inf / NaN gradient elements of the arena */
} dd_grad_clip;
/* Stage 1 (one workgroup per chunk: sums of squares in double and the count of inf / NaN gradient elements, reduced in a fixed order into
 * `partials`, n_chunks * DD_GRAD_PARTIAL_BYTES bytes) and stage 2 (one workgroup: every variable from its chunks in chunk order into
 * var_norms[n_vars], the totals in variable order into *clip).  grad_factor is grad_scale when st is null and grad_scale / st->scale (read
 * on the device, before the scaler's update) otherwise -- the factor of the Adam launch that follows.  clip_norm <= 0 only measures
 * (coef = 1).  chunks, var_first, partials, var_norms and clip are device memory; the whole of var_norms and *clip is rewritten by every
 * call.  grads and values 16-byte aligned.  The entry cannot see the device tables: that every chunk lies inside both arenas, that
 * var_first has n_vars + 1 ascending entries ending in n_chunks and that the output buffers have the sizes above is the caller's
 * responsibility (grad_clip.GradientClipper checks its plan against the arena length before it uploads it). */
int dd_grad_norms(const float* grads, const float* values, const dd_grad_chunk* chunks, int n_chunks, const int* var_first, int n_vars,
                  void* partials, dd_grad_var_norms* var_norms, dd_grad_clip* clip, float clip_norm, float grad_scale,
                  const dd_scaler_state* st, dd_stream stream);
/* The two Adam launches with the gradient grads * grad_factor * clip->coef (clip->coef read on the device).  With clip->coef == 1 the
 * results are bit-identical to those of the unclipped entries; the skip on st->found_nonfinite is unchanged. */
int dd_adam_step_clipped(float* params, const float* grads, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                         float eps, float grad_scale, const dd_grad_clip* clip, dd_stream stream);
int dd_adam_step_scaled_clipped(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1, double beta2,
                                float eps, float grad_scale, const dd_scaler_state* st, const dd_grad_clip* clip, dd_stream stream);

/* ---- inference stitch (Prediction.py:384-441): copy crop windows of row-major tiles into the frame */
typedef struct { int tile; int crop_y0, crop_y1, crop_x0, crop_x1; int dst_img, dst_y, dst_x; } dd_stitch_entry;
/* frames: [n_img, frame_h, frame_w, ldf]; entry copies tiles[tile][crop] to frames[dst_img] at (dst_y, dst_x) */
int dd_stitch(const float* tiles, int tile_size, int ldt, float* frames, int frame_h, int frame_w, int ldf, int C,
              const dd_stitch_entry* table, int n_entries, dd_stream stream);

/* ---- feathered stitch: the overlapping tile predictions blended instead of cropped.  A DEPARTURE from Prediction.py:384-441, which keeps one
 * tile's prediction per output pixel and drops the others: neighbouring tiles see different context and disagree inside their overlap, and
 * the crop turns that disagreement into a step along every tile border.  Here
 *   frames[f][y][x][c] = sum over the tiles (i, j) that cover (y, x), ascending row-major index i * cols->count + j, of
 *                        rows->weights[i][y - oy_i] * cols->weights[j][x - ox_j] * tiles[f * tiles_per_image + (i * cols->count + j - first_tile)][y - oy_i][x - ox_j][c]
 * with normalised per-axis weights (deepdenoiser_amd/tiling.py blend_weights: they add up to 1 over the covering tiles of a coordinate), each
 * term as fmaf(w_y * w_x, value, sum) in fp32.  One call adds the tiles [first_tile, first_tile + n_tiles) of a row-major plan; the tiles of a
 * frame are given in ascending order over one or more calls on one stream.  A float starts from its stored value when a tile below first_tile
 * covers it and from 0 otherwise, is written once per call by the one thread that owns it, and is not touched when none of the call's tiles
 * covers it: frames need no memset, there are no atomics, and the result is bit-identical for every split of the tiles into calls.
 * An axis (a HOST struct; `origins` a host array, the other tables device memory): count tiles of tile_size, ascending origins inside the
 * frame; weights [count][tile_size]; first / last [extent]: the lowest and highest tile index that covers each image coordinate.
 * tiles [n_img * tiles_per_image, tile_size, tile_size, ldt], frames [n_img, frame_h, frame_w, ldf], 1 <= C <= 4, ldt >= C, ldf >= C. */
typedef struct { int count; const int* origins; const int* origins_dev; const float* weights; const int* first; const int* last; } dd_blend_axis;
int dd_stitch_blend(const float* tiles, int tile_size, int ldt, int tiles_per_image, float* frames, int n_img, int frame_h, int frame_w, int ldf,
                    int C, const dd_blend_axis* rows, const dd_blend_axis* cols, int first_tile, int n_tiles, dd_stream stream);

/* ---- inference tile extraction (Prediction.py:283-310: tiled_feature = feature[lower_h:upper_h, lower_w:upper_w] for every window
 * of the plan): tiles[i] = frame[origin_y[i] : +tile_size, origin_x[i] : +tile_size, 0:C].  frame [frame_h, frame_w, ldf],
 * tiles [n_tiles, tile_size, tile_size, ldt] fp32; origins: n_tiles (y, x) int pairs on the device. */
int dd_extract_tiles(const float* frame, int frame_h, int frame_w, int ldf, int C, float* tiles, int tile_size, int ldt,
                     const int* origins_yx, int n_tiles, dd_stream stream);

/* ---- recombination (Prediction.py:443-481): image = sum_k color_k*(direct_k+indirect_k) + sum_j single_j ; also writes each
 * combined_k if combined[k] != NULL.  All tensors [npix, 3] fp32 contiguous. */
typedef struct {
  int n_triples; const float* color[4]; const float* direct[4]; const float* indirect[4]; float* combined[4];
  int n_singles; const float* single[8];
  float* image;
} dd_recombine_desc;
int dd_recombine(const dd_recombine_desc* desc, long npix, dd_stream stream);

/* ---- NaN / Inf samples of render passes in device memory (csrc/dd_nonfinite.hip).  A table of up to DD_NONFINITE_MAX_PLANES planes that share
 * N, H, W (a frame: N = 1; a batch of tiles: N > 1), all served by ONE launch.  A plane: fp32 data [N,H,W,ld] of which the first C (1 or 3)
 * channels are looked at, ld >= C, and its uint8 mask [N,H,W].  "Non-finite" is a test on the bits -- all eight exponent bits set: +-inf,
 * quiet and signalling NaNs of either sign; +-FLT_MAX, denormals and -0 are finite.  desc is a HOST struct (copied by value).  A bad argument
 * (a NULL table or counts, n_planes outside 1 .. 32, C outside {1, 3}, ld < C, a NULL plane pointer, N H W beyond the 32-bit pixel index,
 * radius outside 1 .. 4) returns a negative status without a launch.  No host sync. */
#define DD_NONFINITE_MAX_PLANES 32
typedef struct { float* data; int C; int ld; unsigned char* mask; } dd_nonfinite_plane;
typedef struct { int n_planes; dd_nonfinite_plane plane[DD_NONFINITE_MAX_PLANES]; } dd_nonfinite_desc;
/* What NaNHighlighter.py:40-42 computes per file on the host (255 * !isfinite per channel), for every plane of the table: mask byte of every
 * pixel = bit c set when channel c is non-finite (zero bytes are written too: the mask needs no memset), and
 * counts[2 * plane] += non-finite values, counts[2 * plane + 1] += pixels with at least one (DEVICE uint64 pairs, zeroed by the caller;
 * integer atomics: exact, the same from run to run).  Every value is read once; a dense plane (ld == C, data 16-byte and mask 4-byte
 * aligned) with 16-byte loads. */
int dd_nonfinite_scan(const dd_nonfinite_desc* desc, int N, int H, int W, uint64_t* counts, dd_stream stream);
/* Where OpenEXRDirectory.py:72-76 gives the frame up (it marks a directory with a non-finite value invalid), repair it IN PLACE after a
 * dd_nonfinite_scan of the same table: every value whose mask bit is set becomes the mean of the values of the same channel and image in
 * the (2 radius + 1)^2 window around it whose mask bit is clear -- the window clipped to the image, the values added in row-major window
 * order in fp32 and divided once by their count; 0.0f when the window holds none.  Usable neighbours are decided from the mask planes alone;
 * only masked positions are written and only unmasked ones read, so the result does not depend on scheduling.  Values that are not masked
 * are never written.  The workgroups of a plane with counts[2 * plane + 1] == 0 return at once. */
int dd_nonfinite_repair(const dd_nonfinite_desc* desc, int N, int H, int W, int radius, const uint64_t* counts, dd_stream stream);

/* ---- full-frame quality of a denoised frame against its target, where the frames are (csrc/dd_quality.hip).  Up to DD_QUALITY_MAX_PAIRS
 * (prediction, target) pairs of one frame size in ONE call: one scoring launch over all pairs and one launch that adds the workgroups'
 * partial records up.  A pair: two fp32 images [H,W,ld] of which the first nch (1 or 3) channels are used, ld >= nch (a 1-channel
 * prediction is a [..., :1] view of a 3-wide frame: ld 3, nch 1).  pairs is a HOST array (copied by value).
 *   valid pixel  : all nch channels of BOTH images finite (the bit test of dd_nonfinite_scan); an invalid pixel adds to nothing but is
 *                  missing from pixels_valid.  valid window: all 121 pixels of an 11 x 11 window valid.
 * A RECORD (DEVICE, 72 bytes, 8-byte aligned, overwritten):
 *   uint64 pixels_valid, windows_valid     exact
 *   uint64 ldr_sq_err                      sum over valid pixels and channels of (b_p - b_t)^2, the byte b of a channel = the number of entries
 *                                          of `thresholds` <= exposure * value (one fp32 multiply; the rule and the table of dd_loss_previews,
 *                                          metrics.preview_thresholds: the sRGB display value).  Exact.  PSNR_8bit = 10 log10(255^2 n / this)
 *   double se, ae, rse, smape              scene-referred sums over valid pixels and channels of the fp32 terms (one rounding per operation)
 *                                          (p-t)^2 | |p-t| | (p-t)^2 / (t^2 + epsilon) | |p-t| / (|p| + |t| + epsilon): the SQUARED, ABSOLUTE
 *                                          and SMAPE forms of LossDifference.py:18-34 (epsilon: its 1e-2) and the relative MSE; `exposure`
 *                                          never touches them
 *   double ssim_sum                        sum over valid windows of the window's SSIM: on byte / 255, per channel the 11 x 11 Gaussian of
 *                                          sigma 1.5 (normalised, VALID positions), C1 = 0.01^2, C2 = 0.03^2 (tf.image.ssim as the ms_ssim term
 *                                          calls it, max_val 1: csrc/dd_loss_msssim.hip level 0),
 *                                          (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)), then the mean over the channels
 *   float max_abs; float reserved (0)      max over valid pixels and channels of the fp32 |p-t|
 * ssim_maps: HOST array of n_pairs DEVICE pointers, or NULL; a non-NULL entry receives the pair's [(H-10),(W-10)] fp32 map, an invalid window
 * as NaN: every element written exactly once and nothing else.  With H < 11 or W < 11 there are no windows: windows_valid = 0, ssim_sum = 0,
 * the map pointer is ignored.  Window moments are accumulated in double from the integer bytes, every sum across a workgroup's pixels and
 * across workgroups in double in a fixed order (no floating-point atomics): two runs give the same bits, and a pair's record depends neither
 * on its index nor on the other pairs of the call.  A workgroup owns DD_QUALITY_TILE^2 pixels and the windows that start there.  scratch:
 * >= dd_frame_quality_scratch_bytes (negative for a bad shape), 8-byte aligned.  A bad argument (n_pairs outside 1 .. 32, nch outside {1, 3},
 * ld < nch, H or W < 1, a NULL pred / target / thresholds / records / scratch) returns a negative status without a launch.  No host sync. */
#define DD_QUALITY_MAX_PAIRS 32
#define DD_QUALITY_TILE 32
typedef struct { const float* pred; const float* target; int pred_ld, target_ld, nch; } dd_quality_pair;
typedef struct {
  uint64_t pixels_valid, windows_valid, ldr_sq_err;
  double se, ae, rse, smape, ssim_sum;
  float max_abs, reserved;
} dd_quality_record;
long dd_frame_quality_scratch_bytes(int n_pairs, int H, int W);
int dd_frame_quality(const dd_quality_pair* pairs, int n_pairs, int H, int W, const float* thresholds, float exposure, float epsilon,
                     float* const* ssim_maps, void* records, void* scratch, dd_stream stream);

/* ---- temporal stabilisation of a denoised frame sequence (csrc/dd_temporal.hip).  The reference has no such step (Prediction.py denoises
 * every frame on its own); it stands behind predict's --temporal.  Up to DD_TEMPORAL_MAX_PASSES passes of one frame size in ONE call: one
 * stabilising launch over all passes and one launch that adds the workgroups' partial records up.  A pass: `current` (the frame just denoised),
 * `history` (the stabilised previous frame) and `out`, fp32 images [H,W,ld] of which the first nch (1 or 3) channels are used, ld >= nch each
 * (a 1-channel prediction is a [..., :1] view of a 3-wide frame: ld 3, nch 1).  motion: fp32 [H,W,motion_ld], channels 0 and 1 used.  A
 * guide: `current` and `previous` of the same form and a tolerance.  passes and guides are HOST arrays (copied by value).
 * Per pixel (x = column, y = row), decided ONCE and shared by all passes, in fp32 with one rounding per operation:
 *   px = x + sx * motion[y,x,0], py = y + sy * motion[y,x,1]: where the pixel was in the previous frame
 *   offscreen    : px or py not finite or outside [0, W-1] x [0, H-1]
 *   taps         : x0 = floor(px), fx = px - x0, y0 = floor(py), fy = py - y0; (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), indices clamped
 *   guide        : for ANY guide, |current[y,x,c] - previous[floor(py + 0.5), floor(px + 0.5), c]| (indices clamped) is not <= tolerance for
 *                  some channel c (a non-finite difference rejects).  offscreen takes precedence over guide.
 * Per pass and pixel:
 *   h            : (t00 (1-fx) + t01 fx)(1-fy) + (t10 (1-fx) + t11 fx) fy of `history`
 *   per channel  : the 3 x 3 window of `current` around the pixel (coordinates clamped at the border), its mean m (the nine values added in
 *                  row-major order, times 1/9) and population standard deviation s = sqrt(E[v^2] - m^2), taken as sqrt(mean((v - m)^2));
 *                  lo = m - gamma s, hi = m + gamma s, hc = min(max(h, lo), hi)
 *   nonfinite    : any used channel of h or of the nine window values is not finite
 *   out          : `current` bit for bit (NaN payloads included) where the pixel is offscreen, guide-rejected or nonfinite; every other pixel
 *                  is BLENDED: current + alpha * (hc - current).  Every used channel of every pixel of out is written exactly once; channels
 *                  nch .. ld-1 are not touched.
 * A RECORD per pass (DEVICE, 64 bytes, 8-byte aligned, overwritten):
 *   uint64 pixels_offscreen, pixels_guide, pixels_nonfinite, pixels_blended     exact; they add up to H * W
 *   uint64 values_clamped                  channels of blended pixels with h < lo or h > hi
 *   double change, flicker_before, flicker_after     sums over blended pixels and channels of the fp32 terms |out - current| | |current - h| |
 *                                          |out - h|, added in double in a fixed order across a workgroup and across workgroups (no
 *                                          floating-point atomics)
 * Two runs give the same bits, and a pass's record and output depend neither on its index nor on the other passes of the call.  A workgroup
 * owns DD_TEMPORAL_TILE^2 pixels.  scratch: >= dd_temporal_scratch_bytes (negative for a bad shape), 8-byte aligned; a shorter one cannot be
 * detected.  Refused with a negative status before any launch: n_passes outside 1 .. 32, n_guides outside 0 .. 4, nch outside {1, 3}, an
 * ld < nch, motion_ld < 2, H or W < 1, alpha outside [0, 1], gamma < 0, a negative tolerance or a non-finite parameter, a NULL pointer, and
 * an `out` that is `current` or `history` of any pass of the call (neighbours read both, so in place is not possible).  No host sync. */
#define DD_TEMPORAL_MAX_PASSES 32
#define DD_TEMPORAL_MAX_GUIDES 4
#define DD_TEMPORAL_TILE 16
typedef struct { const float* current; const float* history; float* out; int current_ld, history_ld, out_ld, nch; } dd_temporal_pass;
typedef struct { const float* current; const float* previous; int current_ld, previous_ld, nch; float tolerance; } dd_temporal_guide;
typedef struct {
  uint64_t pixels_offscreen, pixels_guide, pixels_nonfinite, pixels_blended, values_clamped;
  double change, flicker_before, flicker_after;
} dd_temporal_record;
long dd_temporal_scratch_bytes(int n_passes, int H, int W);
int dd_temporal_stabilize(const dd_temporal_pass* passes, int n_passes, const dd_temporal_guide* guides, int n_guides, int H, int W,
                          const float* motion, int motion_ld, float sx, float sy, float alpha, float gamma, void* records, void* scratch,
                          dd_stream stream);

/* ---- temporal error of a denoised frame sequence against its target frames, where the frames are (csrc/dd_sequence_quality.hip).  The
 * reference has no such measure; it stands behind predict's --target_sequence.  Up to DD_SEQQ_MAX_PAIRS pairs of one frame size in ONE call:
 * one scoring launch over all pairs and one launch that adds the workgroups' partial records up.  A pair: `pred` and `target` (the denoised
 * frame and its ground truth), `pred_previous` and `target_previous` (the same of the frame before), fp32 images [H,W,ld] of which the first
 * nch (1 or 3) channels are used, every image with an ld >= nch of its own (a 1-channel pass is a [..., :1] view of a 3-wide frame: ld 3,
 * nch 1).  motion: fp32 [H,W,motion_ld] of the CURRENT frame, channels 0 and 1 used.  pairs is a HOST array (copied by value).
 * Per pixel (x = column, y = row), decided ONCE and shared by all pairs, in fp32 with one rounding per operation (dd_motion_previous of
 * csrc/dd_frame_common.h, the function dd_temporal_stabilize compiles too: its rules without its guides):
 *   px = x + sx * motion[y,x,0], py = y + sy * motion[y,x,1]: where the pixel was in the previous frame
 *   offscreen    : px or py not finite or outside [0, W-1] x [0, H-1]
 *   taps         : x0 = floor(px), fx = px - x0, y0 = floor(py), fy = py - y0; (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), indices clamped
 * Per pair and pixel that is not offscreen:
 *   nonfinite    : any of the nch channels of pred[y,x], of target[y,x] or of one of the four taps of pred_previous or target_previous is
 *                  not finite (the bit test of dd_nonfinite_scan; a tap with weight 0 still counts).  offscreen takes precedence.
 *   valid        : every other pixel.  Per channel, in fp32 with one rounding per operation:
 *                  hp = (a00 (1-fx) + a01 fx)(1-fy) + (a10 (1-fx) + a11 fx) fy over the taps of pred_previous, ht the same over the taps of
 *                  target_previous; dp = p - hp, dt = t - ht, e = dp - dt: the change of the error image E = P - T along the motion,
 *                  E_t(x) - warp(E_t-1)(x), zero for a static bias and large for error that changes from frame to frame.
 *                  Display-referred: the byte b(v) = the number of entries of `thresholds` <= exposure * v (one fp32 multiply; the rule and
 *                  the table of dd_frame_quality); Hp, Ht: the same bilinear form over the bytes of the taps as floats;
 *                  DP = b(p) - Hp, DT = b(t) - Ht, in byte units.
 * A RECORD per pair (DEVICE, 72 bytes, 8-byte aligned, overwritten):
 *   uint64 pixels_offscreen, pixels_nonfinite, pixels_valid      exact; they add up to H * W
 *   double change_prediction, change_target, temporal_error      sums over valid pixels and channels of |dp| | |dt| | |e|
 *   double ldr_change_prediction, ldr_change_target, ldr_temporal_error      the same sums of |DP| | |DT| | |DP - DT|
 * The fp32 terms are added in double in a fixed order across a workgroup and across workgroups (no floating-point atomics): two runs give
 * the same bits, and a pair's record depends neither on its index nor on the other pairs of the call.  A workgroup owns DD_SEQQ_TILE^2
 * pixels.  No image is written.  scratch: >= dd_sequence_quality_scratch_bytes (negative for a bad shape), 8-byte aligned; a shorter one
 * cannot be detected.  Refused with a negative status before any launch: n_pairs outside 1 .. 32, nch outside {1, 3}, an ld < nch,
 * motion_ld < 2, H or W < 1, a non-finite sx, sy or exposure, a NULL or not 4-byte aligned image pointer, NULL motion, thresholds, records
 * or scratch.  No host sync. */
#define DD_SEQQ_MAX_PAIRS 32
#define DD_SEQQ_TILE 16
typedef struct {
  const float* pred; const float* pred_previous; const float* target; const float* target_previous;
  int pred_ld, pred_previous_ld, target_ld, target_previous_ld, nch;
} dd_seqq_pair;
typedef struct {
  uint64_t pixels_offscreen, pixels_nonfinite, pixels_valid;
  double change_prediction, change_target, temporal_error, ldr_change_prediction, ldr_change_target, ldr_temporal_error;
} dd_seqq_record;
long dd_sequence_quality_scratch_bytes(int n_pairs, int H, int W);
int dd_sequence_quality(const dd_seqq_pair* pairs, int n_pairs, int H, int W, const float* motion, int motion_ld, float sx, float sy,
                        const float* thresholds, float exposure, void* records, void* scratch, dd_stream stream);

/* ---- small helpers of the graph executor */
/* dst (+)= src * (mask > 0)   (identity/residual gradient paths into ReLU outputs); mask may be NULL; dst == src is allowed.
 * dd_masked_add, dd_zero_stuff, dd_zero_unstuff and dd_space_to_depth2 move 4 elements at a time: C (cp) and every ld multiples of 4, every
 * pointer aligned to 4 elements (8 bytes bf16 / fp16, 16 bytes f32); a bad dtype code or alignment returns -1 before a launch. */
int dd_masked_add(void* dst, int lddst, const void* src, int ldsrc, const void* mask, int ldmask, int C, long npix,
                  int accumulate, int dtype, dd_stream stream);
/* dst[pix][0:nch] = convert(src[pix][0:nch]); dst[pix][nch:dst_pad] = 0   (dtype codes per tensor; fp32 <-> graph dtype) */
int dd_convert_channels(const void* src, int src_dtype, int ldsrc, void* dst, int dst_dtype, int lddst, int nch, int dst_pad,
                        long npix, dd_stream stream);
/* ---- data augmentation of one render pass of a batch of tiles (DataAugmentation.py:10-200 as applied by Training.py:794-821,
 * FeatureTrainingAugmentation Training.py:551-604): dst[b] = rotate_normal(permute_rgb(rotate_90(flip_left_right(src[b])))) with
 * per-tile draws.  src/dst: [B,H,W,C] float32, C = 1 or 3.  draws: B device records.  kind: DD_AUG_PLAIN (geometry only), DD_AUG_RGB
 * (RenderPasses.is_rgb_color_render_pass: the channel permutation applies), DD_AUG_NORMAL (world-space normal: the 3x3 rotation applies;
 * v_out = v_in * M, row vector times matrix), DD_AUG_SCREEN_NORMAL (flip negates x; rot90 k maps (x,y) -> (-y,x), (-x,-y), (y,-x)).
 * use_* : the DataAugmentationUsage switches.  Rotation by an odd k needs H == W (tiles are square). */
typedef struct { int flip; int rotate; int permute; float normal_rotation[9]; } dd_augment_draw;
enum { DD_AUG_PLAIN = 0, DD_AUG_RGB = 1, DD_AUG_NORMAL = 2, DD_AUG_SCREEN_NORMAL = 3 };
int dd_augment(const float* src, float* dst, int C, int B, int H, int W, const dd_augment_draw* draws, int kind,
               int use_flip, int use_rotate, int use_permute, int use_normal_rotation, dd_stream stream);

/* ---- training tiles cut from frames that stay in device memory (csrc/dd_tile_sampler.hip).  Replaces the tile set the reference writes
 * to disk (TFRecordsCreator.py:125-133: the fixed grid of non-overlapping tiles; :221-231: one record per tile), its decode
 * (Training.py:507-524) and the per-pass augmentation launches (Training.py:794-821): ONE launch fills every input and target tile buffer of
 * a mini-batch,
 *     dst[b, y, x, 0:C] = augment(plane[y0 : y0 + T, x0 : x0 + T, :])[y, x, :]
 * with `augment` exactly dd_augment's for the pass's kind, the record's draw and the four use_* switches.  Channels C .. ld_dst-1 of dst are
 * not written.
 *   plane   : one rendering of one scene.  Every pass has a DEVICE array of n_planes base pointers (fp32 [h, w, C], contiguous; NULL where the
 *             pass is not loaded for that rendering: such a block writes nothing); plane_hw is the DEVICE table [n_planes][2] of (h, w),
 *             shared by all passes (scenes differ in size).
 *   record  : DEVICE, one per example: the plane the source passes read, the plane the target passes read, the window's origin, the draw.
 *             Records cannot be checked on the host; the kernel clamps the plane index into 0 .. n_planes-1 and the origin into
 *             [0, h-T] x [0, w-T] (a plane smaller than a tile is skipped), so a bad record reads no byte outside a plane.
 *   pass    : C in {1, 3}; kind DD_AUG_*; dst fp32 [B, T, T, ld_dst], ld_dst >= C; from_target: reads the record's target plane.
 * desc is a HOST struct (copied by value).  Refused with a negative status and no launch: NULL pointers, n_passes outside
 * 1 .. DD_TILE_MAX_PASSES, C outside {1, 3}, a kind other than DD_AUG_PLAIN with C != 3, ld_dst < C, use_flip with a DD_AUG_NORMAL pass (as
 * dd_augment), T < 1, B < 1.  No host sync. */
#define DD_TILE_MAX_PASSES 64
typedef struct { int source_plane; int target_plane; int y0; int x0; dd_augment_draw draw; } dd_tile_record;
typedef struct { const float* const* planes; float* dst; int C; int kind; int ld_dst; int from_target; } dd_tile_pass;
typedef struct { int n_passes; int n_planes; const int* plane_hw; dd_tile_pass pass[DD_TILE_MAX_PASSES]; } dd_tile_sampler_desc;
int dd_sample_tiles(const dd_tile_sampler_desc* desc, const dd_tile_record* records, int B, int T, int use_flip, int use_rotate,
                    int use_permute, int use_normal_rotation, dd_stream stream);

/* ---- data-set statistics of frames that stay in device memory (csrc/dd_frame_statistics.hip).  Replaces the two sweeps over a tile set on
 * disk by which the reference makes <mode>_statistics.json (TFRecordsStatistics.py:109-140 and :162-193, per tile
 * _first_statistics_iteration :236-285 and _second_statistics_iteration :287-316; the tiles are the grid of TFRecordsCreator.py:125-133):
 * ONE launch reads every sample of every (window, pass) once and writes a row of DD_STAT_FIELDS doubles per (window, pass),
 *     out[(window * n_passes + pass) * DD_STAT_FIELDS + field]
 * from which the host joins the file (deepdenoiser_amd/statistics.py).  With x the T x T x C window of the pass, l = sign(x) log1p(|x|)
 * (Utilities.signed_log1p), the pivot K = the window's first sample x[0, 0, 0] and Kl = signed_log1p(K), the fields are
 *     DD_STAT_PRESENT                1.0, or 0.0: the plane does not hold the pass (a NULL plane pointer) or is smaller than a window;
 *                                    every other field of such a row is 0
 *     DD_STAT_MIN, _MAX              min x, max x                      DD_STAT_MIN_LOG1P, _MAX_LOG1P     min l, max l
 *                                    (min l and max l are signed_log1p of min x and max x -- the function is monotone -- rounded to the
 *                                    nearest double; the log1p inside the sums is the math library's, within an ulp)
 *     DD_STAT_PIVOT, _PIVOT_LOG1P    K, Kl
 *     DD_STAT_SUM, _SUM_SQ           sum (x - K), sum (x - K)^2        DD_STAT_SUM_LOG1P, _SUM_SQ_LOG1P  sum (l - Kl), sum (l - Kl)^2
 *                                    over all T * T * C samples
 *     DD_STAT_COUNT                  the number of pixels with sum_c |x_c| != 0 (Conv2dUtilities.non_zero_mask; is_alpha: x - 1 in place
 *                                    of x, TFRecordsStatistics.py:262-264 and :277-280)
 *     DD_STAT_MASK_SUM               sum over pixels of m = sign(sum_c |mask_c|), the mask pass read at the same window of mask_plane (:246-249)
 *     DD_STAT_MASKED_SUM, ...        the four shifted sums with every term times m(pixel), over all three channels (:252, :258, :270, :309, :312)
 * The sums are shifted because the global mean the variance is taken about (:289-290) is known only after every window has been seen: with
 * d = mean - K,  sum (x - mean)^2 = sum (x - K)^2 - 2 d sum (x - K) + n d^2, and a plane is read once (a raw sum of squares would lose
 * everything next to Blender's Depth of 1e10 where no surface is hit).  Without a mask (mask_planes NULL, a NULL mask plane pointer, or a mask
 * plane smaller than a window) DD_STAT_MASK_SUM and the masked sums are 0.
 *   plane, plane_hw : as dd_sample_tiles: per pass a DEVICE array of n_planes base pointers (fp32 [h, w, C], contiguous, NULL where the pass
 *             is not loaded), and the DEVICE table [n_planes][2] of (h, w).  mask_planes: the same array of the target COLOUR pass
 *             (3 channels) the pass is masked by, or NULL.
 *   window  : DEVICE table.  Windows cannot be checked on the host; the kernel clamps plane and mask_plane into 0 .. n_planes-1 and the
 *             origin into [0, h-T] x [0, w-T] of the plane it reads (the mask plane's own size for the mask), so a bad window reads no byte
 *             outside a plane.
 * log1p and every sum are double.  The order of a sum is fixed (a thread's pixels in ascending order, a shift-down tree over the wave, the
 * waves in order through LDS) and there are no atomics: two launches on the same input give the same bytes.
 * desc is a HOST struct (copied by value).  Refused with a negative status and no launch: NULL pointers, n_passes outside
 * 1 .. DD_STAT_MAX_PASSES, C outside {1, 3}, a mask pass on a pass with C != 3 (the reference stacks the mask three times, :252), T < 1 (or
 * above 16384), n_windows < 1.  No host sync. */
#define DD_STAT_MAX_PASSES 64
enum { DD_STAT_PRESENT = 0, DD_STAT_MIN, DD_STAT_MAX, DD_STAT_MIN_LOG1P, DD_STAT_MAX_LOG1P, DD_STAT_PIVOT, DD_STAT_PIVOT_LOG1P,
       DD_STAT_SUM, DD_STAT_SUM_SQ, DD_STAT_SUM_LOG1P, DD_STAT_SUM_SQ_LOG1P, DD_STAT_COUNT, DD_STAT_MASK_SUM,
       DD_STAT_MASKED_SUM, DD_STAT_MASKED_SUM_SQ, DD_STAT_MASKED_SUM_LOG1P, DD_STAT_MASKED_SUM_SQ_LOG1P, DD_STAT_FIELDS };
typedef struct { int plane; int mask_plane; int y0; int x0; } dd_stat_window;
typedef struct { const float* const* planes; const float* const* mask_planes; int C; int is_alpha; } dd_stat_pass;
typedef struct { int n_passes; int n_planes; const int* plane_hw; dd_stat_pass pass[DD_STAT_MAX_PASSES]; } dd_stat_desc;
int dd_tile_statistics(const dd_stat_desc* desc, const dd_stat_window* windows, int n_windows, int T, double* out, dd_stream stream);

/* ---- importance scores of frames that stay in device memory (csrc/dd_frame_importance.hip): how much the noisy source renderings differ
 * from the target rendering, per G x G cell, in the measure of the loss itself -- the SMAPE of LossDifference.py:30-34 with its default
 * epsilon.  The reference fixes its training tiles on disk once and for all (TFRecordsCreator.py:125-133: the grid of non-overlapping tiles);
 * with resident frames a training window can be drawn where the noise is (deepdenoiser_amd/frame_importance.py makes the density from these
 * cells, `train.py --frames_crops importance`).  ONE launch reads every sample of the colour passes once and writes one double per cell:
 * with t the cell's target plane and s_k the source planes source_plane0 + k, k < n_sources, over the G x G x 3 samples of every pass p,
 *     out[n] = sum_p sum_k sum_pixels sum_c  |s_k - t| / ((|s_k| + |t|) + epsilon)
 * A term is evaluated in fp32 in exactly that order with a division rounded to nearest (there is no product: nothing contracts into an FMA);
 * the terms -- none negative, so nothing cancels -- are added in double.  A (pass, source) pair whose source or target plane pointer is NULL
 * adds nothing; a cell one of whose planes is smaller than G x G gets out[n] = 0.
 *   plane, plane_hw : as dd_sample_tiles: per pass a DEVICE array of n_planes base pointers (fp32 [h, w, 3], contiguous, NULL where the pass is
 *             not loaded), and the DEVICE table [n_planes][2] of (h, w).  Every pass is a 3-channel colour pass.
 *   cell    : DEVICE table.  Cells cannot be checked on the host; the kernel clamps target_plane into 0 .. n_planes-1, source_plane0 so that
 *             source_plane0 + n_sources - 1 stays in that range, and the origin into [0, h-G] x [0, w-G] of the plane it reads, as
 *             dd_tile_statistics does, so a bad cell reads no byte outside a plane.
 * The order of a sum is fixed (one wave per cell; a lane's pixels in ascending row-major order, per pixel the passes in order, per pass the
 * sources in order, channels 0 .. 2; the shift-down tree of dd_tile_statistics over the wave) and there are no atomics: two launches on the
 * same input give the same bytes, so data-parallel ranks arrive at the same table.
 * desc is a HOST struct (copied by value).  Refused with a negative status and no launch: NULL pointers, n_passes outside
 * 1 .. DD_IMPORTANCE_MAX_PASSES, n_planes < 1, n_sources < 1, G outside 1 .. 64, n_cells < 1, an epsilon that is not positive and finite.
 * No host sync. */
#define DD_IMPORTANCE_MAX_PASSES 16
typedef struct { int source_plane0; int target_plane; int y0; int x0; } dd_importance_cell;
typedef struct { const float* const* planes; } dd_importance_pass;
typedef struct { int n_passes; int n_planes; const int* plane_hw; int n_sources; float epsilon; dd_importance_pass pass[DD_IMPORTANCE_MAX_PASSES]; } dd_importance_desc;
int dd_importance_cells(const dd_importance_desc* desc, const dd_importance_cell* cells, int n_cells, int G, double* out, dd_stream stream);

/* ---- importance scores refreshed from the running model's error (csrc/dd_importance_update.hip).  dd_importance_cells measures noise only
 * and its scores never change while the network trains; this launch scores the mini-batch that was just forwarded in the SAME measure -- the
 * mean SMAPE(prediction, target) of a cell, so a network that returns its input scores exactly the noise map -- and the host moves the
 * visited cells of the density towards it (deepdenoiser_amd/frame_importance.py: ImportanceScorer, ImportanceMap.fold;
 * `train.py --frames_importance_refresh`).  It runs inside the step, between the forward and the first backward launch (the backward may
 * reuse prediction buffers).
 *   records : DEVICE, the table dd_sample_tiles has just cut the mini-batch from; use_flip / use_rotate: the switches it was given.
 *   pass    : a 3-channel colour pass: pred fp32 [B, T, T, pred_ld], target fp32 [B, T, T, target_ld], both leading dimensions >= 3.
 *   cell    : the G x G cells of a scene, h / G by w / G, row-major, scenes in order (the order of dd_importance_cells' table as
 *             frame_importance.cell_table writes it).  cell_base is a DEVICE int[n_planes]: for a target plane the index of its scene's first
 *             cell in the flat accumulators, -1 for every other plane.  plane_hw: as dd_sample_tiles.
 * With (y0, x0) an example's origin in its target plane, the cells (cy, cx) that lie WHOLLY inside [y0, y0 + T) x [x0, x0 + T) are scored
 * (per axis T / G of them when the origin is a multiple of G, T / G - 1 otherwise); a cell the window covers in part gets nothing.  The pixel
 * (fy, fx) of the un-augmented window is read at the one tile pixel that shows it: the inverse of dd_sample_tiles' geometry for the record's
 * rotate & 3 and flip under the two switches (the RGB permutation and the normal rotation do not matter: prediction and target carry the same
 * permutation and a term is summed over the channels).  One wave per (example, cell slot); a lane owns the cell's pixels l, l + 64, ... in
 * the FRAME's row-major order, per pixel the passes in order, channels 0 .. 2; a term is |p - t| / ((|p| + |t|) + epsilon) in fp32 in exactly
 * that order with a division rounded to nearest, the terms are added in double and the lanes combined by dd_importance_cells' shift-down tree
 * -- with the prediction replaced by the sampled source tile the sum is the one dd_importance_cells forms.  Then
 *     mean = sum / (G G 3 n_passes);   finite:  acc_sum[cell] += llrint(mean 2^32),  acc_count[cell] += 1     (integer atomics)
 * and a mean that is not finite (an fp16 overflow or a NaN in a prediction) adds nothing.  Integer sums do not depend on the order of the
 * adds: two runs over the same predictions leave the same bytes, and data-parallel ranks can add their tables exactly.
 * Records cannot be checked on the host; the kernel clamps the target plane index into 0 .. n_planes-1 and the origin into
 * [0, h-T] x [0, w-T] as dd_sample_tiles does; a plane smaller than a tile, or one with cell_base < 0, adds nothing.
 * desc is a HOST struct (copied by value).  Refused with a negative status and no launch: NULL pointers, n_passes outside
 * 1 .. DD_IMPORTANCE_MAX_PASSES, pred_ld or target_ld below 3, G outside 1 .. 64 or not a divisor of T, T < 1, B < 1 (or above
 * dd_sample_tiles' bounds), n_planes < 1, an epsilon that is not positive and finite.  No host sync. */
typedef struct { const float* pred; const float* target; int pred_ld; int target_ld; } dd_importance_update_pass;
typedef struct { int n_passes; int n_planes; const int* plane_hw; const int* cell_base; float epsilon;
                 dd_importance_update_pass pass[DD_IMPORTANCE_MAX_PASSES]; } dd_importance_update_desc;
int dd_importance_update(const dd_importance_update_desc* desc, const dd_tile_record* records, int B, int T, int G, int use_flip, int use_rotate,
                         unsigned long long* acc_sum, unsigned int* acc_count, dd_stream stream);

/* ---- OpenEXR scan-line chunks rebuilt on the device (csrc/dd_exr_decode.hip).  Replaces the decode the reference leaves to OpenCV
 * (OpenEXRDirectory.py:125-151: cv2.imdecode of the file's bytes, BGR -> RGB, float32) and everything deepdenoiser_amd/openexr.py's host
 * reader does after inflate: the host parses the header and the offset table and inflates (or run-length decodes) each chunk into ONE staged
 * buffer for a whole batch of files; ONE launch then undoes the byte predictor and the even / odd byte split of every coded chunk, splits rows
 * and channels, converts UINT / HALF / FLOAT samples to fp32, writes the [H, W, C] fp32 planes and counts the non-finite samples per file.
 * The planes are bit-identical to openexr.read_image(path)[..., :C].
 *   chunk   : n = rows * row_bytes bytes at `offset` of the staged buffer (16-byte aligned; the chunk owns the bytes up to the next multiple
 *             of 16), row_bytes = sum over the file's channels of W * sample size; rows row0 .. row0 + rows - 1 of file `file`.  coded != 0:
 *             the bytes t are as deflate / the run-length coder saw them -- s[i] = (t[0] + sum_{j=1..i} (t[j] - 128)) & 0xFF in place, then
 *             the original byte p is s[p >> 1] (p even) or s[(n + 1) / 2 + (p >> 1)] (p odd).  coded == 0: the bytes are original
 *             (NO_COMPRESSION, or a chunk stored raw because coding did not shrink it).  Within a row the file's channels follow one another
 *             in header order, W samples each; one workgroup of 256 threads per chunk, a chunk need not fit LDS.
 *   file    : dst fp32 [H, W, C] contiguous; per file channel c < n_channels its pixel type (0 UINT: (float)u rounded to nearest even, 1 HALF:
 *             widened exactly, subnormals included, 2 FLOAT: the bits are moved) and dst_mask[c], the set of destination channels it is
 *             written to (bit d = channel d of dst): 0 for a channel that is skipped (A of an RGBA file), several bits for the single channel
 *             of a file that read_image replicates.  A destination channel no mask names is not written.
 *   counts  : DEVICE uint64[n_files], zeroed by the caller: counts[file] += the destination samples written whose value is NaN or +-Inf
 *             (== np.count_nonzero(~np.isfinite(plane))); one integer atomic add per workgroup.
 * Both tables are given twice: the HOST copy is validated here, the DEVICE copy is what the kernel reads -- and, because it cannot trust
 * device memory, checks again: a chunk whose file index is out of range, whose rows fall outside [0, H) or whose bytes leave the staged
 * buffer is skipped, so nothing is written outside a plane.
 * Refused with a negative status and no launch: NULL tables or buffers while n_chunks > 0, n_chunks < 0, rows outside 1 .. 16, a file with 0
 * or more than DD_EXR_MAX_CHANNELS channels, a pixel type outside 0 .. 2, W < 1 or H < 1, C outside 1 .. 32, a destination channel >= C, a
 * chunk whose file index or rows do not fit its file, an offset that is not 16-byte aligned or leaves staged_bytes.  n_chunks == 0 is a no-op
 * that returns 0.  No host sync. */
#define DD_EXR_MAX_CHANNELS 8
typedef struct { long long offset; int file; int row0; int rows; int coded; } dd_exr_chunk;
typedef struct { float* dst; int H; int W; int C; int n_channels; int type[DD_EXR_MAX_CHANNELS]; unsigned int dst_mask[DD_EXR_MAX_CHANNELS]; } dd_exr_file;
int dd_exr_reconstruct(const dd_exr_chunk* chunks_host, const dd_exr_chunk* chunks, int n_chunks, const dd_exr_file* files_host,
                       const dd_exr_file* files, int n_files, void* staged, long staged_bytes, unsigned long long* counts, dd_stream stream);

/* ---- The zlib streams of ZIP / ZIPS chunks inflated on the device (csrc/dd_exr_inflate.hip, decoder core csrc/dd_inflate_core.h).  Replaces
 * the inflate inside the decode the reference leaves to OpenCV (OpenEXRDirectory.py:125-151: cv2.imdecode of the file's bytes) and the
 * zlib.decompress calls of deepdenoiser_amd/openexr.py's host threads: the host only reads the files; ONE launch inflates every stream of a
 * batch into the staged buffer, where dd_exr_reconstruct (same stream, no sync in between) expects each chunk's post-inflate bytes.
 *   stream  : one zlib stream (RFC 1950 around RFC 1951: stored, fixed and dynamic blocks, any number of them) at src[src_offset ..
 *             + src_bytes) that must expand to exactly dst_bytes bytes, written to staged + dst_offset (16-byte aligned; the stream owns the
 *             bytes up to the next multiple of 16).  One wave per stream.
 *   status  : DEVICE int[n_streams], one DD_INFLATE_* code per stream.  A stream whose status is DD_INFLATE_OK holds exactly the bytes
 *             zlib's inflate gives for it (the Adler-32 is verified); the decoder may be stricter than zlib, never laxer.  A stream with
 *             another status may leave anything inside its own dst_bytes (rounded up to 16) and nothing outside.
 * The table is given twice: the HOST copy is validated here, the DEVICE copy is what the kernel reads -- and checks again
 * (DD_INFLATE_RECORD: the record does not fit the buffers; nothing is read or written through it).
 * Refused with a negative status and no launch: NULL pointers while n_streams > 0, n_streams < 0, src_bytes < 1, dst_bytes outside
 * 1 .. 1 << 30, a source range leaving src_total, a dst_offset that is negative or not 16-byte aligned or whose dst_bytes rounded up to 16
 * leave staged_bytes, a source that overlaps the staged buffer.  n_streams == 0 is a no-op that returns 0.  No host sync. */
#define DD_INFLATE_OK 0
#define DD_INFLATE_HEADER 1      /* method != 8, window bits > 15, (CMF * 256 + FLG) % 31 != 0, or FDICT set */
#define DD_INFLATE_TRUNCATED 2   /* the input ends inside the header, a block, a symbol, extra bits or the Adler-32 */
#define DD_INFLATE_BLOCK_TYPE 3  /* block type 3 */
#define DD_INFLATE_STORED 4      /* LEN != ~NLEN */
#define DD_INFLATE_LENGTHS 5     /* a defective dynamic header */
#define DD_INFLATE_SYMBOL 6      /* literal/length symbol 286 / 287, distance symbol 30 / 31, or a bit pattern that is no code */
#define DD_INFLATE_DISTANCE 7    /* a match reaching before the first output byte */
#define DD_INFLATE_OVERRUN 8     /* output beyond dst_bytes */
#define DD_INFLATE_SHORT 9       /* the final block ended with fewer bytes */
#define DD_INFLATE_CHECK 10      /* Adler-32 mismatch */
#define DD_INFLATE_RECORD 11     /* the device copy of the record does not fit the buffers */
typedef struct { long long src_offset; long long dst_offset; int src_bytes; int dst_bytes; } dd_exr_stream;   /* 24 bytes */
int dd_exr_inflate(const dd_exr_stream* streams_host, const dd_exr_stream* streams, int n_streams, const void* src, long src_total,
                   void* staged, long staged_bytes, int* status, dd_stream stream);

/* ---- OpenEXR scan-line chunks packed on the device (csrc/dd_exr_encode.hip): the inverse of dd_exr_reconstruct.  Prediction.py:483-510 stores
 * every denoised pass as .npy only; the EXR writer of this project replaces openexr.write_exr's host loop (a Python join per scan line, the
 * numpy predictor and byte split): ONE launch turns the fp32 planes of a whole frame's passes into chunk bytes.
 *   chunk   : dd_exr_chunk as above: n = rows * row_bytes bytes written to staged + offset (16-byte aligned; the chunk owns the bytes up to
 *             the next multiple of 16: the padding is written as zero, nothing outside).  The raw bytes are, per row, per file channel in
 *             name order, that channel's W samples little-endian.  coded != 0: the bytes deflate sees -- t = the even raw bytes, then the odd
 *             ones ((n + 1) / 2 even bytes), d[0] = t[0], d[i] = t[i] - t[i-1] + 128 (openexr._interleave_and_predict).  coded == 0: the raw
 *             bytes (NO_COMPRESSION, and chunks stored raw because deflate did not shrink them).
 *   source  : src fp32 [H, W, C] contiguous; file channel k < n_channels is src[y, x, src_channel[k]] stored as type[k]: 1 HALF (round to
 *             nearest even, overflow to +-inf, subnormals; every non-NaN input bit-identical to numpy.astype(float16); a NaN stays a NaN),
 *             2 FLOAT (the bits are moved).  UINT is refused: the planes are fp32.
 * Both tables are given twice: the HOST copy is validated here, the DEVICE copy is what the kernel reads -- and checks again: a chunk that
 * does not fit its source or the staged buffer writes nothing.
 * Refused with a negative status and no launch: NULL tables or buffer while n_chunks > 0, n_chunks < 0, n_sources < 1, a source with a null
 * plane, H < 1 or W < 1, C outside 1 .. 32, 0 or more than DD_EXR_MAX_CHANNELS channels, a pixel type other than 1 or 2, a src_channel
 * outside [0, C), rows outside 1 .. 16, a chunk whose file index or rows do not fit its source, an offset that is not 16-byte aligned or
 * leaves staged_bytes, a staged buffer that is not 16-byte aligned.  n_chunks == 0 is a no-op that returns 0.  No host sync. */
typedef struct { const float* src; int H; int W; int C; int n_channels; int type[DD_EXR_MAX_CHANNELS]; int src_channel[DD_EXR_MAX_CHANNELS]; } dd_exr_source;
int dd_exr_pack(const dd_exr_chunk* chunks_host, const dd_exr_chunk* chunks, int n_chunks, const dd_exr_source* sources_host,
                const dd_exr_source* sources, int n_sources, void* staged, long staged_bytes, dd_stream stream);

/* ---- The packed chunks deflated on the device (csrc/dd_exr_deflate.hip, coder core csrc/dd_deflate_core.h).  Prediction.py:483-510 stores
 * .npy only; this replaces the zlib.compress call of openexr.write_exr's host loop: ONE launch turns every chunk of a batch into a zlib
 * stream, one wave per stream.
 *   stream  : src_bytes bytes at src + src_offset -> a zlib stream (RFC 1950 around RFC 1951, 32 KiB window, the Adler-32 of the source
 *             bytes) at out + dst_offset (16-byte aligned) of at most dst_capacity bytes.  The host passes src_bytes - 1: a chunk that does
 *             not shrink is stored raw, the format's own rule.
 *   status  : DEVICE int[n_streams]; sizes: DEVICE int[n_streams], the stream's bytes when the status is DD_DEFLATE_OK, else 0.
 *   workspace: DEVICE, dd_exr_deflate_workspace(n_streams) bytes (the token buffers; everything else lives in LDS).
 * The same input gives the same bytes on every run.  Whatever the status, nothing is written outside the stream's own dst_capacity rounded
 * up to 16, or outside its own slice of the workspace.  The table is given twice: the HOST copy is validated here, the DEVICE copy is what
 * the kernel reads -- and checks again (DD_DEFLATE_RECORD).
 * Refused with a negative status and no launch: NULL pointers while n_streams > 0, n_streams < 0, src_bytes outside 1 .. 1 << 30,
 * dst_capacity < 0, a source range leaving src_total, a dst_offset that is negative or not 16-byte aligned or whose dst_capacity rounded up
 * to 16 leaves out_bytes, an output that is not 16-byte aligned, a workspace that is not 4-byte aligned or smaller than
 * dd_exr_deflate_workspace(n_streams), a source that overlaps the output.  n_streams == 0 is
 * a no-op that returns 0.  No host sync. */
#define DD_DEFLATE_OK 0
#define DD_DEFLATE_RAW 1         /* the stream would not fit dst_capacity: the chunk is stored raw */
#define DD_DEFLATE_RECORD 2      /* the device copy of the record does not fit the buffers; nothing is read or written through it */
typedef struct { long long src_offset; long long dst_offset; int src_bytes; int dst_capacity; } dd_exr_deflate_stream;   /* 24 bytes */
long dd_exr_deflate_workspace(int n_streams);
int dd_exr_deflate(const dd_exr_deflate_stream* streams_host, const dd_exr_deflate_stream* streams, int n_streams, const void* src, long src_total,
                   void* out, long out_bytes, void* workspace, long workspace_bytes, int* status, int* sizes, dd_stream stream);

/* ---- Denoised passes as 8-bit sRGB PNGs, packed on the device (csrc/dd_png_encode.hip, row coder csrc/dd_png_core.h).  Prediction.py:483-510
 * stores every denoised pass as .npy only, and its own PNG line (the commented-out `cv2.imwrite(... + '/combined.png', ...)` behind that block,
 * :514-517) never runs; this replaces it: ONE launch turns the fp32 planes of all passes of a frame into FILTERED PNG rows, cut into segments of whole rows.
 *   image   : src fp32 [H, W, C] contiguous; n_channels 3 (RGB, colour type 2) or 1 (gray, colour type 0); byte k of a pixel is
 *             src[y, x, src_channel[k]] * exposure (one fp32 multiply) counted against `thresholds`, DEVICE float[255], the table of
 *             metrics.preview_thresholds that dd_loss_previews takes: byte = number of entries <= v (-inf, negatives, -0.0 -> 0, +inf -> 255).
 *             A NaN in any channel makes an RGB pixel (255, 0, 255), a NaN gray sample 0.
 *   segment : rows y0 .. y0 + rows of image `image`: n = rows * (1 + W * n_channels) bytes -- per row the filter type (0 None, 1 Sub, 2 Up,
 *             3 Average, 4 Paeth: the one with the smallest sum of |filtered byte as signed 8-bit|, ties to the lowest number; the row above
 *             row 0 is zeros) and the filtered bytes -- written to staged + offset (16-byte aligned; the segment owns the bytes up to the next
 *             multiple of 16: the padding is written as zero, nothing outside).  W * n_channels <= DD_PNG_MAX_ROW_BYTES and
 *             n <= DD_PNG_STAGE_BYTES: a segment is staged in the workgroup's LDS.
 * Both tables are given twice: the HOST copy is validated here, the DEVICE copy is what the kernel reads -- and checks again: a segment that
 * does not fit its image or the staged buffer writes nothing.
 * Refused with a negative status and no launch: NULL tables, thresholds or buffer while n_segments > 0, n_segments < 0, n_images < 1,
 * staged_bytes < 16, an image with a null plane, H < 1 or W < 1, C outside 1 .. 32, n_channels other than 1 or 3, a src_channel outside
 * [0, C), a row of more than DD_PNG_MAX_ROW_BYTES bytes, a plane that overlaps the staged buffer, a segment whose image index or rows do not
 * fit its image or whose bytes exceed DD_PNG_STAGE_BYTES, an offset that is not 16-byte aligned or leaves staged_bytes, a staged buffer that
 * is not 16-byte aligned, thresholds that are not 4-byte aligned.  n_segments == 0 is a no-op that returns 0.  No host sync. */
#define DD_PNG_MAX_ROW_BYTES 12288   /* W * n_channels of an image: two row buffers of this size in LDS */
#define DD_PNG_STAGE_BYTES 36864     /* the bytes of a segment: the staging buffer in LDS */
typedef struct { const float* src; int H; int W; int C; int n_channels; int src_channel[3]; float exposure; } dd_png_image;   /* 40 bytes */
typedef struct { long long offset; int image; int y0; int rows; int reserved; } dd_png_segment;                              /* 24 bytes */
int dd_png_pack(const dd_png_segment* segments_host, const dd_png_segment* segments, int n_segments, const dd_png_image* images_host,
                const dd_png_image* images, int n_images, const float* thresholds, void* staged, long staged_bytes, dd_stream stream);

/* ---- The packed segments deflated on the device (csrc/dd_png_encode.hip, coder core csrc/dd_deflate_core.h in its segment framing).
 * Prediction.py:483-510 stores .npy only (its PNG line, the commented-out `cv2.imwrite(... + '/combined.png', ...)` at :514-517, would have
 * compressed on the host); ONE launch turns every segment of every pass into a raw-deflate body (RFC 1951), one wave per segment.  The bodies of a file's
 * segments, in order, behind the two bytes 78 01 and in front of the Adler-32 of all filtered bytes, are the zlib stream of its IDAT chunk.
 *   stream  : src_bytes bytes at src + src_offset -> at most dst_capacity bytes at out + dst_offset (16-byte aligned).  last == 0: no block
 *             is final and the body ends with an empty stored block (three zero bits, zero bits up to the byte border, 00 00 FF FF), so it
 *             ends on a byte border; last == 1: the last block is final and padded to the byte border.  The host passes src_bytes - 1: a
 *             segment that does not shrink (DD_DEFLATE_RAW) is written as stored blocks by the host.
 *   status  : DEVICE int[n_streams] (DD_DEFLATE_*); sizes: DEVICE int[n_streams], the body's bytes when the status is DD_DEFLATE_OK, else 0;
 *   adler   : DEVICE unsigned[n_streams], the Adler-32 of the stream's source bytes when the status is OK or RAW (the host combines them).
 *   workspace: DEVICE, dd_png_deflate_workspace(n_streams) bytes.
 * The same input gives the same bytes on every run.  Whatever the status, nothing is written outside the stream's own dst_capacity rounded up
 * to 16, or outside its own slice of the workspace.  The table is given twice: the HOST copy is validated here, the DEVICE copy is what the
 * kernel reads -- and checks again (DD_DEFLATE_RECORD).
 * Refused with a negative status and no launch: NULL pointers while n_streams > 0, n_streams < 0, src_bytes outside 1 .. 1 << 30,
 * dst_capacity < 0, last other than 0 or 1, a source range leaving src_total, a dst_offset that is negative or not 16-byte aligned or whose
 * dst_capacity rounded up to 16 leaves out_bytes, an output that is not 16-byte aligned, a workspace that is not 4-byte aligned or smaller
 * than dd_png_deflate_workspace(n_streams), a source that overlaps the output.  n_streams == 0 is a no-op that returns 0.  No host sync. */
typedef struct { long long src_offset; long long dst_offset; int src_bytes; int dst_capacity; int last; int reserved; } dd_png_stream;   /* 32 bytes */
long dd_png_deflate_workspace(int n_streams);
int dd_png_deflate(const dd_png_stream* streams_host, const dd_png_stream* streams, int n_streams, const void* src, long src_total, void* out,
                   long out_bytes, void* workspace, long workspace_bytes, int* status, int* sizes, unsigned* adler, dd_stream stream);

/* 3x3/s2 transpose conv (Tiramisu.py:62-64) = 3x3 SAME conv of the zero-stuffed input with the flipped kernel:
 * y[B,2H,2W,C] = 0 except y[2i+1,2j+1] = x[i,j]; and its adjoint dx[i,j] (+)= dy[2i+1,2j+1] * (mask>0). */
int dd_zero_stuff(const void* x, int ldx, void* y, int ldy, int C, int B, int H, int W, int dtype, dd_stream stream);
int dd_zero_unstuff(const void* dy, int lddy, void* dx, int lddx, const void* mask, int ldmask, int C, int B, int H, int W,
                    int accumulate, int dtype, dd_stream stream);

/* ---- backward of the 3x3/s2 transposed conv WITHOUT the zero-stuffed form (bf16 / f16 storage).  TensorFlow differentiates
 * tf.layers.conv2d_transpose (Tiramisu.py:60-65) into a stride-2 conv of the output gradient (the data gradient) and a filter gradient over the
 * output grid (Training.py:701-702).  With dy rearranged by output parity,
 *   s[b][i][j][(py*2 + px)*cp + co] = dy[b][2i + py][2j + px][co]        (dd_space_to_depth2; cp = cout rounded up to 16, the padding zero),
 * both become dense work on the INPUT grid:
 *   dx[i][j][ci]     = sum over the 9 taps (a, b) of  s[i + (a == 2)][j + (b == 2)][plane(a, b)*cp + co] * K[a][b][co][ci],  plane = (a & 1)*2 + (b & 1)
 *                      = dd_conv3x3_ks mode 6 over s (a 2 x 2-tap conv with offsets 0 / +1: 16 cout MACs per input pixel and ci against the 36 of
 *                      the 3x3 conv over the zero-stuffed 2H x 2W image, and no stuffed tensors);
 *   dK[a][b][co][ci] += sum_p s[p + off(a, b)][plane(a, b)*cp + co] * x[p][ci]      (dd_convt3_wgrad: exactly the 9 cout cin products per pixel).
 * TensorFlow kernel layout [3][3][cout][cin], fp32 atomics: zero dK first. */
int dd_space_to_depth2(const void* y, int ldy, void* s, int lds, int C, int cp, int B, int H, int W, int dtype, dd_stream stream);
typedef struct {
  const void* s; int lds; int cout; int cp;   /* space-to-depth output gradient [B,H,W,lds], lds >= 4 cp, cp % 16 == 0 */
  const void* x; int ldx; int cin;            /* the layer's input [B,H,W,ldx]; channels up to the next multiple of 8 readable and zero */
  float* dk;                                  /* [3][3][cout][cin] fp32 */
  int B, H, W;                                /* input grid */
  int dtype;
} dd_convt3_wgrad_args;
int dd_convt3_wgrad(const dd_convt3_wgrad_args* a, dd_stream stream);

/* ---- host-side helper (no device work): CRC-32C (Castagnoli) of `n` bytes, continuing from `crc` (0 to start).  The checksum of
 * the reference's on-disk formats: TFRecord framing (TFRecordsCreator.py:233-252) and TensorFlow checkpoint bundles written by the
 * Estimator (Training.py:944-1000 model_dir).  Returns the plain (unmasked) CRC through *out. */
int dd_crc32c(const void* data, size_t n, uint32_t crc, uint32_t* out);

/* ---- probes used by the test-suite to pin hardware fragment layouts the kernels rely on */
int dd_probe_tr16(const uint16_t* lds_image_4096, const int32_t* lane_byte_addr_64, uint16_t* out_64x4, dd_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* DD_HIP_H */
