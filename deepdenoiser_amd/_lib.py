"""ctypes binding of libdd_hip.so (the C-ABI declared in include/dd_hip.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing the compute
layers raises.  (Build it with `python -m deepdenoiser_amd.build`.)
"""

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DD_LIB", os.path.join(_HERE, "libdd_hip.so"))   # DD_LIB: experiment builds (tools/)

DD_F32, DD_BF16, DD_F16 = 0, 1, 2
IN_RELU, OUT_RELU, ACCUM, PIXSHUF, GATHER2X2 = 1, 2, 4, 8, 16
MAX_FEATURES, MAX_COMBINED = 32, 8
METRIC_SOURCES = MAX_FEATURES + MAX_COMBINED + 1      # DD_METRIC_SOURCES: rows of the dd_loss_metrics table per image
# histogram records (dd_histogram_values / dd_loss_histograms): uint32 counts[nb] | double min, max, sum, sum_squares | uint64 num, nonfinite
HISTOGRAM_DIFFERENCE, HISTOGRAM_VARIATION_DIFFERENCE, HISTOGRAM_MASKED_DIFFERENCE = 0, 1, 2
HISTOGRAM_VALUES_SCRATCH_BYTES = 20480
# dd_loss_previews: panel bits, the most images of one launch, the length of the threshold table
PREVIEW_SOURCE, PREVIEW_PREDICTION, PREVIEW_TARGET, PREVIEW_DIFFERENCE = 1, 2, 4, 8
PREVIEW_MAX_IMAGES, PREVIEW_THRESHOLDS = 16, 255
NONFINITE_MAX_PLANES = 32      # DD_NONFINITE_MAX_PLANES
QUALITY_MAX_PAIRS, QUALITY_TILE = 32, 32      # DD_QUALITY_MAX_PAIRS, DD_QUALITY_TILE
TEMPORAL_MAX_PASSES, TEMPORAL_MAX_GUIDES, TEMPORAL_TILE = 32, 4, 16      # DD_TEMPORAL_MAX_PASSES, DD_TEMPORAL_MAX_GUIDES, DD_TEMPORAL_TILE
SEQQ_MAX_PAIRS, SEQQ_TILE = 32, 16      # DD_SEQQ_MAX_PAIRS, DD_SEQQ_TILE
GRAD_CHUNK, GRAD_PARTIAL_BYTES = 4096, 24      # DD_GRAD_CHUNK, DD_GRAD_PARTIAL_BYTES


def histogram_stats_offset(nb):
    """DD_HISTOGRAM_STATS_OFFSET"""
    return (nb + 1) // 2 * 8


def histogram_record_bytes(nb):
    """DD_HISTOGRAM_RECORD_BYTES"""
    return histogram_stats_offset(nb) + 48


# every symbol include/dd_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = (
    "dd_version", "dd_last_error", "dd_pack_weights", "dd_pack_weights_batched", "dd_conv_igemm", "dd_conv_wgrad", "dd_colsum", "dd_colsum_segments",
    "dd_maxpool_fwd", "dd_maxpool_bwd", "dd_avgpool", "dd_prepare_feature", "dd_gather_input",
    "dd_kpcn_fwd", "dd_kpcn_bwd", "dd_kpcn_hidden_fwd", "dd_kpcn_hidden_bwd", "dd_compose_pack", "dd_compose_blend_fwd", "dd_compose_blend_bwd",
    "dd_compose_unpack_bwd", "dd_invert_std_fwd", "dd_invert_std_bwd", "dd_loss_head", "dd_adam_step",
    "dd_stitch", "dd_recombine", "dd_probe_tr16", "dd_masked_add", "dd_zero_stuff", "dd_zero_unstuff", "dd_convert_channels",
    "dd_augment", "dd_loss_mask_sums", "dd_crc32c", "dd_extract_tiles", "dd_compose_net_fwd", "dd_compose_net_bwd",
    "dd_kpcn_head_fwd", "dd_kpcn_head_bwd", "dd_kpcn_head_bwd_multi", "dd_assemble_input", "dd_assemble_input_frames", "dd_conv3x3_bwd", "dd_conv3x3_bwd_multi", "dd_convt2x2_fwd", "dd_convt2x2_bwd", "dd_convt_bwd_wide_count", "dd_conv3x3_ks",
    "dd_conv_pw_count", "dd_wgrad_pw_count", "dd_conv_route_count", "dd_space_to_depth2", "dd_convt3_wgrad", "dd_compose_stream_plan", "dd_compose_bwd_scratch_bytes",
    "dd_loss_msssim_scratch_bytes", "dd_loss_msssim_fwd", "dd_loss_msssim_bwd", "dd_loss_msssim_values",
    "dd_loss_metrics_scratch_bytes", "dd_loss_metrics", "dd_loss_head_path_count",
    "dd_loss_head_dscale", "dd_loss_msssim_bwd_dscale", "dd_grads_nonfinite", "dd_adam_step_scaled", "dd_scaler_update",
    "dd_histogram_values", "dd_loss_histograms_scratch_bytes", "dd_loss_histograms", "dd_loss_previews",
    "dd_nonfinite_scan", "dd_nonfinite_repair", "dd_frame_quality_scratch_bytes", "dd_frame_quality", "dd_stitch_blend",
    "dd_grad_norms", "dd_adam_step_clipped", "dd_adam_step_scaled_clipped", "dd_sample_tiles",
    "dd_tile_statistics", "dd_importance_cells", "dd_importance_update", "dd_exr_reconstruct", "dd_exr_inflate",
    "dd_exr_pack", "dd_exr_deflate_workspace", "dd_exr_deflate", "dd_png_pack", "dd_png_deflate_workspace", "dd_png_deflate",
    "dd_temporal_scratch_bytes", "dd_temporal_stabilize", "dd_sequence_quality_scratch_bytes", "dd_sequence_quality",
)


# enum dd_conv_route (include/dd_hip.h): the kernels dd_conv_igemm / dd_conv3x3_ks / dd_conv_wgrad route a call to, in the header's order
ROUTES = ("igemm_resident", "igemm_streamed", "igemm_ws", "rw_6_2", "rw12", "rw12_mask", "rw12_res", "rw8_kc2", "rw8_kc4", "rw8_kc4_mask", "pw",
          "ks", "ks_pw_taps", "wgrad_dma", "wgrad_reg", "wgrad_pw", "wgrad_stacked")


def route_counts():
    """{route name: launches this process sent down it} (dd_conv_route_count)."""
    lib = load()
    return {name: lib.dd_conv_route_count(r) for r, name in enumerate(ROUTES)}


# sub-counts behind the routes (the header's order goes on): launches already counted under a route that took a narrower instantiation
SUBROUTES = ("rw8_k32",)


def subroute_counts():
    """{sub-count name: launches}: rw8_k32 = the launches of rw8_kc2 that ran conv_rw8_kernel with one K chunk."""
    lib = load()
    return {name: lib.dd_conv_route_count(len(ROUTES) + r) for r, name in enumerate(SUBROUTES)}


class ConvT3WgradArgs(C.Structure):
    """dd_convt3_wgrad_args (include/dd_hip.h)."""
    _fields_ = [("s", C.c_void_p), ("lds", C.c_int), ("cout", C.c_int), ("cp", C.c_int),
                ("x", C.c_void_p), ("ldx", C.c_int), ("cin", C.c_int),
                ("dk", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class ConvArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("cin", C.c_int),
                ("wp", C.c_void_p), ("k_pad", C.c_int), ("n_pad", C.c_int),
                ("bias", C.c_void_p), ("nbias", C.c_int),
                ("res", C.c_void_p), ("ldres", C.c_int),
                ("mask", C.c_void_p), ("ldmask", C.c_int),
                ("y", C.c_void_p), ("ldy", C.c_int), ("n", C.c_int),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("taps", C.c_int), ("flags", C.c_int), ("dtype", C.c_int)]


class WgradArgs(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ldp", C.c_int), ("m", C.c_int),
                ("q", C.c_void_p), ("ldq", C.c_int), ("n", C.c_int),
                ("out", C.c_void_p), ("bias_out", C.c_void_p), ("bias_mode", C.c_int),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("taps", C.c_int), ("flags", C.c_int), ("dtype", C.c_int), ("ksplit", C.c_int),
                ("stack_blocks", C.c_int), ("stack_width", C.c_int), ("stack_m0", C.c_int),
                ("stack_out", C.c_void_p * 8), ("stack_bias", C.c_void_p * 8)]


class ConvBwdArgs(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("ld_dy", C.c_int), ("cout", C.c_int),
                ("x", C.c_void_p), ("ld_x", C.c_int), ("cin", C.c_int),
                ("wd", C.c_void_p), ("n_pad", C.c_int), ("k_pad", C.c_int),
                ("dx", C.c_void_p), ("ld_dx", C.c_int),
                ("dw", C.c_void_p), ("db", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("use_mask", C.c_int), ("accumulate", C.c_int), ("dtype", C.c_int)]


class ConvTArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ld_x", C.c_int), ("cin", C.c_int),
                ("y", C.c_void_p), ("ld_y", C.c_int), ("cout", C.c_int),
                ("w", C.c_void_p), ("n_pad", C.c_int), ("k_pad", C.c_int),
                ("bias", C.c_void_p), ("relu", C.c_int),
                ("dx", C.c_void_p), ("ld_dx", C.c_int), ("dw", C.c_void_p), ("db", C.c_void_p), ("use_mask", C.c_int), ("accumulate", C.c_int),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class ConvKsArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("cin", C.c_int),
                ("wp", C.c_void_p), ("n_pad", C.c_int), ("k_pad", C.c_int),
                ("bias", C.c_void_p), ("nbias", C.c_int),
                ("y", C.c_void_p), ("ldy", C.c_int),
                ("n0", C.c_int), ("n", C.c_int),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("mode", C.c_int), ("flags", C.c_int), ("dtype", C.c_int),
                ("mask", C.c_void_p), ("ldmask", C.c_int)]


class PackDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("taps", C.c_int), ("n", C.c_int), ("k", C.c_int), ("n_pad", C.c_int),
                ("k_pad", C.c_int), ("tap_flip", C.c_int), ("s_tap", C.c_long), ("s_n", C.c_long), ("s_k", C.c_long),
                ("dst_ld", C.c_long), ("dst_tap_stride", C.c_long)]


class FeatureParams(C.Structure):
    _fields_ = [("use_log1p", C.c_int), ("mean", C.c_float), ("inv_std", C.c_float),
                ("use_variance", C.c_int), ("variance_before", C.c_int), ("mode_neighbor", C.c_int),
                ("relative", C.c_int), ("compress", C.c_int), ("epsilon", C.c_float)]


class GatherEntry(C.Structure):
    _fields_ = [("src", C.c_void_p), ("pixel_stride", C.c_int), ("batch_stride_pixels", C.c_int),
                ("nch", C.c_int), ("dst_ch", C.c_int)]


class AssembleEntry(C.Structure):
    _fields_ = [("src", C.c_void_p), ("cs", C.c_int), ("kind", C.c_int), ("fp", FeatureParams), ("nch", C.c_int), ("dst_ch", C.c_int),
                ("std_out", C.c_void_p), ("ld_std", C.c_int)]


class LossDesc(C.Structure):
    _fields_ = [("n_features", C.c_int),
                ("pred", C.c_void_p * MAX_FEATURES), ("target", C.c_void_p * MAX_FEATURES),
                ("dpred", C.c_void_p * MAX_FEATURES),
                ("target_ld", C.c_int * MAX_FEATURES), ("pred_ld", C.c_int * MAX_FEATURES), ("nch", C.c_int * MAX_FEATURES),
                ("weight", C.c_float * MAX_FEATURES), ("var_weight", C.c_float * MAX_FEATURES),
                ("masked_weight", C.c_float * MAX_FEATURES), ("mask_feature", C.c_int * MAX_FEATURES),
                ("n_combined", C.c_int), ("comb", (C.c_int * 3) * MAX_COMBINED),
                ("comb_weight", C.c_float * MAX_COMBINED), ("comb_var_weight", C.c_float * MAX_COMBINED),
                ("comb_masked_weight", C.c_float * MAX_COMBINED), ("comb_mask_feature", C.c_int * MAX_COMBINED),
                ("n_image_combined", C.c_int), ("image_combined", C.c_int * MAX_COMBINED),
                ("n_image_features", C.c_int), ("image_features", C.c_int * MAX_FEATURES),
                ("image_weight", C.c_float), ("image_var_weight", C.c_float), ("kind", C.c_int), ("epsilon", C.c_float),
                ("mask_sums", C.c_void_p),
                ("pred_std", C.c_void_p * MAX_FEATURES), ("pred_inv", C.c_void_p * MAX_FEATURES),
                ("inv_log1p", C.c_int * MAX_FEATURES), ("inv_mean", C.c_float * MAX_FEATURES), ("inv_std", C.c_float * MAX_FEATURES)]


class MsSsimDesc(C.Structure):      # dd_loss_msssim_desc
    _fields_ = [("n_features", C.c_int),
                ("pred", C.c_void_p * MAX_FEATURES), ("target", C.c_void_p * MAX_FEATURES), ("dpred", C.c_void_p * MAX_FEATURES),
                ("target_ld", C.c_int * MAX_FEATURES), ("pred_ld", C.c_int * MAX_FEATURES), ("nch", C.c_int * MAX_FEATURES),
                ("ssim_weight", C.c_float * MAX_FEATURES),
                ("n_combined", C.c_int), ("comb", (C.c_int * 3) * MAX_COMBINED), ("comb_ssim_weight", C.c_float * MAX_COMBINED),
                ("n_image_combined", C.c_int), ("image_combined", C.c_int * MAX_COMBINED),
                ("n_image_features", C.c_int), ("image_features", C.c_int * MAX_FEATURES),
                ("image_ssim_weight", C.c_float)]


class ScalerState(C.Structure):
    """dd_scaler_state (include/dd_hip.h): the device-resident record of the dynamic loss scale.  Five 4-byte words; `scale` is the first, so a
    pointer to the record is a pointer to the scale (what the *_dscale loss launches take)."""
    _fields_ = [("scale", C.c_float), ("good_steps", C.c_int), ("found_nonfinite", C.c_int), ("adam_t", C.c_int), ("skipped_total", C.c_int)]


class GradChunk(C.Structure):          # dd_grad_chunk: one row of the chunk table of dd_grad_norms (16 bytes)
    _fields_ = [("offset", C.c_long), ("length", C.c_int), ("variable", C.c_int)]


class GradVarNorms(C.Structure):       # dd_grad_var_norms: what dd_grad_norms leaves per variable in device memory (24 bytes)
    _fields_ = [("grad_sq", C.c_double), ("weight_sq", C.c_double), ("nonfinite", C.c_uint), ("reserved", C.c_uint)]


class GradClip(C.Structure):           # dd_grad_clip: the clip record of dd_grad_norms, read by the *_clipped Adam launches (five 4-byte words)
    _fields_ = [("grad_norm", C.c_float), ("coef", C.c_float), ("grad_factor", C.c_float), ("nonfinite_variables", C.c_uint),
                ("nonfinite_total", C.c_uint)]


class AugmentDraw(C.Structure):
    _fields_ = [("flip", C.c_int), ("rotate", C.c_int), ("permute", C.c_int), ("normal_rotation", C.c_float * 9)]


AUG_PLAIN, AUG_RGB, AUG_NORMAL, AUG_SCREEN_NORMAL = 0, 1, 2, 3
TILE_MAX_PASSES = 64      # DD_TILE_MAX_PASSES


class TileRecord(C.Structure):         # dd_tile_record: one example of dd_sample_tiles, in device memory (64 bytes)
    _fields_ = [("source_plane", C.c_int), ("target_plane", C.c_int), ("y0", C.c_int), ("x0", C.c_int), ("draw", AugmentDraw)]


class TilePass(C.Structure):           # dd_tile_pass: `planes` is a device array of n_planes base pointers
    _fields_ = [("planes", C.c_void_p), ("dst", C.c_void_p), ("C", C.c_int), ("kind", C.c_int), ("ld_dst", C.c_int), ("from_target", C.c_int)]


class TileSamplerDesc(C.Structure):    # dd_tile_sampler_desc: a host struct, `plane_hw` is the device table [n_planes][2] of (h, w)
    _fields_ = [("n_passes", C.c_int), ("n_planes", C.c_int), ("plane_hw", C.c_void_p), ("pass_", TilePass * TILE_MAX_PASSES)]


STAT_MAX_PASSES = 64      # DD_STAT_MAX_PASSES
# the fields of a dd_tile_statistics row, in the order of the header's enum (DD_STAT_*)
STAT_FIELD_NAMES = ("present", "min", "max", "min_log1p", "max_log1p", "pivot", "pivot_log1p", "sum", "sum_sq", "sum_log1p", "sum_sq_log1p",
                    "count", "mask_sum", "masked_sum", "masked_sum_sq", "masked_sum_log1p", "masked_sum_sq_log1p")
STAT_FIELDS = len(STAT_FIELD_NAMES)      # DD_STAT_FIELDS


class StatWindow(C.Structure):         # dd_stat_window: one window of dd_tile_statistics, in device memory (16 bytes)
    _fields_ = [("plane", C.c_int), ("mask_plane", C.c_int), ("y0", C.c_int), ("x0", C.c_int)]


class StatPass(C.Structure):           # dd_stat_pass: `planes` / `mask_planes` are device arrays of n_planes base pointers (mask_planes may be NULL)
    _fields_ = [("planes", C.c_void_p), ("mask_planes", C.c_void_p), ("C", C.c_int), ("is_alpha", C.c_int)]


class StatDesc(C.Structure):           # dd_stat_desc: a host struct, `plane_hw` is the device table [n_planes][2] of (h, w)
    _fields_ = [("n_passes", C.c_int), ("n_planes", C.c_int), ("plane_hw", C.c_void_p), ("pass_", StatPass * STAT_MAX_PASSES)]


IMPORTANCE_MAX_PASSES = 16      # DD_IMPORTANCE_MAX_PASSES


class ImportanceCell(C.Structure):     # dd_importance_cell: one G x G cell of dd_importance_cells, in device memory (16 bytes)
    _fields_ = [("source_plane0", C.c_int), ("target_plane", C.c_int), ("y0", C.c_int), ("x0", C.c_int)]


class ImportancePass(C.Structure):     # dd_importance_pass: `planes` is a device array of n_planes base pointers of a 3-channel colour pass
    _fields_ = [("planes", C.c_void_p)]


class ImportanceDesc(C.Structure):     # dd_importance_desc: a host struct, `plane_hw` is the device table [n_planes][2] of (h, w)
    _fields_ = [("n_passes", C.c_int), ("n_planes", C.c_int), ("plane_hw", C.c_void_p), ("n_sources", C.c_int), ("epsilon", C.c_float),
                ("pass_", ImportancePass * IMPORTANCE_MAX_PASSES)]


class ImportanceUpdatePass(C.Structure):   # dd_importance_update_pass: a 3-channel colour pass, pred fp32 [B,T,T,pred_ld], target fp32 [B,T,T,target_ld]
    _fields_ = [("pred", C.c_void_p), ("target", C.c_void_p), ("pred_ld", C.c_int), ("target_ld", C.c_int)]


class ImportanceUpdateDesc(C.Structure):   # dd_importance_update_desc: a host struct, `plane_hw` and `cell_base` are device tables over the planes
    _fields_ = [("n_passes", C.c_int), ("n_planes", C.c_int), ("plane_hw", C.c_void_p), ("cell_base", C.c_void_p), ("epsilon", C.c_float),
                ("pass_", ImportanceUpdatePass * IMPORTANCE_MAX_PASSES)]


EXR_MAX_CHANNELS = 8            # DD_EXR_MAX_CHANNELS
EXR_MAX_STREAM_BYTES = 1 << 30  # dd_exr_inflate / dd_exr_deflate refuse a stream with more bytes to write / to read


class ExrChunk(C.Structure):           # dd_exr_chunk: one scan-line chunk in the staged buffer of dd_exr_reconstruct (24 bytes)
    _fields_ = [("offset", C.c_longlong), ("file", C.c_int), ("row0", C.c_int), ("rows", C.c_int), ("coded", C.c_int)]


class ExrFile(C.Structure):            # dd_exr_file: the plane a file is decoded into and, per file channel, its pixel type and destination set
    _fields_ = [("dst", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("n_channels", C.c_int),
                ("type", C.c_int * EXR_MAX_CHANNELS), ("dst_mask", C.c_uint * EXR_MAX_CHANNELS)]


class ExrStream(C.Structure):          # dd_exr_stream: one zlib stream of dd_exr_inflate and where its bytes go in the staged buffer (24 bytes)
    _fields_ = [("src_offset", C.c_longlong), ("dst_offset", C.c_longlong), ("src_bytes", C.c_int), ("dst_bytes", C.c_int)]


class ExrSource(C.Structure):          # dd_exr_source: the fp32 plane a file is packed from and, per file channel, its pixel type and plane channel
    _fields_ = [("src", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("n_channels", C.c_int),
                ("type", C.c_int * EXR_MAX_CHANNELS), ("src_channel", C.c_int * EXR_MAX_CHANNELS)]


class ExrDeflateStream(C.Structure):   # dd_exr_deflate_stream: one packed chunk of dd_exr_deflate and the slot of its zlib stream (24 bytes)
    _fields_ = [("src_offset", C.c_longlong), ("dst_offset", C.c_longlong), ("src_bytes", C.c_int), ("dst_capacity", C.c_int)]


PNG_MAX_ROW_BYTES, PNG_STAGE_BYTES = 12288, 36864      # DD_PNG_MAX_ROW_BYTES, DD_PNG_STAGE_BYTES: what the pack kernel holds in LDS


class PngImage(C.Structure):           # dd_png_image: the fp32 plane a PNG is packed from, its sample channels and the exposure (40 bytes)
    _fields_ = [("src", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("n_channels", C.c_int), ("src_channel", C.c_int * 3),
                ("exposure", C.c_float)]


class PngSegment(C.Structure):         # dd_png_segment: rows y0 .. y0 + rows of an image and the slot of their filtered bytes (24 bytes)
    _fields_ = [("offset", C.c_longlong), ("image", C.c_int), ("y0", C.c_int), ("rows", C.c_int), ("reserved", C.c_int)]


class PngStream(C.Structure):          # dd_png_stream: one packed segment of dd_png_deflate and the slot of its raw-deflate body (32 bytes)
    _fields_ = [("src_offset", C.c_longlong), ("dst_offset", C.c_longlong), ("src_bytes", C.c_int), ("dst_capacity", C.c_int), ("last", C.c_int),
                ("reserved", C.c_int)]


# DD_DEFLATE_*: the per-stream status codes of dd_exr_deflate and dd_png_deflate
DEFLATE_OK, DEFLATE_RAW, DEFLATE_RECORD = range(3)
DEFLATE_STATUS_NAMES = ("OK", "RAW", "RECORD")
DEFLATE_BLOCK_TOKENS = 16384     # DD_DEFLATE_BLOCK_TOKENS (csrc/dd_deflate_core.h): 32-bit tokens per stream in the workspace

# DD_INFLATE_*: the per-stream status codes of dd_exr_inflate
(INFLATE_OK, INFLATE_HEADER, INFLATE_TRUNCATED, INFLATE_BLOCK_TYPE, INFLATE_STORED, INFLATE_LENGTHS, INFLATE_SYMBOL, INFLATE_DISTANCE,
 INFLATE_OVERRUN, INFLATE_SHORT, INFLATE_CHECK, INFLATE_RECORD) = range(12)
INFLATE_STATUS_NAMES = ("OK", "HEADER", "TRUNCATED", "BLOCK_TYPE", "STORED", "LENGTHS", "SYMBOL", "DISTANCE", "OVERRUN", "SHORT", "CHECK", "RECORD")


class StitchEntry(C.Structure):
    _fields_ = [("tile", C.c_int), ("crop_y0", C.c_int), ("crop_y1", C.c_int), ("crop_x0", C.c_int),
                ("crop_x1", C.c_int), ("dst_img", C.c_int), ("dst_y", C.c_int), ("dst_x", C.c_int)]


class BlendAxis(C.Structure):          # dd_blend_axis: `origins` is a host array, the other tables are device memory
    _fields_ = [("count", C.c_int), ("origins", C.POINTER(C.c_int)), ("origins_dev", C.c_void_p), ("weights", C.c_void_p),
                ("first", C.c_void_p), ("last", C.c_void_p)]


class ComposeArgs(C.Structure):
    _fields_ = [("small", C.c_void_p), ("ld_small", C.c_int), ("fine", C.c_void_p), ("ld_fine", C.c_int), ("out", C.c_void_p), ("ld_out", C.c_int),
                ("w_in", C.c_void_p), ("b_in", C.c_void_p), ("w_res", C.c_void_p * 4), ("b_res", C.c_void_p * 4),
                ("w_out", C.c_void_p), ("b_out", C.c_void_p),
                ("save_netin", C.c_void_p), ("ld_netin", C.c_int), ("save_act", C.c_void_p * 5), ("ld_act", C.c_int * 5),
                ("save_wl", C.c_void_p), ("ld_wl", C.c_int),
                ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int)]


class ComposeBwdArgs(C.Structure):
    _fields_ = [("small", C.c_void_p), ("ld_small", C.c_int), ("fine", C.c_void_p), ("ld_fine", C.c_int), ("dout", C.c_void_p), ("ld_dout", C.c_int),
                ("act", C.c_void_p * 5), ("ld_act", C.c_int * 5), ("wl", C.c_void_p), ("ld_wl", C.c_int),
                ("w_in", C.c_void_p), ("w_res", C.c_void_p * 4), ("w_out", C.c_void_p),
                ("d_small", C.c_void_p), ("ld_dsmall", C.c_int), ("accumulate_small", C.c_int), ("d_fine", C.c_void_p), ("ld_dfine", C.c_int),
                ("dw_in", C.c_void_p), ("db_in", C.c_void_p), ("dw_res", C.c_void_p * 4), ("db_res", C.c_void_p * 4),
                ("dw_out", C.c_void_p), ("db_out", C.c_void_p),
                ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("dtype", C.c_int),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_long)]


class HeadArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("C", C.c_int), ("src", C.c_void_p), ("ldsrc", C.c_int),
                ("wa", C.c_void_p), ("ba", C.c_void_p), ("wb", C.c_void_p), ("bb", C.c_void_p),
                ("out", C.c_void_p), ("ld_out", C.c_int), ("dout", C.c_void_p), ("ld_dout", C.c_int),
                ("dx", C.c_void_p), ("ld_dx", C.c_int), ("accumulate_dx", C.c_int),
                ("dwa", C.c_void_p), ("dba", C.c_void_p), ("dwb", C.c_void_p), ("dbb", C.c_void_p),
                ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("ksize", C.c_int), ("dtype", C.c_int)]


class RecombineDesc(C.Structure):
    _fields_ = [("n_triples", C.c_int), ("color", C.c_void_p * 4), ("direct", C.c_void_p * 4), ("indirect", C.c_void_p * 4),
                ("combined", C.c_void_p * 4), ("n_singles", C.c_int), ("single", C.c_void_p * 8), ("image", C.c_void_p)]


class NonfinitePlane(C.Structure):      # dd_nonfinite_plane
    _fields_ = [("data", C.c_void_p), ("C", C.c_int), ("ld", C.c_int), ("mask", C.c_void_p)]


class NonfiniteDesc(C.Structure):       # dd_nonfinite_desc
    _fields_ = [("n_planes", C.c_int), ("plane", NonfinitePlane * NONFINITE_MAX_PLANES)]


class QualityPair(C.Structure):         # dd_quality_pair
    _fields_ = [("pred", C.c_void_p), ("target", C.c_void_p), ("pred_ld", C.c_int), ("target_ld", C.c_int), ("nch", C.c_int)]


class QualityRecord(C.Structure):       # dd_quality_record: what dd_frame_quality leaves per pair in device memory (72 bytes)
    _fields_ = [("pixels_valid", C.c_uint64), ("windows_valid", C.c_uint64), ("ldr_sq_err", C.c_uint64),
                ("se", C.c_double), ("ae", C.c_double), ("rse", C.c_double), ("smape", C.c_double), ("ssim_sum", C.c_double),
                ("max_abs", C.c_float), ("reserved", C.c_float)]


class TemporalPass(C.Structure):        # dd_temporal_pass (40 bytes)
    _fields_ = [("current", C.c_void_p), ("history", C.c_void_p), ("out", C.c_void_p), ("current_ld", C.c_int), ("history_ld", C.c_int),
                ("out_ld", C.c_int), ("nch", C.c_int)]


class TemporalGuide(C.Structure):       # dd_temporal_guide (32 bytes)
    _fields_ = [("current", C.c_void_p), ("previous", C.c_void_p), ("current_ld", C.c_int), ("previous_ld", C.c_int), ("nch", C.c_int),
                ("tolerance", C.c_float)]


class TemporalRecord(C.Structure):      # dd_temporal_record: what dd_temporal_stabilize leaves per pass in device memory (64 bytes)
    _fields_ = [("pixels_offscreen", C.c_uint64), ("pixels_guide", C.c_uint64), ("pixels_nonfinite", C.c_uint64), ("pixels_blended", C.c_uint64),
                ("values_clamped", C.c_uint64), ("change", C.c_double), ("flicker_before", C.c_double), ("flicker_after", C.c_double)]


class SequenceQualityPair(C.Structure):        # dd_seqq_pair (56 bytes)
    _fields_ = [("pred", C.c_void_p), ("pred_previous", C.c_void_p), ("target", C.c_void_p), ("target_previous", C.c_void_p), ("pred_ld", C.c_int),
                ("pred_previous_ld", C.c_int), ("target_ld", C.c_int), ("target_previous_ld", C.c_int), ("nch", C.c_int)]


class SequenceQualityRecord(C.Structure):      # dd_seqq_record: what dd_sequence_quality leaves per pair in device memory (72 bytes)
    _fields_ = [("pixels_offscreen", C.c_uint64), ("pixels_nonfinite", C.c_uint64), ("pixels_valid", C.c_uint64), ("change_prediction", C.c_double),
                ("change_target", C.c_double), ("temporal_error", C.c_double), ("ldr_change_prediction", C.c_double), ("ldr_change_target", C.c_double),
                ("ldr_temporal_error", C.c_double)]


_lib = None


def _check_source_hash(lib):
    """The .so travels prebuilt (git-ignored) next to its sources: refuse one that was built from different sources (dd_version() carries
    the hash of csrc/* and include/dd_hip.h it was compiled from, deepdenoiser_amd/build.py).  DD_LIB experiment builds are exempt."""
    if "DD_LIB" in os.environ:
        return
    from . import build as _build
    try:
        want = _build.source_hash()
    except OSError:          # an installation without the sources next to the library: nothing to compare with
        return
    got = lib.dd_version().decode()
    if ("src=" + want) not in got:
        raise RuntimeError("libdd_hip.so is stale: built from sources %s, the sources here hash to %s -- run `python -m deepdenoiser_amd.build`"
                           % (got.split("src=")[-1], want))


def source_hash():
    """Hash of the kernel sources the loaded library was built from (== build.source_hash() of the tree, checked at load time)."""
    return load().dd_version().decode().split("src=")[-1]


def load():
    """Returns the loaded library; raises RuntimeError (never falls back) if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (same SONAME as /opt/rocm's): it must be loaded FIRST so that this library binds
    # to the runtime that owns torch's streams and allocations (otherwise two runtimes coexist and no device is found).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libdd_hip.so is not built (%s missing): run `python -m deepdenoiser_amd.build`. "
                           "There is no CPU/PyTorch fallback for the hot path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError("libdd_hip.so lacks symbols %s: rebuild it" % missing)
    lib.dd_version.restype = C.c_char_p
    lib.dd_last_error.restype = C.c_char_p
    _check_source_hash(lib)
    for s in SYMBOLS[2:]:
        getattr(lib, s).restype = C.c_int
    vp, i, l, f = C.c_void_p, C.c_int, C.c_long, C.c_float
    lib.dd_pack_weights.argtypes = [vp, vp, i, i, i, i, i, i, l, l, l, i, vp]
    lib.dd_pack_weights_batched.argtypes = [vp, i, i, vp]
    lib.dd_conv_igemm.argtypes = [C.POINTER(ConvArgs), vp]
    lib.dd_conv_wgrad.argtypes = [C.POINTER(WgradArgs), vp]
    lib.dd_conv3x3_bwd.argtypes = [C.POINTER(ConvBwdArgs), vp]
    lib.dd_conv3x3_bwd_multi.argtypes = [C.POINTER(ConvBwdArgs), i, vp]
    lib.dd_convt2x2_fwd.argtypes = [C.POINTER(ConvTArgs), vp]
    lib.dd_convt2x2_bwd.argtypes = [C.POINTER(ConvTArgs), vp]
    lib.dd_conv3x3_ks.argtypes = [C.POINTER(ConvKsArgs), vp]
    lib.dd_space_to_depth2.argtypes = [vp, i, vp, i, i, i, i, i, i, i, vp]
    lib.dd_convt3_wgrad.argtypes = [C.POINTER(ConvT3WgradArgs), vp]
    lib.dd_conv_pw_count.argtypes = []
    lib.dd_conv_pw_count.restype = C.c_long
    lib.dd_wgrad_pw_count.argtypes = []
    lib.dd_wgrad_pw_count.restype = C.c_long
    lib.dd_convt_bwd_wide_count.argtypes = []
    lib.dd_convt_bwd_wide_count.restype = C.c_long
    lib.dd_conv_route_count.argtypes = [i]
    lib.dd_conv_route_count.restype = C.c_long
    lib.dd_colsum.argtypes = [vp, i, i, l, vp, i, vp]
    lib.dd_colsum_segments.argtypes = [vp, i, i, l, i, vp, i, vp, i, vp]
    lib.dd_maxpool_fwd.argtypes = [vp, i, vp, i, vp, i, i, i, i, i, i, i, i, vp]
    lib.dd_maxpool_bwd.argtypes = [vp, i, vp, vp, i, vp, i, i, i, i, i, i, i, i, i, vp]
    lib.dd_avgpool.argtypes = [vp, i, vp, i, i, i, i, i, i, vp]
    lib.dd_prepare_feature.argtypes = [vp, i, vp, i, C.POINTER(FeatureParams), i, i, i, vp]
    lib.dd_gather_input.argtypes = [vp, i, i, vp, i, i, i, i, i, i, vp]
    lib.dd_kpcn_fwd.argtypes = [vp, i, vp, i, vp, i, i, i, i, i, i, vp]
    lib.dd_kpcn_bwd.argtypes = [vp, i, vp, i, vp, i, vp, i, i, i, i, i, i, i, vp]
    lib.dd_kpcn_hidden_fwd.argtypes = [vp, i, vp, i, i, vp, i, vp, vp, i, i, i, i, i, i, vp]
    lib.dd_kpcn_hidden_bwd.argtypes = [vp, i, vp, i, i, vp, i, vp, vp, i, vp, i, i, i, i, i, i, i, vp]
    lib.dd_compose_pack.argtypes = [vp, i, vp, i, vp, i, i, i, i, i, i, vp]
    lib.dd_compose_blend_fwd.argtypes = [vp, i, vp, i, vp, i, vp, i, i, i, i, i, vp]
    lib.dd_compose_blend_bwd.argtypes = [vp, i, vp, i, vp, i, vp, i, vp, i, i, vp, i, vp, i, i, i, i, i, i, vp]
    lib.dd_compose_unpack_bwd.argtypes = [vp, i, vp, i, vp, i, i, i, i, i, vp]
    lib.dd_invert_std_fwd.argtypes = [vp, vp, l, i, f, f, vp]
    lib.dd_invert_std_bwd.argtypes = [vp, vp, vp, l, i, f, f, vp]
    lib.dd_loss_head.argtypes = [C.POINTER(LossDesc), i, i, i, vp, f, vp]
    lib.dd_loss_head_path_count.argtypes = [i]
    lib.dd_loss_head_path_count.restype = C.c_long
    lib.dd_loss_msssim_scratch_bytes.argtypes = [i, i, i, i]
    lib.dd_loss_msssim_scratch_bytes.restype = C.c_long
    lib.dd_loss_msssim_fwd.argtypes = [C.POINTER(MsSsimDesc), i, i, i, vp, vp, vp]
    lib.dd_loss_msssim_bwd.argtypes = [C.POINTER(MsSsimDesc), i, i, i, vp, f, vp]
    lib.dd_loss_msssim_values.argtypes = [C.POINTER(MsSsimDesc), i, i, i, vp, vp, vp]
    lib.dd_loss_metrics_scratch_bytes.argtypes = [i, i, i]
    lib.dd_loss_metrics_scratch_bytes.restype = C.c_long
    lib.dd_loss_metrics.argtypes = [C.POINTER(LossDesc), i, i, i, vp, vp, vp]
    lib.dd_histogram_values.argtypes = [vp, l, vp, i, vp, vp, vp]
    lib.dd_loss_histograms_scratch_bytes.argtypes = [i, i, i, i]
    lib.dd_loss_histograms_scratch_bytes.restype = C.c_long
    lib.dd_loss_histograms.argtypes = [C.POINTER(LossDesc), i, i, i, C.POINTER(C.c_int), i, vp, i, vp, vp, vp]
    lib.dd_loss_previews.argtypes = [C.POINTER(LossDesc), C.POINTER(vp), C.POINTER(C.c_int), i, i, i, C.POINTER(C.c_int), i, C.POINTER(C.c_int), i, i, vp, f, f,
                                     vp, vp]
    lib.dd_adam_step.argtypes = [vp, vp, vp, vp, l, f, f, f, f, f, vp]
    lib.dd_loss_head_dscale.argtypes = [C.POINTER(LossDesc), i, i, i, vp, vp, vp]
    lib.dd_loss_msssim_bwd_dscale.argtypes = [C.POINTER(MsSsimDesc), i, i, i, vp, vp, vp]
    lib.dd_grads_nonfinite.argtypes = [vp, l, vp, vp]
    lib.dd_adam_step_scaled.argtypes = [vp, vp, vp, vp, l, C.c_double, C.c_double, C.c_double, f, f, vp, vp]
    lib.dd_scaler_update.argtypes = [vp, f, f, i, f, f, vp]
    lib.dd_grad_norms.argtypes = [vp, vp, vp, i, vp, i, vp, vp, vp, f, f, vp, vp]
    lib.dd_adam_step_clipped.argtypes = [vp, vp, vp, vp, l, f, f, f, f, f, vp, vp]
    lib.dd_adam_step_scaled_clipped.argtypes = [vp, vp, vp, vp, l, C.c_double, C.c_double, C.c_double, f, f, vp, vp, vp]
    lib.dd_nonfinite_scan.argtypes = [C.POINTER(NonfiniteDesc), i, i, i, vp, vp]
    lib.dd_nonfinite_repair.argtypes = [C.POINTER(NonfiniteDesc), i, i, i, i, vp, vp]
    lib.dd_frame_quality_scratch_bytes.argtypes = [i, i, i]
    lib.dd_frame_quality_scratch_bytes.restype = C.c_long
    lib.dd_frame_quality.argtypes = [C.POINTER(QualityPair), i, i, i, vp, f, f, C.POINTER(vp), vp, vp, vp]
    lib.dd_stitch.argtypes = [vp, i, i, vp, i, i, i, i, vp, i, vp]
    lib.dd_stitch_blend.argtypes = [vp, i, i, i, vp, i, i, i, i, i, C.POINTER(BlendAxis), C.POINTER(BlendAxis), i, i, vp]
    lib.dd_recombine.argtypes = [C.POINTER(RecombineDesc), l, vp]
    lib.dd_probe_tr16.argtypes = [vp, vp, vp, vp]
    lib.dd_masked_add.argtypes = [vp, i, vp, i, vp, i, i, l, i, i, vp]
    lib.dd_convert_channels.argtypes = [vp, i, i, vp, i, i, i, i, l, vp]
    lib.dd_zero_stuff.argtypes = [vp, i, vp, i, i, i, i, i, i, vp]
    lib.dd_zero_unstuff.argtypes = [vp, i, vp, i, vp, i, i, i, i, i, i, i, vp]
    lib.dd_augment.argtypes = [vp, vp, i, i, i, i, vp, i, i, i, i, i, vp]
    lib.dd_loss_mask_sums.argtypes = [vp, i, i, i, vp, vp]
    lib.dd_crc32c.argtypes = [vp, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.dd_extract_tiles.argtypes = [vp, i, i, i, i, vp, i, i, vp, i, vp]
    lib.dd_compose_net_fwd.argtypes = [C.POINTER(ComposeArgs), vp]
    lib.dd_compose_net_bwd.argtypes = [C.POINTER(ComposeBwdArgs), vp]
    lib.dd_compose_stream_plan.argtypes = [i, i, i, i, C.POINTER(C.c_int)]
    lib.dd_compose_bwd_scratch_bytes.argtypes = [i, i, i]
    lib.dd_compose_bwd_scratch_bytes.restype = C.c_long
    lib.dd_assemble_input.argtypes = [vp, i, i, vp, i, i, i, i, i, i, vp]
    lib.dd_assemble_input_frames.argtypes = [vp, i, i, vp, i, i, i, i, i, i, vp, i, i, vp]
    lib.dd_kpcn_head_fwd.argtypes = [C.POINTER(HeadArgs), vp]
    lib.dd_kpcn_head_bwd.argtypes = [C.POINTER(HeadArgs), vp]
    lib.dd_kpcn_head_bwd_multi.argtypes = [C.POINTER(HeadArgs), i, vp]
    lib.dd_sample_tiles.argtypes = [C.POINTER(TileSamplerDesc), vp, i, i, i, i, i, i, vp]
    lib.dd_tile_statistics.argtypes = [C.POINTER(StatDesc), vp, i, i, vp, vp]
    lib.dd_importance_cells.argtypes = [C.POINTER(ImportanceDesc), vp, i, i, vp, vp]
    lib.dd_importance_update.argtypes = [C.POINTER(ImportanceUpdateDesc), vp, i, i, i, i, i, vp, vp, vp]
    lib.dd_exr_reconstruct.argtypes = [vp, vp, i, vp, vp, i, vp, l, vp, vp]
    lib.dd_exr_inflate.argtypes = [vp, vp, i, vp, l, vp, l, vp, vp]
    lib.dd_exr_pack.argtypes = [vp, vp, i, vp, vp, i, vp, l, vp]
    lib.dd_exr_deflate_workspace.argtypes = [i]
    lib.dd_exr_deflate_workspace.restype = l
    lib.dd_exr_deflate.argtypes = [vp, vp, i, vp, l, vp, l, vp, l, vp, vp, vp]
    lib.dd_png_pack.argtypes = [vp, vp, i, vp, vp, i, vp, vp, l, vp]
    lib.dd_png_deflate_workspace.argtypes = [i]
    lib.dd_png_deflate_workspace.restype = l
    lib.dd_png_deflate.argtypes = [vp, vp, i, vp, l, vp, l, vp, l, vp, vp, vp, vp]
    lib.dd_temporal_scratch_bytes.argtypes = [i, i, i]
    lib.dd_temporal_scratch_bytes.restype = l
    lib.dd_temporal_stabilize.argtypes = [C.POINTER(TemporalPass), i, C.POINTER(TemporalGuide), i, i, i, vp, i, f, f, f, f, vp, vp, vp]
    lib.dd_sequence_quality_scratch_bytes.argtypes = [i, i, i]
    lib.dd_sequence_quality_scratch_bytes.restype = l
    lib.dd_sequence_quality.argtypes = [C.POINTER(SequenceQualityPair), i, i, i, vp, i, f, f, vp, f, vp, vp, vp]
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RuntimeError("libdd_hip: %s (status %d)" % (load().dd_last_error().decode(), rc))
