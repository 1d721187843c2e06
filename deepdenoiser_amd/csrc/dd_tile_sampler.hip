// Training tiles cut from frames that stay in device memory (include/dd_hip.h, dd_tile_sampler_desc): ONE launch fills every input and target
// tile buffer of a mini-batch -- crop at the record's origin, then the augmentation of augment_kernel (csrc/dd_pointwise.hip) for the pass's
// kind, in the same pass over the data.
//
// Shape.  grid = (blocks of kBlock x kBlock OUTPUT pixels of a tile, example b, pass).  A pixel is 4 or 12 bytes and a window starts at any
// x0, so nothing is 16-byte aligned: both sides move single floats, lane i at float i of a row segment (256 consecutive bytes per wave
// instruction).  rot90 by 1 or 3 would turn the row reads of such a block into column reads, so the block goes through LDS: the SOURCE
// rectangle the output block maps to (kBlock x kBlock pixels, transposed for an odd rotation) is read along the frame's rows into LDS, and
// every thread then produces one output float, the threads of a wave walking along the tile's rows; the gather that inverts rot90(flip(.))
// happens in LDS.  The row pitch of the LDS block is odd (97 floats), so the column walk of a rotated read touches 64 different banks.
// Plain C++: no inline assembly, no scratch (build.NO_SCRATCH).
#include "dd_common.h"

namespace {

#define S(stream) reinterpret_cast<hipStream_t>(stream)

constexpr int kThreads = 256;
constexpr int kBlock = 32;                    // output pixels per workgroup: kBlock x kBlock
constexpr int kPitch = kBlock * 3 + 1;        // floats per LDS row

// the pixel of the (un-augmented) T x T window that output pixel (y, x) shows: augment_kernel's inversion of rot90(flip(.), k)
__device__ __forceinline__ void source_pixel(int y, int x, int T, int k, bool flip, int& fy, int& fx) {
  fy = y; fx = x;
  if (k == 1) { fy = x; fx = T - 1 - y; }
  else if (k == 2) { fy = T - 1 - y; fx = T - 1 - x; }
  else if (k == 3) { fy = T - 1 - x; fx = y; }
  if (flip) fx = T - 1 - fx;
}

template <int C>
__device__ __forceinline__ void sample_block(const float* __restrict__ win, long row_floats, float* __restrict__ out, int ld_dst, int T, int kind,
                                             const dd_augment_draw& d, int k, bool flip, int use_permute, int use_normal_rotation,
                                             int oy0, int ox0, int bh, int bw, float* __restrict__ lds) {
  // the source rectangle of this output block: its two opposite corners map to opposite corners
  int ay, ax, by, bx;
  source_pixel(oy0, ox0, T, k, flip, ay, ax);
  source_pixel(oy0 + bh - 1, ox0 + bw - 1, T, k, flip, by, bx);
  const int sy0 = min(ay, by), sx0 = min(ax, bx);
  const int sh = (k & 1) ? bw : bh, sw = (k & 1) ? bh : bw;
  const int srow = sw * C;
  for (int i = threadIdx.x; i < sh * srow; i += kThreads) {
    const int ly = i / srow, j = i - ly * srow;
    lds[ly * kPitch + j] = win[(long)(sy0 + ly) * row_floats + (long)sx0 * C + j];
  }
  __syncthreads();
  const int orow = bw * C;
  for (int i = threadIdx.x; i < bh * orow; i += kThreads) {
    const int y = i / orow, j = i - y * orow;
    const int x = j / C, c = j - x * C;
    int fy, fx;
    source_pixel(oy0 + y, ox0 + x, T, k, flip, fy, fx);
    const float* s = lds + (fy - sy0) * kPitch + (fx - sx0) * C;
    float* o = out + ((long)(oy0 + y) * T + ox0 + x) * ld_dst;
    if (C != 3) {
      o[c] = s[c];
      continue;
    }
    float v0 = s[0], v1 = s[1], v2 = s[2];
    if (kind == DD_AUG_SCREEN_NORMAL) {
      if (flip) v0 = -v0;
      if (k == 1) { const float t = v0; v0 = -v1; v1 = t; }
      else if (k == 2) { v0 = -v0; v1 = -v1; }
      else if (k == 3) { const float t = v1; v1 = -v0; v0 = t; }
    } else if (kind == DD_AUG_RGB && use_permute) {
      const float a0 = v0, a1 = v1, a2 = v2;
      switch (d.permute) {
        case 1: v0 = a0; v1 = a2; v2 = a1; break;
        case 2: v0 = a1; v1 = a0; v2 = a2; break;
        case 3: v0 = a1; v1 = a2; v2 = a0; break;
        case 4: v0 = a2; v1 = a0; v2 = a1; break;
        case 5: v0 = a2; v1 = a1; v2 = a0; break;
        default: break;
      }
    } else if (kind == DD_AUG_NORMAL && use_normal_rotation) {
      const float* m = d.normal_rotation;
      const float a0 = v0, a1 = v1, a2 = v2;
      v0 = a0 * m[0] + a1 * m[3] + a2 * m[6];
      v1 = a0 * m[1] + a1 * m[4] + a2 * m[7];
      v2 = a0 * m[2] + a1 * m[5] + a2 * m[8];
    }
    o[c] = c == 0 ? v0 : (c == 1 ? v1 : v2);
  }
}

__global__ __launch_bounds__(kThreads) void tile_sampler_kernel(const dd_tile_sampler_desc desc, const dd_tile_record* __restrict__ records,
                                                                int T, int use_flip, int use_rotate, int use_permute,
                                                                int use_normal_rotation) {
  __shared__ float lds[kBlock * kPitch];
  const dd_tile_pass& p = desc.pass[blockIdx.z];
  const int b = blockIdx.y;
  const dd_tile_record& r = records[b];
  // a record cannot be checked on the host (it lives in device memory): plane and origin are clamped, so no read leaves a plane
  int plane = p.from_target ? r.target_plane : r.source_plane;
  plane = min(max(plane, 0), desc.n_planes - 1);
  const int h = desc.plane_hw[2 * plane], w = desc.plane_hw[2 * plane + 1];
  const float* __restrict__ frame = p.planes[plane];
  if (frame == nullptr || h < T || w < T) return;      // (uniform over the workgroup: before any barrier)
  const int y0 = min(max(r.y0, 0), h - T), x0 = min(max(r.x0, 0), w - T);
  const int nbx = (T + kBlock - 1) / kBlock;
  const int oy0 = (blockIdx.x / nbx) * kBlock, ox0 = (blockIdx.x % nbx) * kBlock;
  const int bh = min(kBlock, T - oy0), bw = min(kBlock, T - ox0);
  const int k = use_rotate ? (r.draw.rotate & 3) : 0;
  const bool flip = use_flip && r.draw.flip > 0;
  const int C = p.C;
  const long row_floats = (long)w * C;
  const float* win = frame + ((long)y0 * w + x0) * C;
  float* out = p.dst + (long)b * T * T * p.ld_dst;
  if (C == 3) sample_block<3>(win, row_floats, out, p.ld_dst, T, p.kind, r.draw, k, flip, use_permute, use_normal_rotation, oy0, ox0, bh, bw, lds);
  else sample_block<1>(win, row_floats, out, p.ld_dst, T, p.kind, r.draw, k, flip, use_permute, use_normal_rotation, oy0, ox0, bh, bw, lds);
}

}  // namespace

extern "C" int dd_sample_tiles(const dd_tile_sampler_desc* desc, const dd_tile_record* records, int B, int T, int use_flip, int use_rotate,
                               int use_permute, int use_normal_rotation, dd_stream stream) {
  DD_REQUIRE(desc && records, "dd_sample_tiles: null descriptor or records");
  DD_REQUIRE(desc->n_passes >= 1 && desc->n_passes <= DD_TILE_MAX_PASSES, "dd_sample_tiles: n_passes=%d (1 .. %d passes fit the descriptor)",
             desc->n_passes, DD_TILE_MAX_PASSES);
  DD_REQUIRE(desc->plane_hw && desc->n_planes >= 1, "dd_sample_tiles: null plane size table or n_planes=%d", desc->n_planes);
  DD_REQUIRE(T >= 1 && T <= 32768, "dd_sample_tiles: T=%d (1 .. 32768)", T);
  DD_REQUIRE(B >= 1 && B <= 65535, "dd_sample_tiles: B=%d (1 .. 65535)", B);
  for (int i = 0; i < desc->n_passes; ++i) {
    const dd_tile_pass& p = desc->pass[i];
    DD_REQUIRE(p.planes && p.dst, "dd_sample_tiles: pass %d has a null pointer", i);
    DD_REQUIRE(p.C == 1 || p.C == 3, "dd_sample_tiles: pass %d has C=%d (1 or 3)", i, p.C);
    DD_REQUIRE(p.ld_dst >= p.C, "dd_sample_tiles: pass %d has ld_dst=%d < C=%d", i, p.ld_dst, p.C);
    DD_REQUIRE(p.kind >= DD_AUG_PLAIN && p.kind <= DD_AUG_SCREEN_NORMAL && (p.kind == DD_AUG_PLAIN || p.C == 3),
               "dd_sample_tiles: pass %d: kind=%d needs 3 channels", i, p.kind);
    DD_REQUIRE(!(p.kind == DD_AUG_NORMAL && use_flip), "dd_sample_tiles: flipping normals is not supported (DataAugmentation.py:22-23)");
  }
  const int nb = (T + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(tile_sampler_kernel, dim3(nb * nb, B, desc->n_passes), dim3(kThreads), 0, S(stream), *desc, records, T, use_flip, use_rotate,
                     use_permute, use_normal_rotation);
  DD_LAUNCH_CHECK();
  return DD_OK;
}
