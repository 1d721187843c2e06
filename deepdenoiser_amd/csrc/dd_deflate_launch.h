// The launch side of the coder core (dd_deflate_core.h), shared by its two launches: exr_deflate_kernel (dd_exr_deflate.hip, whole zlib streams)
// and png_deflate_kernel (dd_png_encode.hip, segments of one stream).  Both run one wave per record of a table in device memory:
//   sink       WaveOut: where a wave's words and bytes go
//   workspace  every record owns a slice of DD_DEFLATE_BLOCK_TOKENS tokens
//   record     deflate_record_fits: what the kernel asks of a record before it reads or writes anything through it
//   host       deflate_check: the entry point's argument checks under the caller's name; its per-record part states deflate_record_fits
//              condition by condition, each with its message
// The record types (dd_exr_deflate_stream, dd_png_stream) share src_offset, dst_offset, src_bytes and dst_capacity.  Plain C++.
#pragma once
#include "dd_common.h"
#include "dd_deflate_core.h"

constexpr int kLanes = DD_DEFLATE_LANES;
constexpr long kSliceBytes = (long)DD_DEFLATE_BLOCK_TOKENS * 4;

struct WaveOut {
  unsigned char* at0;      // 16-byte aligned
  __device__ __forceinline__ void word(int at, unsigned v) { *reinterpret_cast<unsigned*>(at0 + at) = v; }
  __device__ __forceinline__ void byte(int at, unsigned v) { at0[at] = (unsigned char)v; }
};

inline long deflate_workspace_bytes(int n_streams) { return n_streams > 0 ? (long)n_streams * kSliceBytes : 0l; }

// the source lies in the src_total source bytes; the slot (the capacity up to the next multiple of 16, at a multiple of 16) in the out_bytes
template <typename Stream>
__host__ __device__ __forceinline__ bool deflate_record_fits(const Stream& r, long src_total, long out_bytes) {
  const bool source_fits = r.src_bytes >= 1 && r.src_bytes <= DD_DEFLATE_MAX_BYTES && r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes;
  const bool capacity_fits = r.dst_capacity >= 0 && r.dst_capacity <= DD_DEFLATE_MAX_BYTES;
  const bool place_fits = capacity_fits && r.dst_offset >= 0 && (r.dst_offset & 15) == 0 && r.dst_offset <= out_bytes - (((long)r.dst_capacity + 15) & ~15l);
  return source_fits && place_fits;
}

// The argument checks of dd_exr_deflate / dd_png_deflate under the caller's name `fn` (the messages are pinned by the ABI tests).  The
// result arrays differ: the caller passes whether it has them all (`arrays`) and how the message calls them.  more(k, record) -> DD_OK or
// an error it has set: what the caller asks of a record beyond the common fields, placed where its message has always stood.  DD_OK with
// n_streams == 0 means there is nothing to launch.
template <typename Stream, typename More>
inline int deflate_check(const char* fn, const Stream* streams_host, const Stream* streams, int n_streams, const void* src, long src_total, const void* out,
                         long out_bytes, const void* workspace, long workspace_bytes, bool arrays, const char* arrays_named, More more) {
  DD_REQUIRE(n_streams >= 0, "%s: n_streams=%d", fn, n_streams);
  if (n_streams == 0) return DD_OK;
  DD_REQUIRE(streams_host && streams, "%s: null stream table", fn);
  DD_REQUIRE(src && out && workspace && arrays, "%s: null source, output, workspace, %s", fn, arrays_named);
  DD_REQUIRE((reinterpret_cast<unsigned long long>(out) & 15ull) == 0ull && (reinterpret_cast<unsigned long long>(workspace) & 3ull) == 0ull,
             "%s: the output is not 16-byte aligned or the workspace not 4-byte aligned", fn);
  DD_REQUIRE(workspace_bytes >= deflate_workspace_bytes(n_streams), "%s: workspace_bytes=%ld, %d streams need %ld", fn, workspace_bytes, n_streams,
             deflate_workspace_bytes(n_streams));
  {
    const char* s0 = static_cast<const char*>(src);
    const char* d0 = static_cast<const char*>(out);
    DD_REQUIRE(src_total < 0 || out_bytes < 0 || s0 + src_total <= d0 || d0 + out_bytes <= s0, "%s: the source (%ld bytes) and the output (%ld bytes) overlap", fn,
               src_total, out_bytes);
  }
  for (int k = 0; k < n_streams; ++k) {
    const Stream& r = streams_host[k];
    DD_REQUIRE(r.src_bytes >= 1 && r.src_bytes <= DD_DEFLATE_MAX_BYTES, "%s: stream %d: src_bytes=%d (1 .. %d)", fn, k, r.src_bytes, DD_DEFLATE_MAX_BYTES);
    DD_REQUIRE(r.dst_capacity >= 0 && r.dst_capacity <= DD_DEFLATE_MAX_BYTES, "%s: stream %d: dst_capacity=%d", fn, k, r.dst_capacity);
    if (const int rc = more(k, r); rc != DD_OK) return rc;
    DD_REQUIRE(r.src_offset >= 0 && r.src_offset <= src_total - r.src_bytes, "%s: stream %d: src_offset=%lld (%d bytes) leaves the %ld source bytes", fn, k,
               r.src_offset, r.src_bytes, src_total);
    DD_REQUIRE(r.dst_offset >= 0 && (r.dst_offset & 15) == 0, "%s: stream %d: dst_offset=%lld is negative or not 16-byte aligned", fn, k, r.dst_offset);
    DD_REQUIRE(r.dst_offset <= out_bytes - (((long)r.dst_capacity + 15) & ~15l), "%s: stream %d: dst_offset=%lld (capacity %d) leaves the %ld output bytes", fn, k,
               r.dst_offset, r.dst_capacity, out_bytes);
  }
  return DD_OK;
}
