// The PNG row coder (deepdenoiser_amd/csrc/dd_png_core.h) and the segment framing of the deflate coder core (csrc/dd_deflate_core.h) on the CPU: a
// stand-alone program for tests/test_png_core.py, built with -fsanitize=address,undefined and not loaded into Python.  The lanes are loops (256
// workers for a row, as the pack kernel's workgroup; 64 for the coder).  Every buffer is a heap object of exactly its size -- a row buffer
// of W * n bytes, a segment's source of n bytes, its body of dst_capacity = n - 1 bytes (what the host passes to dd_png_deflate), the token
// workspace of the size the core asks for -- so a read or write outside any of them is reported.
//   usage: png_core_main corpus.bin result.bin
//   corpus: 255 floats (the threshold table), uint32 count, then per job uint32 kind and
//     kind 0, an image: int32 H, W, C, n, src_channel[3], float exposure, uint32 segment_rows, H * W * C floats
//     kind 1, bytes   : uint32 n, uint32 segments, `segments` uint32 lengths, n bytes
//   result: per job uint32 filtered bytes and the filtered rows (0 for kind 1), uint32 segments, then per segment int32 status, int32 size,
//     uint32 adler and `size` bytes (the body when the status is OK)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../deepdenoiser_amd/csrc/dd_deflate_core.h"
#include "../deepdenoiser_amd/csrc/dd_png_core.h"

namespace {

constexpr int kWorkers = 256;

struct HeapOut {
  unsigned char* at0;
  void word(int at, unsigned v) { std::memcpy(at0 + at, &v, 4); }      // (little-endian hosts)
  void byte(int at, unsigned v) { at0[at] = (unsigned char)v; }
};

bool read_exact(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// the filtered rows of an image, as png_pack_kernel builds them: row by row, the row above kept
std::vector<unsigned char> filter_image(const float* thr, const float* plane, int H, int W, int C, int n, const int* channel, float exposure) {
  const int nbytes = W * n;
  std::vector<unsigned char> out;
  std::unique_ptr<unsigned char[]> rows[2] = {std::unique_ptr<unsigned char[]>(new unsigned char[nbytes]), std::unique_ptr<unsigned char[]>(new unsigned char[nbytes])};
  std::unique_ptr<unsigned char[]> dst(new unsigned char[1 + nbytes]);
  for (int y = 0; y < H; ++y) {
    unsigned char* cur = rows[(y + 1) & 1].get();
    const unsigned char* up = y > 0 ? rows[y & 1].get() : nullptr;
    for (int lane = 0; lane < kWorkers; ++lane) dd_png_quantise_row(thr, plane + (long)y * W * C, W, C, n, channel, exposure, lane, kWorkers, cur);
    unsigned cost[DD_PNG_FILTERS] = {0u, 0u, 0u, 0u, 0u};
    for (int lane = kWorkers - 1; lane >= 0; --lane) dd_png_row_costs(cur, up, nbytes, n, lane, kWorkers, cost);      // (any order: integers)
    const int type = dd_png_pick(cost);
    for (int lane = 0; lane < kWorkers; ++lane) dd_png_write_row(type, cur, up, nbytes, n, lane, kWorkers, dst.get());
    out.insert(out.end(), dst.get(), dst.get() + 1 + nbytes);
  }
  return out;
}

// one segment through the coder -> its record in the result file
bool code_segment(std::FILE* res, dd_deflate_state* state, const unsigned char* data, int n, bool last, unsigned fill) {
  std::unique_ptr<unsigned char[]> src(new unsigned char[n]);
  std::memcpy(src.get(), data, n);
  const int capacity = n - 1;
  std::unique_ptr<unsigned char[]> dst(new unsigned char[capacity]);
  std::memset(dst.get(), 0xA5, capacity);
  std::unique_ptr<unsigned[]> tokens(new unsigned[DD_DEFLATE_BLOCK_TOKENS]);
  std::memset(static_cast<void*>(state), 0xA5 ^ (int)(fill & 0xff), sizeof(dd_deflate_state));      // (LDS is not cleared between workgroups either)
  std::memset(tokens.get(), 0xA5, sizeof(unsigned) * DD_DEFLATE_BLOCK_TOKENS);
  HeapOut out{dst.get()};
  int32_t size = 0;
  uint32_t adler = 0;
  const int32_t status = dd_deflate_segment(src.get(), n, capacity, last, tokens.get(), state, out, &size, &adler);
  if (status == DD_DEFLATE_OK && (size < 1 || size > capacity)) return false;
  if (status != DD_DEFLATE_OK) size = 0;
  std::fwrite(&status, 4, 1, res);
  std::fwrite(&size, 4, 1, res);
  std::fwrite(&adler, 4, 1, res);
  if (size) std::fwrite(dst.get(), 1, size, res);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* res = std::fopen(argv[2], "wb");
  if (!in || !res) return 2;
  std::unique_ptr<float[]> thr(new float[DD_PNG_THRESHOLDS]);
  uint32_t count = 0;
  if (!read_exact(in, thr.get(), sizeof(float) * DD_PNG_THRESHOLDS) || !read_exact(in, &count, 4)) return 2;
  std::unique_ptr<dd_deflate_state> state(new dd_deflate_state);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t kind = 0;
    if (!read_exact(in, &kind, 4) || kind > 1) return 2;
    std::vector<unsigned char> data;
    std::vector<uint32_t> lengths;
    if (kind == 0) {
      int32_t head[7];
      float exposure = 0.f;
      uint32_t segment_rows = 0;
      if (!read_exact(in, head, sizeof(head)) || !read_exact(in, &exposure, 4) || !read_exact(in, &segment_rows, 4)) return 2;
      const int H = head[0], W = head[1], C = head[2], n = head[3];
      if (H < 1 || W < 1 || C < 1 || (n != 1 && n != 3) || segment_rows < 1 || (long)H * W * C > (1l << 26)) return 2;
      for (int c = 0; c < n; ++c)
        if (head[4 + c] < 0 || head[4 + c] >= C) return 2;
      std::unique_ptr<float[]> plane(new float[(size_t)H * W * C]);
      if (!read_exact(in, plane.get(), sizeof(float) * (size_t)H * W * C)) return 2;
      const int channel[3] = {head[4], head[n == 3 ? 5 : 4], head[n == 3 ? 6 : 4]};
      data = filter_image(thr.get(), plane.get(), H, W, C, n, channel, exposure);
      for (int y0 = 0; y0 < H; y0 += (int)segment_rows) lengths.push_back((uint32_t)((H - y0 < (int)segment_rows ? H - y0 : (int)segment_rows) * (1 + W * n)));
      const uint32_t total = (uint32_t)data.size();
      std::fwrite(&total, 4, 1, res);
      std::fwrite(data.data(), 1, data.size(), res);
    } else {
      uint32_t n = 0, segments = 0;
      if (!read_exact(in, &n, 4) || !read_exact(in, &segments, 4) || n < 1 || n > (uint32_t)DD_DEFLATE_MAX_BYTES || segments < 1 || segments > n) return 2;
      lengths.resize(segments);
      if (!read_exact(in, lengths.data(), 4 * (size_t)segments)) return 2;
      data.resize(n);
      if (!read_exact(in, data.data(), n)) return 2;
      const uint32_t zero = 0;
      std::fwrite(&zero, 4, 1, res);
    }
    const uint32_t segments = (uint32_t)lengths.size();
    std::fwrite(&segments, 4, 1, res);
    size_t at = 0;
    for (uint32_t s = 0; s < segments; ++s) {
      if (lengths[s] < 1 || at + lengths[s] > data.size()) return 2;
      if (!code_segment(res, state.get(), data.data() + at, (int)lengths[s], s + 1 == segments, k + s)) return 3;
      at += lengths[s];
    }
    if (at != data.size()) return 2;
  }
  std::fclose(in);
  return std::fclose(res) == 0 ? 0 : 2;
}
