// The deflate coder core (deepdenoiser_amd/csrc/dd_deflate_core.h) on the CPU: a stand-alone program for tests/test_exr_deflate_core.py, built
// with -fsanitize=address,undefined.  Every stream is written into a heap buffer of exactly dst_capacity = n - 1 bytes (what the host passes to
// dd_exr_deflate), the token workspace has exactly the size the core asks for, and the state is a heap object of its own, so a write outside
// any of them is reported.
//   usage: exr_deflate_core_main corpus.bin result.bin
//   corpus: uint32 count, then per input uint32 n and n bytes;  result: per input int32 status, int32 size, then `size` bytes when status is OK
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../deepdenoiser_amd/csrc/dd_deflate_core.h"

namespace {

struct HeapOut {
  unsigned char* at0;
  void word(int at, unsigned v) { std::memcpy(at0 + at, &v, 4); }      // (little-endian hosts)
  void byte(int at, unsigned v) { at0[at] = (unsigned char)v; }
};

bool read_exact(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* res = std::fopen(argv[2], "wb");
  if (!in || !res) return 2;
  uint32_t count = 0;
  if (!read_exact(in, &count, 4)) return 2;
  std::unique_ptr<dd_deflate_state> state(new dd_deflate_state);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0;
    if (!read_exact(in, &n, 4) || n < 1 || n > (uint32_t)DD_DEFLATE_MAX_BYTES) return 2;
    std::unique_ptr<unsigned char[]> src(new unsigned char[n]);
    if (!read_exact(in, src.get(), n)) return 2;
    const int capacity = (int)n - 1;
    std::unique_ptr<unsigned char[]> dst(new unsigned char[capacity]);
    std::memset(dst.get(), 0xA5, capacity);
    std::unique_ptr<unsigned[]> tokens(new unsigned[DD_DEFLATE_BLOCK_TOKENS]);
    std::memset(static_cast<void*>(state.get()), 0xA5 ^ (int)(k & 0xff), sizeof(dd_deflate_state));      // (LDS is not cleared between workgroups either)
    std::memset(tokens.get(), 0xA5, sizeof(unsigned) * DD_DEFLATE_BLOCK_TOKENS);
    HeapOut out{dst.get()};
    int32_t size = 0;
    const int32_t status = dd_deflate_stream(src.get(), (int)n, capacity, tokens.get(), state.get(), out, &size);
    if (status == DD_DEFLATE_OK && (size < 1 || size > capacity)) return 3;
    if (status != DD_DEFLATE_OK) size = 0;
    std::fwrite(&status, 4, 1, res);
    std::fwrite(&size, 4, 1, res);
    if (size) std::fwrite(dst.get(), 1, size, res);
  }
  std::fclose(in);
  return std::fclose(res) == 0 ? 0 : 2;
}
