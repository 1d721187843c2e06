// The inflate decoder core (deepdenoiser_amd/csrc/dd_inflate_core.h) on the CPU: a stand-alone program that tests/test_exr_inflate_core.py
// compiles with -fsanitize=address,undefined and runs over a corpus of streams, before the same core runs on a GPU.
//   exr_inflate_core_main CORPUS RESULT
// CORPUS: int32 count, then per stream int32 src_bytes, int32 dst_bytes and the stream.  RESULT: per stream int32 status and dst_bytes output
// bytes.  Every stream is copied into a heap block of exactly src_bytes and decoded into one of exactly dst_bytes (0xA5-filled), so a read
// or a write one byte outside either is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../deepdenoiser_amd/csrc/dd_inflate_core.h"

namespace {

struct PlainSink {
  unsigned char* out;
  void literal(int at, unsigned value) { out[at] = (unsigned char)value; }
  void stored(int at, const unsigned char* from, int n) { std::memcpy(out + at, from, (size_t)n); }
  void match(int at, int distance, int length) {
    for (int i = 0; i < length; ++i) out[at + i] = out[at - distance + i % distance];
  }
  unsigned adler(int n) {
    unsigned a = 1u, b = 0u;
    for (int i = 0; i < n; ++i) {
      a = (a + out[i]) % 65521u;
      b = (b + a) % 65521u;
    }
    return (b << 16) | a;
  }
};

bool read_int(FILE* f, int32_t* v) { return std::fread(v, 4, 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s CORPUS RESULT\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  int32_t count = 0;
  if (!in || !out || !read_int(in, &count) || count < 0) return 2;
  dd_inflate_tables* tables = new dd_inflate_tables;
  for (int32_t k = 0; k < count; ++k) {
    int32_t src_bytes = 0, dst_bytes = 0;
    if (!read_int(in, &src_bytes) || !read_int(in, &dst_bytes) || src_bytes < 0 || dst_bytes < 0) return 2;
    unsigned char* src = static_cast<unsigned char*>(std::malloc((size_t)src_bytes ? (size_t)src_bytes : 1));
    unsigned char* dst = static_cast<unsigned char*>(std::malloc((size_t)dst_bytes ? (size_t)dst_bytes : 1));
    if (src_bytes && std::fread(src, 1, (size_t)src_bytes, in) != (size_t)src_bytes) return 2;
    std::memset(dst, 0xA5, (size_t)dst_bytes);
    std::memset(tables, 0xEE, sizeof(*tables));      // (no table entry of an earlier stream is relied on)
    PlainSink sink{dst};
    const int32_t status = dd_inflate_stream(src, src_bytes, dst_bytes, tables, sink);
    std::fwrite(&status, 4, 1, out);
    std::fwrite(dst, 1, (size_t)dst_bytes, out);
    std::free(src);
    std::free(dst);
  }
  delete tables;
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 2;
}
