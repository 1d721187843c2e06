// Host stand-in for csrc/dd_common.h, for tests/test_preview_host.py only: csrc/dd_preview.hip and csrc/dd_loss_common.h compile against it as
// plain C++, and a "launch" runs the kernel's threads one after another on the CPU.  What it checks is the kernel's arithmetic, indexing and
// argument checks against tests/preview_ref.py on a machine without a GPU; what it cannot check is anything the hardware decides.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include "dd_hip.h"
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static dim3 threadIdx, blockIdx;
inline void __syncthreads() {}
using std::max;
using std::min;
typedef void* hipStream_t;
static char host_error[512];
inline void dd_set_error(const char* fmt, ...) {
  va_list a;
  va_start(a, fmt);
  vsnprintf(host_error, sizeof host_error, fmt, a);
  va_end(a);
}
extern "C" const char* dd_last_error() { return host_error; }
#define DD_REQUIRE(cond, ...)     \
  do {                            \
    if (!(cond)) {                \
      dd_set_error(__VA_ARGS__);  \
      return DD_ERR_INVALID;      \
    }                             \
  } while (0)
#define DD_LAUNCH_CHECK() \
  do {                    \
  } while (0)
// Every workgroup runs twice: a barrier separates the threads that fill the (static) shared table from the threads that read it, and here
// the threads run in turn, so the first pass fills the table and the second pass is the one whose stores count (they overwrite the first's).
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)   \
  do {                                                              \
    const dim3 g_ = grid, b_ = block;                               \
    for (unsigned bx_ = 0; bx_ < g_.x; ++bx_)                       \
      for (int pass_ = 0; pass_ < 2; ++pass_)                       \
        for (unsigned tx_ = 0; tx_ < b_.x; ++tx_) {                 \
          blockIdx.x = bx_;                                         \
          threadIdx.x = tx_;                                        \
          kernel(__VA_ARGS__);                                      \
        }                                                           \
  } while (0)
