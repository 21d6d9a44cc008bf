// arl_util.h -- the small items every kernel file of the library needs: the launch check, the workspace rounding, the width ladder and the
// counter hash of the in-kernel random draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// after a kernel launch inside a function that returns an arl status / hipError_t as int
#define ARL_LAUNCH_CHECK()                                  \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return (int)e__;             \
    } while (0)

// the embedding widths the templated kernels are built for; RUN(DD) must return
#define ARL_DISPATCH_WIDTH(d, RUN) \
    do {                           \
        if ((d) == 16) RUN(16);    \
        if ((d) == 32) RUN(32);    \
        if ((d) == 64) RUN(64);    \
        RUN(128);                  \
    } while (0)

namespace {

inline bool arl_width_ok(int64_t d) { return d == 16 || d == 32 || d == 64 || d == 128; }

// workspace sections start on 16-byte boundaries
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// the splitmix64 finaliser: the counter hash behind every draw made inside a kernel, and (on the host) behind the key of a call
__host__ __device__ __forceinline__ uint64_t arl_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

}  // namespace
