// svc_fdiv.h — division of an index by a launch-invariant divisor as multiply + shift.  No HIP dependency: the library's kernels
// and the host harness of the tests (tests/native/fdiv_harness.cpp) evaluate the same inline expression, fdiv_q.
//
// A runtime integer division costs ~40 VALU instructions on gfx950, more than the arithmetic of most element-wise kernels here.
//
// make_fdiv(d): l = ceil(log2 d), s = 32 + l, m = ceil(2^s / d).  Then m d = 2^s + e with 0 <= e < d <= 2^l, so
//     n m / 2^s = n / d + n e / (d 2^s).
// n / d lies at least 1 / d below the next integer, so floor(n m / 2^s) = floor(n / d) as long as the excess n e / (d 2^s) stays
// under 1 / d, i.e. n e < 2^s; with e < 2^l that holds for every n < 2^32.  What limits the domain is the 64-bit product:
// m < 2^s / d + 1 <= 2^33 (d > 2^(l-1) for l >= 1; d = 1 gives m = 2^32), so n m < 2^64 is only certain for n < 2^31.
// Exact for every n < 2^31 and every 1 <= d <= 2^31 (the divisors in use reach 960 * 540 = 518 400; nothing here is limited to
// 16 bits).  WRONG for n >= 2^31: the product wraps.  tests/test_fdiv_host.py checks both statements on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVC_FDIV_FN __host__ __device__ __forceinline__
#else
#define SVC_FDIV_FN static inline
#endif

struct FDiv {
    uint64_t m;
    uint32_t d;
    int s;
};
static inline FDiv make_fdiv(uint32_t d) {
    FDiv f;
    f.d = d;
    int l = 0;
    while (((uint64_t)1 << l) < d) ++l;
    f.s = 32 + l;
    f.m = (((uint64_t)1 << f.s) + d - 1) / d;
    return f;
}
// the quotient n / d for n < 2^31
SVC_FDIV_FN uint32_t fdiv_q(uint32_t n, uint64_t m, int s) { return (uint32_t)(((uint64_t)n * m) >> s); }
