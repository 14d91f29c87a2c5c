// CPU harness for retargetvid_amd/csrc/svc_fdiv.h (division by a launch-invariant divisor as multiply + shift, as the kernels
// evaluate it: the same inline expression fdiv_q).  Built by tests/ only (g++), never loaded by the product.
#include <stdint.h>

#include "../../retargetvid_amd/csrc/svc_fdiv.h"

extern "C" uint32_t fdiv_one(uint32_t d, uint32_t n) {
    const FDiv f = make_fdiv(d);
    return fdiv_q(n, f.m, f.s);
}

extern "C" void fdiv_constants(uint32_t d, uint64_t *m, int *s) {
    const FDiv f = make_fdiv(d);
    *m = f.m;
    *s = f.s;
}

static inline uint64_t next_random(uint64_t &x) {      // xorshift64
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
}

// For every divisor: m < 2^33, and the quotient equals n / d at n = k d - 1, k d and k d + d - 1 (where 0 <= n < limit) for k over
// the first `span` multiples, the last `span` multiples below `limit` and `span` random ones.  -> the number of failures;
// bad[0..2] = (d, n, quotient) of the first (d, 0, 0 where m is too large), checked = the dividends tried.
extern "C" uint64_t fdiv_sweep(const uint32_t *divisors, int count, uint32_t span, uint64_t limit, uint64_t seed, uint64_t *bad,
                               uint64_t *checked) {
    uint64_t failures = 0, tried = 0, rnd = seed | 1;
    auto fail = [&](uint64_t d, uint64_t n, uint64_t q) {
        if (!failures++) { bad[0] = d; bad[1] = n; bad[2] = q; }
    };
    for (int i = 0; i < count; ++i) {
        const uint32_t d = divisors[i];
        const FDiv f = make_fdiv(d);
        if (f.m >= ((uint64_t)1 << 33) || f.d != d) fail(d, 0, 0);
        const uint64_t kmax = (limit - 1) / d;                      // the last multiple below the limit
        auto at = [&](uint64_t k) {
            const uint64_t base = k * d;
            const uint64_t ns[3] = {base - 1, base, base + d - 1};
            for (int j = 0; j < 3; ++j) {
                if ((j == 0 && k == 0) || ns[j] >= limit) continue;
                const uint32_t n = (uint32_t)ns[j];
                const uint32_t q = fdiv_q(n, f.m, f.s);
                ++tried;
                if (q != n / d) fail(d, n, q);
            }
        };
        for (uint64_t k = 0; k < span && k <= kmax; ++k) at(k);
        for (uint64_t k = kmax >= span ? kmax - span + 1 : 0; k <= kmax; ++k) at(k);
        for (uint32_t r = 0; r < span; ++r) at(next_random(rnd) % (kmax + 1));
    }
    *checked = tried;
    return failures;
}
