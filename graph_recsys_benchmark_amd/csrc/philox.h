// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the Random123 constants), the counter-based stream of every device-side
// sampler (sampler.hip, walk.hip).  oracle/philox.py restates it in numpy and pins the published known-answer vectors.
#pragma once
#include <hip/hip_runtime.h>

namespace pea {

struct U4 {
    unsigned x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
        c = U4{(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

}  // namespace pea
