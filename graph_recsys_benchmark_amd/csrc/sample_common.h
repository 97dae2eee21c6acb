// What the three device-side samplers share (sampler.hip, kg_sampler.hip, cf_sampler.hip): the search of a sorted key table, the
// tags that keep their Philox streams apart, and the keyed bijection of the epoch shuffle (include/peahip_sample.h states it).
// The third counter word carries the tag from bit 8 up, the attempt below it:
//   0        the negative item of a CF row (sampler.hip, cf_sampler.hip)
//   1 << 8   the negative tail of a KG triple (kg_sampler.hip)
//   2 << 8   the round function of the shuffle
//   3 << 8   the entity columns of a CF row (cf_sampler.hip)
#pragma once
#include "philox.h"

namespace pea {

constexpr int kMaxAttempts = 64;  // a user who has seen almost every item: the last draw is kept and flagged
constexpr unsigned kTagDraw = 1u << 8, kTagShuffle = 2u << 8, kTagEntity = 3u << 8;

struct Stream {
    unsigned k0, k1, offset;
};

// whether `key` is in keys[0 .. n) (ascending): the first index with keys[idx] >= key, compared
__device__ __forceinline__ bool contains(const long long *__restrict__ keys, long long n, long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && keys[lo] == key;
}

__device__ __forceinline__ unsigned round_fn(unsigned r, unsigned j, const Stream &st) {
    return philox4x32_10(U4{r, j, kTagShuffle, st.offset}, st.k0, st.k1).x;
}

// perm(x) for x < n: the pass (L, R) -> (R, L ^ F_j(R)), j = 0..3, repeated while the result is >= n
__device__ __forceinline__ unsigned long long perm_of(unsigned long long x, unsigned long long n, int hb, const Stream &st) {
    const unsigned long long m = (1ull << hb) - 1;
    do {
        unsigned long long L = x >> hb, R = x & m;
#pragma unroll 1
        for (unsigned j = 0; j < 4; ++j) {
            const unsigned long long t = L ^ ((unsigned long long)round_fn((unsigned)R, j, st) & m);
            L = R;
            R = t;
        }
        x = (L << hb) | R;
    } while (x >= n);
    return x;
}

// hb of the header: half the bit length of n - 1, rounded up, at least 1
inline int half_bits(long long n) {
    int b = 0;
    for (unsigned long long v = (unsigned long long)(n - 1); v; v >>= 1) ++b;
    if (b < 1) b = 1;
    return (b + 1) / 2;
}

}  // namespace pea
