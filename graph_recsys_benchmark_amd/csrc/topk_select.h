// Selection pieces shared by the full-catalogue kernels of topk.hip (MLP scorer) and dot_score.hip (inner-product
// scorer): the sentinel of an empty list entry, the search in a user's ascending exclusion list, and the bitonic merge
// that orders a user's partial K-entry columns by (score descending, catalogue index ascending).
#ifndef PEA_TOPK_SELECT_H_
#define PEA_TOPK_SELECT_H_

#include "common.h"

namespace pea {
namespace {

constexpr int kMaxMerge = 2048;     // partial entries of one user (columns * K) the merge kernel folds
constexpr int kEmpty = 0x7fffffff;  // item slot of a list entry that holds nothing

// is `node` in the strictly ascending list ex[lo, hi)?
__device__ __forceinline__ bool in_sorted(const int64_t *__restrict__ ex, int64_t lo, int64_t hi, int64_t node) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t v = ex[mid];
        if (v == node) return true;
        if (v < node) lo = mid + 1; else hi = mid;
    }
    return false;
}

// One workgroup per user: the S unordered K-entry columns (padded with empty entries to a power of two) are put in
// (score descending, index ascending) order by a bitonic network in LDS and the first K written.  Catalogue indices are
// unique, so the order is total over the real entries; empty entries (-inf, kEmpty) compare equal to each other only and
// end up last, where they become the (-1, -inf) tail of a user with fewer than K eligible items.
__global__ __launch_bounds__(256) void topk_merge_kernel(int64_t U, int K, int S, int P2, int64_t item_lo,
                                                         const float *__restrict__ part_s, const int *__restrict__ part_i,
                                                         int64_t *__restrict__ out_items, float *__restrict__ out_scores) {
    __shared__ float cs[kMaxMerge];
    __shared__ int ci[kMaxMerge];
    const int64_t q = blockIdx.x;
    const int M = S * K;
    for (int m = threadIdx.x; m < P2; m += blockDim.x) {
        cs[m] = m < M ? part_s[(int64_t)m * U + q] : -INFINITY;
        ci[m] = m < M ? part_i[(int64_t)m * U + q] : kEmpty;
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P2; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const float si = cs[i], sl = cs[l];
                    const int ii = ci[i], il = ci[l];
                    const bool l_first = sl > si || (sl == si && il < ii);   // entry l belongs ahead of entry i
                    const bool i_first = si > sl || (si == sl && ii < il);
                    if ((i & k) == 0 ? l_first : i_first) {
                        cs[i] = sl; ci[i] = il;
                        cs[l] = si; ci[l] = ii;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        const bool real = j < P2 && ci[j] != kEmpty;
        out_items[q * K + j] = real ? item_lo + ci[j] : -1;
        out_scores[q * K + j] = real ? cs[j] : -INFINITY;
    }
}

}  // namespace
}  // namespace pea
#endif  // PEA_TOPK_SELECT_H_
