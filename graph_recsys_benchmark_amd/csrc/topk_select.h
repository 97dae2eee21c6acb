// Selection pieces shared by the full-catalogue kernels of topk.hip (MLP scorer) and dot_score.hip (inner-product
// scorer): how the catalogue is cut into item ranges and what both check about it, the sentinel of an empty list entry,
// the search in a user's ascending exclusion list, the per-lane K-entry list, the bitonic merge that orders a user's
// partial K-entry columns by (score descending, catalogue index ascending), and the finish of the all-item rank.
#ifndef PEA_TOPK_SELECT_H_
#define PEA_TOPK_SELECT_H_

#include <algorithm>

#include "common.h"

namespace pea {
namespace {

constexpr int kMaxMerge = 2048;     // partial entries of one user (columns * K) the merge kernel folds
constexpr int kEmpty = 0x7fffffff;  // item slot of a list entry that holds nothing
constexpr int kMaxSplits = 64;      // item ranges of one call

// The catalogue in S item ranges of `span` items (a multiple of the kernel's item tile), so that few users still fill the
// machine: ~4 workgroups per CU over `user_blocks` blocks of users, a range worth >= 512 items, and no more partial
// entries per user (`entries` per range) than the merge folds.
inline void catalogue_split(int64_t user_blocks, int64_t n_items, int entries, int tile_items, int *S, int64_t *span) {
    int64_t s = (1024 + user_blocks - 1) / user_blocks;
    s = std::min<int64_t>(s, std::max<int64_t>(n_items / 512, 1));
    s = std::min<int64_t>(s, std::min<int64_t>(kMaxSplits, kMaxMerge / entries));
    s = std::max<int64_t>(s, 1);
    int64_t sp = (std::max<int64_t>(n_items, 1) + s - 1) / s;
    sp = (sp + tile_items - 1) / tile_items * tile_items;
    *span = sp;
    *S = (int)std::max<int64_t>((n_items + sp - 1) / sp, 1);
}

// what every full-catalogue entry point checks besides its scorer's width
inline int check_catalogue(const char *what, int64_t U, int64_t num_nodes, int64_t item_lo, int64_t n_items) {
    PEA_REQUIRE(U >= 0 && num_nodes > 0 && n_items >= 0 && n_items < ((int64_t)1 << 31) - 1, PEA_ERR_ARG,
                "%s: U=%lld n_items=%lld", what, (long long)U, (long long)n_items);
    PEA_REQUIRE(item_lo >= 0 && item_lo + n_items <= num_nodes, PEA_ERR_RANGE,
                "%s: catalogue [%lld, %lld) outside [0, num_nodes = %lld)", what, (long long)item_lo,
                (long long)(item_lo + n_items), (long long)num_nodes);
    return PEA_OK;
}

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

// A lane's K best (score, catalogue index) so far: an unordered column of LDS, entry j at cs / ci[j * stride + lane].  The lane
// keeps the slot and score of the worst entry (lowest score, highest index among equals); its items arrive in ascending
// index, so only a strictly higher score displaces the worst.
// (topk_scan_kernel writes list_init's loop out: topk.hip says why.)
__device__ __forceinline__ void list_init(float *cs, int *ci, int stride, int lane, int K) {
    for (int j = 0; j < K; ++j) {
        cs[j * stride + lane] = -INFINITY;
        ci[j * stride + lane] = kEmpty;
    }
}

// (s, idx) replaces the worst entry (the caller saw s > thr), then the column is rescanned for the new worst
__device__ __forceinline__ void list_insert(float *cs, int *ci, int stride, int lane, int K, float s, int idx, int &wslot,
                                            float &thr) {
    cs[wslot * stride + lane] = s;
    ci[wslot * stride + lane] = idx;
    float w = cs[lane];
    int wi = ci[lane];
    wslot = 0;
    for (int m = 1; m < K; ++m) {
        const float sc = cs[m * stride + lane];
        const int id = ci[m * stride + lane];
        if (sc < w || (sc == w && id > wi)) {
            w = sc;
            wi = id;
            wslot = m;
        }
    }
    thr = w;
}

// the column goes to the workspace as partial column `col` of user q ([cols, K, U] scores and indices) for the merge
__device__ __forceinline__ void list_store(const float *cs, const int *ci, int stride, int lane, int K, int64_t col, int64_t U,
                                           int64_t q, float *part_s, int *part_i) {
    for (int j = 0; j < K; ++j) {
        const int64_t o = (col * K + j) * U + q;
        part_s[o] = cs[j * stride + lane];
        part_i[o] = ci[j * stride + lane];
    }
}

// The all-item rank of user q once the scans have counted (s > pos) and (s < pos) over EVERY catalogue item, per partial
// column ([cols, 2, U] in `part`): sums the columns, then walks the user's exclusion list once and takes out what those
// items contributed.  score(node) must give the bits the scan compared.  The scan counted the positive's own catalogue
// row too: it compares equal to itself, so it is in neither counter.
template <class Scorer>
__device__ __forceinline__ void rank_finish(int64_t q, int64_t U, int cols, int64_t n_items, int64_t item_lo, float pos, int64_t pn,
                                            const int64_t *__restrict__ excl_rowptr, const int64_t *__restrict__ excl_items,
                                            const int *__restrict__ part, const Scorer &score, int32_t *rank, float *auc,
                                            float *pos_score) {
    int64_t hi = 0, lo = 0;
    for (int c = 0; c < cols; ++c) {
        hi += part[((int64_t)c * 2) * U + q];
        lo += part[((int64_t)c * 2 + 1) * U + q];
    }
    int64_t others = n_items - ((pn >= item_lo && pn < item_lo + n_items) ? 1 : 0);
    if (excl_rowptr) {
        for (int64_t e = excl_rowptr[q]; e < excl_rowptr[q + 1]; ++e) {
            const int64_t node = excl_items[e];
            if (node < item_lo || node >= item_lo + n_items || node == pn) continue;
            const float s = score(node);
            hi -= s > pos ? 1 : 0;
            lo -= s < pos ? 1 : 0;
            --others;
        }
    }
    if (rank) rank[q] = (int32_t)hi;
    if (auc) auc[q] = others > 0 ? (float)lo / (float)others : 0.f;
    if (pos_score) pos_score[q] = pos;
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
