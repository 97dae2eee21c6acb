// Selection pieces shared by the full-catalogue kernels of topk.hip (MLP scorer) and dot_score.hip (inner-product
// scorer): how the catalogue is cut into item ranges and what both check about it, the sentinel of an empty list entry,
// the search in a user's ascending exclusion list, the per-lane K-entry list, the bitonic merge that orders a user's
// partial K-entry columns by (score descending, catalogue index ascending), the thread-per-user finish of the all-item
// rank, and the rows, counters and wave-per-user finish of the all-item rank with several positives per user (of which
// the inner product's single-positive rank is the case of one positive per user).
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

// ---------------------------------------------------------------------------------------------- the all-item rank
// The rank with any number of positives per user (include/peahip_eval.h): user q holds the positives
// pos_items[pos_rowptr[q], pos_rowptr[q + 1]), cut into chunks of kPC thresholds.  One (user, chunk) ROW rides in a scan
// where one user rides in a top-K scan, and every catalogue score is compared against the row's thresholds (a compare
// chain over registers).  pea_dot_rank_full is this body with a null pos_rowptr: user q owns flat positive q, so Q = U, a
// row is a user and holds one threshold (and, over very many users, the positives' scores and the finish go by a thread
// per user: pos_team, rank_finish).  pea_rank_full keeps a scan of its own (topk.hip says why).
constexpr int kPC = 8;

// Rows of a call, a bound that needs no look at the data: row q < U is chunk 0 of user q; chunk c >= 1 of a user whose
// positives start at flat index b begins at f = b + c kPC and sits in row U + f / kPC - 1.  Two such chunks start at least
// kPC apart (inside one user by construction, across users because a chunk c >= 1 starts kPC past its user's first entry),
// so no two share a row, and f <= Q - 1 keeps the row below U + Q / kPC.  Rows nobody owns stay idle.  Without a row
// pointer there are no chunks past the first: the rows are the U users.
inline int64_t multi_rows(int64_t U, int64_t Q, bool row_pointer) { return row_pointer ? U + Q / kPC : U; }

// thresholds a row can hold, which is the chunk stride of the partial counters [cols, 2, stride, rows]
inline int multi_chunk(bool row_pointer) { return row_pointer ? kPC : 1; }

// user q's positives [b, e) within [0, Q): clamped, so that a row pointer that breaks its precondition reads nothing out
// of bounds; the q-th alone for a call without a row pointer
__device__ __forceinline__ void pos_span(const int64_t *__restrict__ pos_rowptr, int64_t q, int64_t Q, int64_t &b, int64_t &e) {
    if (!pos_rowptr) {
        b = q;
        e = q + 1;
        return;
    }
    b = pos_rowptr[q];
    e = pos_rowptr[q + 1];
    b = b < 0 ? 0 : (b > Q ? Q : b);
    e = e < b ? b : (e > Q ? Q : e);
}

// the row of threshold j of a user whose positives start at flat index b
__device__ __forceinline__ int64_t multi_row_of(int64_t q, int64_t U, int64_t b, int64_t j) {
    const int64_t c = j / kPC;
    return c == 0 ? q : U + (b + c * kPC) / kPC - 1;
}

// Who rides in row r: user q and the n (1..kPC) thresholds from flat index `first`; n = 0 for an idle row.  A row past U
// (a call with a row pointer only: multi_rows) finds its owner by a search in pos_rowptr: the owner of flat index
// (r - U + 1) kPC is the only user that can have a chunk start in [that, + kPC).
__device__ __forceinline__ void multi_row(int64_t r, int64_t U, int64_t Q, const int64_t *__restrict__ pos_rowptr, int64_t &q,
                                          int64_t &first, int &n) {
    q = 0;
    first = 0;
    n = 0;
    int64_t b, e;
    if (r < U) {
        q = r;
        pos_span(pos_rowptr, q, Q, b, e);
        first = b;
    } else {
        const int64_t at = (r - U + 1) * kPC;
        int64_t lo = 0, hi = U;             // the last user whose row starts at or before `at`
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (pos_rowptr[mid] <= at) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) return;
        q = lo - 1;
        pos_span(pos_rowptr, q, Q, b, e);
        if (at <= b || at >= e) return;     // at == b: the chunk that starts here is the user's chunk 0, row q
        first = b + (at - b + kPC - 1) / kPC * kPC;
        if (first >= e) return;
    }
    n = (int)(e - first < kPC ? e - first : kPC);
}

// one catalogue score against the first T of a row's thresholds: two strict counters per threshold
template <int T, int M>
__device__ __forceinline__ void multi_count(float s, const float (&thr)[M], int (&hi)[M], int (&lo)[M]) {
#pragma unroll
    for (int k = 0; k < T; ++k) {
        hi[k] += s > thr[k] ? 1 : 0;
        lo[k] += s < thr[k] ? 1 : 0;
    }
}

// a row's counters of item range `col` go to the workspace: part [cols, 2, pc, rows], pc = multi_chunk
template <int M>
__device__ __forceinline__ void multi_store(int *__restrict__ part, int64_t col, int pc, int64_t rows, int64_t r, int n,
                                            const int (&hi)[M], const int (&lo)[M]) {
#pragma unroll
    for (int k = 0; k < M; ++k) {
        if (k >= n) break;
        part[((col * 2) * pc + k) * rows + r] = hi[k];
        part[((col * 2 + 1) * pc + k) * rows + r] = lo[k];
    }
}

// The threads that share a user in the kernel that scores the positives (256 threads per workgroup): a wave with a row
// pointer, the thread alone without one, where the user has one positive.  Gives the thread's user and its place.
__device__ __forceinline__ void pos_team(const int64_t *__restrict__ pos_rowptr, int64_t &q, int &lane, int &team) {
    team = pos_rowptr ? kWave : 1;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    q = t / team;
    lane = (int)(t % team);
}
inline unsigned pos_blocks(int64_t U, bool row_pointer) { return (unsigned)((U * (row_pointer ? kWave : 1) + 255) / 256); }

// Thread `lane` of a user's team over the user's positives: their scores, the thresholds of the scan ([Q], flat order).
// score_pos(j) scores flat positive j with the bits the scan gives its catalogue row.
template <class Scorer>
__device__ __forceinline__ void multi_thresholds(int64_t q, int64_t Q, const int64_t *__restrict__ pos_rowptr, int lane, int team,
                                                 const Scorer &score_pos, float *__restrict__ thr) {
    int64_t b, e;
    pos_span(pos_rowptr, q, Q, b, e);
    for (int64_t j = b + lane; j < e; j += team) thr[j] = score_pos(j);
}

// where the finish of a rank call writes.  above and below are its running counters as well, so the caller of a
// single-positive entry point who wants neither is handed room in the workspace; the rest may be null.
struct RankOut {
    int32_t *above, *below;     // [Q]
    float *pos_score;           // [Q] or null
    int32_t *n_neg;             // [U] or null
    float *auc;                 // [Q] or null: (float)below / (float)n_neg of the positive's user, 0 without negatives
};

// The finish of user q by one wave, once the scans have counted (s > t) and (s < t) over EVERY catalogue item for each of
// the user's thresholds t.  Lane j sums the item ranges' partial counts of threshold j in range order.  Then what is no
// negative is taken out: the exclusion entries inside the catalogue, and the user's own positives inside the catalogue
// that the exclusion row does not already name (both rows ascend, so that is a search).  64 of them at a time, a lane
// each, are scored ONCE by score(node) -- the bits the scan compared -- and every score is passed round the wave against
// the thresholds the lanes hold.  A positive compares equal to its own threshold and so leaves it alone.  The counters
// live in out.above / out.below: lane j alone reads and writes entry j.
template <class Scorer>
__device__ __forceinline__ void rank_multi_finish(int64_t q, int64_t U, int64_t Q, int64_t rows, int pc, int cols, int64_t n_items,
                                                  int64_t item_lo, const int64_t *__restrict__ pos_rowptr,
                                                  const int64_t *__restrict__ pos_items, const float *__restrict__ thr,
                                                  const int64_t *__restrict__ excl_rowptr,
                                                  const int64_t *__restrict__ excl_items, const int *__restrict__ part,
                                                  const Scorer &score, int lane, const RankOut &out) {
    int64_t pb, pe;
    pos_span(pos_rowptr, q, Q, pb, pe);
    const int64_t P = pe - pb;
    for (int64_t j = lane; j < P; j += kWave) {
        const int64_t r = multi_row_of(q, U, pb, j);
        const int k = (int)(j % kPC);
        int hi = 0, lo = 0;
        for (int c = 0; c < cols; ++c) {
            hi += part[(((int64_t)c * 2) * pc + k) * rows + r];
            lo += part[(((int64_t)c * 2 + 1) * pc + k) * rows + r];
        }
        out.above[pb + j] = hi;
        out.below[pb + j] = lo;
        if (out.pos_score) out.pos_score[pb + j] = thr[pb + j];
    }
    const int64_t eb = excl_rowptr ? excl_rowptr[q] : 0, ee = excl_rowptr ? excl_rowptr[q + 1] : 0;
    const int64_t E = ee > eb ? ee - eb : 0, L = E + P;
    int64_t gone = 0;
    for (int64_t base = 0; base < L; base += kWave) {
        const int64_t x = base + lane;
        bool live = false;
        float s = 0.f;
        if (x < L) {
            const int64_t node = x < E ? excl_items[eb + x] : pos_items[pb + (x - E)];
            live = node >= item_lo && node < item_lo + n_items;
            if (live && x >= E) live = !in_sorted(excl_items, eb, eb + E, node);
            if (live) s = score(node);
        }
        const unsigned long long mask = __ballot(live);
        gone += __popcll(mask);
        if (mask == 0) continue;
        for (int64_t j0 = 0; j0 < P; j0 += kWave) {
            const int64_t j = j0 + lane;
            const float t = j < P ? thr[pb + j] : 0.f;
            int dh = 0, dl = 0;
            for (unsigned long long m = mask; m != 0; m &= m - 1) {
                const float sk = __shfl(s, __ffsll((long long)m) - 1);
                dh += sk > t ? 1 : 0;
                dl += sk < t ? 1 : 0;
            }
            if (j < P && (dh | dl) != 0) {
                out.above[pb + j] -= dh;
                out.below[pb + j] -= dl;
            }
        }
    }
    const int64_t others = n_items - gone;
    if (lane == 0 && out.n_neg) out.n_neg[q] = (int32_t)others;
    if (out.auc)
        for (int64_t j = lane; j < P; j += kWave) out.auc[pb + j] = others > 0 ? (float)out.below[pb + j] / (float)others : 0.f;
}

// A wave per user is the faster finish while the waves are few: its 64 lanes share the ~150 entries of an exclusion row.
// Over very many users a thread each fills the machine and walks its row alone at a better rate per user (measured on
// the inner product, D = 112, rows of ~150 entries: 162,541 users 3.6 ms by waves against 10.0 ms by threads; 1,704,853
// users 26.5 against 15.8 ms; the two cross near half a million).  So the inner product's call without a row pointer over
// at least kThreadFinishUsers users takes rank_finish below: the same counts and the same bits, by one thread.  The
// threshold looks at U alone and comes from that one shape; where the two cross also moves with the rows' length.
constexpr int64_t kThreadFinishUsers = (int64_t)1 << 19;


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
