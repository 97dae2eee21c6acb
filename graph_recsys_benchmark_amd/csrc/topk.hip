// Full-catalogue scoring for gfx950: top-K recommendation lists and the all-item rank of a held-out positive.
//   predict      graph_recsys_benchmark/models/base.py:208-214   fc2(relu(fc1([repr[u] || repr[i]])))
//   rank / auc   solvers.py:85-96, utils/rec_utils.py:7-30       over EVERY eligible item instead of 99 sampled ones
// fc1 splits by columns, so the user half A[u] = fc1_b + W_u repr[u] and the item half B[i] = W_i repr[i] are computed
// once per requested user / catalogue item (topk_prep) and a pair costs R x (add, max, fma):
//   s(u, i) = (fma chain over k of max(A[u,k] + B[i,k], 0) * fc2_w[k], from 0) + fc2_b            (pair_score)
// Every score of this file goes through pair_score on rows written by topk_prep, so a pair has the same bits wherever
// it is computed (top-K scan, rank scan, the exclusion walk of rank_full, any U / K / item split).  No float atomics.
// pea_rank_full keeps a scan of its own, the RANK form of topk_scan_kernel: over 1.7 M users the T = 1 scan of the
// several-positives rank was measured 3.7 % slower (profiles/r18/rank_one_scan.md); the inner product's pea_dot_rank_full
// IS its several-positives call.
#include <algorithm>

#include "score_common.h"
#include "topk_select.h"
#include "../../include/peahip_eval.h"

namespace pea {
namespace {

constexpr int kTileFloats = 2048;   // LDS tile of item rows: 8 KB = 128 rows at R = 16

// rows are padded to RP in {16, 32, 64} columns with zeros (A, B and fc2_w alike): a padded column adds
// fma(max(0 + 0, 0), 0, o) = o, so the padding changes no bit of the score
int padded_r(int R) { return R <= 16 ? 16 : (R <= 32 ? 32 : 64); }

// what topk_prep writes, at the head of every workspace of this file: fc2_w padded, the user halves A [U, RP], the
// positives' item halves P [Q, RP] and the catalogue's item halves B [n_items, RP]
struct Prep {
    int RP = 16;
    size_t off_w2 = 0, off_a = 0, off_p = 0, off_b = 0, end = 0;
};

Prep make_prep(int64_t U, int64_t Q, int64_t n_items, int R) {
    Prep p;
    p.RP = padded_r(R);
    size_t o = 256;                                                           // error flag
    p.off_w2 = o; o = align256(o + (size_t)p.RP * 4);
    p.off_a = o;  o = align256(o + (size_t)std::max<int64_t>(U, 1) * p.RP * 4);
    p.off_p = o;  o = align256(o + (size_t)std::max<int64_t>(Q, 1) * p.RP * 4);
    p.off_b = o;  o = align256(o + (size_t)std::max<int64_t>(n_items, 1) * p.RP * 4);
    p.end = o;
    return p;
}

struct Layout {
    Prep prep;
    int NT = 128, S = 1;
    int64_t span = 0;
    size_t off_part = 0, bytes = 0;
};

// How a call is cut: NT users per workgroup (one per lane), the catalogue in S item ranges of `span` items so that few
// users still fill the machine.  Depends on (U, n_items, K, R) only, so the workspace query and the call agree.
Layout make_layout(int64_t U, int64_t n_items, int K, int R) {
    Layout L;
    L.prep = make_prep(U, U, n_items, R);      // P: the positives of pea_rank_full
    L.NT = K <= 32 ? 128 : 64;      // a lane's K-entry list is an LDS column of 8 K bytes
    catalogue_split(std::max<int64_t>((U + L.NT - 1) / L.NT, 1), n_items, std::max(K, 1), kTileFloats / L.prep.RP, &L.S, &L.span);
    L.off_part = L.prep.end;
    L.bytes = align256(L.off_part + (size_t)L.S * std::max(K, 1) * std::max<int64_t>(U, 1) * 8);
    return L;
}

// ---------------------------------------------------------------------------------------------- prep
// One thread per (row, column): rows [0, U) the user halves A, [U, U + U_pos) the positives' item halves (the rank forms),
// the rest the catalogue's item halves B.  Fixed summation order: c ascending, bias last.
__global__ __launch_bounds__(256) void topk_prep_kernel(int64_t U, int64_t U_pos, int64_t n_items, int R, int RP, int64_t N,
                                                        const float *__restrict__ repr, const int64_t *__restrict__ unids,
                                                        const int64_t *__restrict__ pos_items, int64_t item_lo,
                                                        const float *__restrict__ fc1_w, const float *__restrict__ fc1_b,
                                                        const float *__restrict__ fc2_w, float *__restrict__ A,
                                                        float *__restrict__ P, float *__restrict__ B,
                                                        float *__restrict__ w2p, int *err) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < RP) w2p[t] = t < R ? fc2_w[t] : 0.f;
    const int64_t row = t / RP;
    const int k = (int)(t % RP);
    if (row >= U + U_pos + n_items) return;
    int64_t node;
    float *dst;
    bool user_half = false;
    if (row < U) {
        node = unids[row];
        dst = A + row * RP;
        user_half = true;
    } else if (row < U + U_pos) {
        node = pos_items[row - U];
        dst = P + (row - U) * RP;
    } else {
        node = item_lo + (row - U - U_pos);
        dst = B + (row - U - U_pos) * RP;
    }
    if (node < 0 || node >= N) {
        if (k == 0) atomicOr(err, 1);
        dst[k] = 0.f;
        return;
    }
    if (k >= R) {
        dst[k] = 0.f;
        return;
    }
    const float *w = fc1_w + (int64_t)k * 2 * R + (user_half ? 0 : R);
    const float *x = repr + node * R;
    float acc = 0.f;
    for (int c = 0; c < R; ++c) acc += w[c] * x[c];
    dst[k] = user_half ? acc + fc1_b[k] : acc;
}

// the one place a pair is scored: a = the user's half (registers), b = the item's half (LDS tile or global row)
template <int RP>
__device__ __forceinline__ float pair_score(const float (&a)[RP], const float *b, const float *__restrict__ w2, float b2) {
    float o = 0.f;
#pragma unroll
    for (int k = 0; k < RP; k += 4) {
        const float4 v = ld4(b + k);
        o = fmaf(fmaxf(a[k] + v.x, 0.f), w2[k], o);
        o = fmaf(fmaxf(a[k + 1] + v.y, 0.f), w2[k + 1], o);
        o = fmaf(fmaxf(a[k + 2] + v.z, 0.f), w2[k + 2], o);
        o = fmaf(fmaxf(a[k + 3] + v.w, 0.f), w2[k + 3], o);
    }
    return o + b2;
}

// pair_score of four consecutive item rows, the four chains advanced side by side: per item the very same operations in
// the very same order as pair_score, so the same bits
template <int RP>
__device__ __forceinline__ void pair_score4(const float (&a)[RP], const float *b, const float *__restrict__ w2, float b2,
                                            float (&out)[4]) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < RP; k += 4) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ld4(b + j * RP + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(fmaxf(a[k] + v[j].x, 0.f), w2[k], o[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(fmaxf(a[k + 1] + v[j].y, 0.f), w2[k + 1], o[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(fmaxf(a[k + 2] + v[j].z, 0.f), w2[k + 2], o[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(fmaxf(a[k + 3] + v[j].w, 0.f), w2[k + 3], o[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = o[j] + b2;
}

template <int RP>
__device__ __forceinline__ void load_half(const float *p, float (&a)[RP]) {
#pragma unroll
    for (int k = 0; k < RP; k += 4) {
        const float4 v = ld4(p + k);
        a[k] = v.x; a[k + 1] = v.y; a[k + 2] = v.z; a[k + 3] = v.w;
    }
}

struct ScanArgs {
    int64_t U, n_items, item_lo, span;
    int K;
    const float *A, *B, *P, *w2, *fc2_b;
    const int64_t *excl_rowptr, *excl_items;
    float *part_s;   // top-K: [S, K, U] scores          rank: unused
    int *part_i;     // top-K: [S, K, U] catalogue index  rank: [S, 2, U] counts of (s > pos), (s < pos)
};

extern __shared__ float topk_smem[];

// A lane owns one user (its half A[q] in RP registers); the workgroup streams its item range through an LDS tile and all
// lanes read the same item row at once (identical addresses: broadcast).
//   RANK = false: the lane keeps its K best (score, index) in the list of topk_select.h.  Only a score above the list's
//     threshold is looked up in the exclusion list and inserted.  The (user, range) column goes to the workspace for
//     topk_merge.
//   RANK = true: two counters, s > pos and s < pos, over every item of the range (exclusions are taken out afterwards by
//     rank_full_kernel, exact because a pair's score has the same bits there).
template <int RP, bool RANK, int NT>
__global__ __launch_bounds__(NT) void topk_scan_kernel(const ScanArgs g) {
    constexpr int TI = kTileFloats / RP;
    float *tile = topk_smem;
    float *ls = topk_smem + kTileFloats;                      // [K][NT]
    int *li = reinterpret_cast<int *>(ls + (RANK ? 0 : g.K * NT));
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * NT + tid;
    const bool valid = q < g.U;
    const int64_t qr = valid ? q : g.U - 1;
    float a[RP];
    load_half<RP>(g.A + qr * RP, a);
    const float b2 = g.fc2_b[0];
    const int K = g.K;
    float pos = 0.f, thr = -INFINITY;
    int hi = 0, lo = 0, wslot = 0;
    int64_t ex_lo = 0, ex_hi = 0;
    if (RANK) {
        pos = pair_score<RP>(a, g.P + qr * RP, g.w2, b2);
    } else {
        // list_init of topk_select.h, written out: with the call inlined here the compiler lowers the control flow of the
        // scan loop below differently (same registers and occupancy, 2.8 % slower on the all-users shape;
        // profiles/r08/scoring_refactor.md, section 3)
        for (int j = 0; j < K; ++j) {
            ls[j * NT + tid] = -INFINITY;
            li[j * NT + tid] = kEmpty;
        }
        if (g.excl_rowptr) {
            ex_lo = g.excl_rowptr[qr];
            ex_hi = g.excl_rowptr[qr + 1];
        }
    }
    const int64_t i0 = (int64_t)blockIdx.y * g.span;
    const int64_t i1 = i0 + g.span < g.n_items ? i0 + g.span : g.n_items;
    for (int64_t t0 = i0; t0 < i1; t0 += TI) {
        const int nt = (int)(i1 - t0 < TI ? i1 - t0 : TI);
        __syncthreads();
        for (int x = tid; x < nt * (RP / 4); x += NT)
            reinterpret_cast<float4 *>(tile)[x] = ld4(g.B + t0 * RP + (int64_t)x * 4);
        __syncthreads();
        // four items at a time: their fma chains are independent, so the scheduler interleaves them (one chain alone
        // waits on itself).  Rows past nt inside the tile are scored from stale LDS and ignored.
        for (int j0 = 0; j0 < nt; j0 += 4) {
            float s4[4];
            pair_score4<RP>(a, tile + j0 * RP, g.w2, b2, s4);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float s = s4[jj];
                if (j0 + jj >= nt) break;
                if (RANK) {
                    hi += s > pos ? 1 : 0;
                    lo += s < pos ? 1 : 0;
                } else if (s > thr) {
                    const int idx = (int)(t0 + j0 + jj);
                    if (ex_lo < ex_hi && in_sorted(g.excl_items, ex_lo, ex_hi, g.item_lo + idx)) continue;
                    list_insert(ls, li, NT, tid, K, s, idx, wslot, thr);
                }
            }
        }
    }
    if (!valid) return;
    if (RANK) {
        g.part_i[((int64_t)blockIdx.y * 2) * g.U + q] = hi;
        g.part_i[((int64_t)blockIdx.y * 2 + 1) * g.U + q] = lo;
    } else {
        list_store(ls, li, NT, tid, K, blockIdx.y, g.U, q, g.part_s, g.part_i);
    }
}

// (the per-range columns are ordered by topk_merge_kernel of topk_select.h)

// One thread per user: rank_finish of topk_select.h with pair_score on the same rows the scan compared (the same bits).
template <int RP>
__global__ __launch_bounds__(64) void rank_full_kernel(int64_t U, int S, int64_t n_items, int64_t item_lo,
                                                       const float *__restrict__ A, const float *__restrict__ B,
                                                       const float *__restrict__ P, const float *__restrict__ w2,
                                                       const float *__restrict__ fc2_b, const int64_t *__restrict__ pos_items,
                                                       const int64_t *__restrict__ excl_rowptr,
                                                       const int64_t *__restrict__ excl_items, const int *__restrict__ part,
                                                       int32_t *rank, float *auc, float *pos_score) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= U) return;
    float a[RP];
    load_half<RP>(A + q * RP, a);
    const float b2 = fc2_b[0];
    const float pos = pair_score<RP>(a, P + q * RP, w2, b2);
    rank_finish(q, U, S, n_items, item_lo, pos, pos_items[q], excl_rowptr, excl_items, part,
                [&](int64_t node) { return pair_score<RP>(a, B + (node - item_lo) * RP, w2, b2); }, rank, auc, pos_score);
}

template <int RP, bool RANK, int NT>
int launch_scan_nt(const Layout &L, const ScanArgs &g, hipStream_t stream) {
    const size_t lds = (size_t)kTileFloats * 4 + (RANK ? 0 : (size_t)g.K * NT * 8);
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&topk_scan_kernel<RP, RANK, NT>), lds));
    const dim3 grid((unsigned)((g.U + NT - 1) / NT), (unsigned)L.S);
    PEA_LAUNCH((topk_scan_kernel<RP, RANK, NT>), grid, dim3(NT), lds, stream, g);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

template <bool RANK>
int launch_scan(const Layout &L, const ScanArgs &g, hipStream_t stream) {
    if (RANK || L.NT == 128) {
        if (L.prep.RP == 16) return launch_scan_nt<16, RANK, 128>(L, g, stream);
        if (L.prep.RP == 32) return launch_scan_nt<32, RANK, 128>(L, g, stream);
        return launch_scan_nt<64, RANK, 128>(L, g, stream);
    }
    if (L.prep.RP == 16) return launch_scan_nt<16, false, 64>(L, g, stream);
    if (L.prep.RP == 32) return launch_scan_nt<32, false, 64>(L, g, stream);
    return launch_scan_nt<64, false, 64>(L, g, stream);
}

int check_r(const char *what, int R) {
    PEA_REQUIRE(R > 0 && R % 4 == 0 && R <= 64, PEA_ERR_ARG, "%s: repr_dim %d must be a multiple of 4, <= 64", what, R);
    return PEA_OK;
}

int launch_prep(const Prep &p, int64_t U, int64_t U_pos, int64_t n_items, int R, int64_t N, const float *repr,
                const int64_t *unids, const int64_t *pos_items, int64_t item_lo, const float *fc1_w, const float *fc1_b,
                const float *fc2_w, char *ws, hipStream_t stream) {
    ProfScope ps("topk_prep", stream, 4.0 * (double)(U + U_pos + n_items) * (R + p.RP));
    const int64_t threads = std::max<int64_t>((U + U_pos + n_items) * p.RP, p.RP);
    PEA_LAUNCH(topk_prep_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, U, U_pos, n_items, R, p.RP, N,
               repr, unids, pos_items, item_lo, fc1_w, fc1_b, fc2_w, (float *)(ws + p.off_a), (float *)(ws + p.off_p),
               (float *)(ws + p.off_b), (float *)(ws + p.off_w2), (int *)ws);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

// ---------------------------------------------------------------------------------------------- several positives per user
// pea_rank_full_multi (include/peahip_eval.h): the rows, counters and finish of topk_select.h with pair_score.
struct MultiLayout {
    Prep prep;
    int S = 1;
    int64_t span = 0, rows = 0;
    size_t off_thr = 0, off_part = 0, bytes = 0;
};

constexpr int kMultiNT = 128;       // rows of one workgroup of the scan, one per lane

// Depends on (U, Q, n_items, R) only: the rows are the bound multi_rows, not the rows in use.
MultiLayout make_multi_layout(int64_t U, int64_t Q, int64_t n_items, int R) {
    MultiLayout L;
    L.prep = make_prep(U, Q, n_items, R);
    L.rows = multi_rows(U, Q, true);
    catalogue_split(std::max<int64_t>((L.rows + kMultiNT - 1) / kMultiNT, 1), n_items, 1, kTileFloats / L.prep.RP, &L.S, &L.span);
    size_t o = L.prep.end;
    L.off_thr = o;  o = align256(o + (size_t)std::max<int64_t>(Q, 1) * 4);
    L.off_part = o; o = align256(o + (size_t)L.S * 2 * kPC * std::max<int64_t>(L.rows, 1) * 4);
    L.bytes = o;
    return L;
}

struct MultiArgs {
    int64_t U, Q, rows, n_items, item_lo, span;
    int S;
    const float *A, *B, *P, *w2, *fc2_b;
    const int64_t *pos_rowptr, *pos_items, *excl_rowptr, *excl_items;
    float *thr;      // [Q] the positives' scores
    int *part;       // [S, 2, kPC, rows] counts of (s > t), (s < t)
};

// one wave per user: multi_thresholds with pair_score on the rows topk_prep wrote
template <int RP>
__global__ __launch_bounds__(256) void rank_multi_pos_kernel(const MultiArgs g) {
    const int lane = threadIdx.x % kWave;
    const int64_t q = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (q >= g.U) return;
    float a[RP];
    load_half<RP>(g.A + q * RP, a);
    const float b2 = g.fc2_b[0];
    multi_thresholds(q, g.Q, g.pos_rowptr, lane, kWave, [&](int64_t j) { return pair_score<RP>(a, g.P + j * RP, g.w2, b2); }, g.thr);
}

// topk_scan_kernel's RANK loop with a (user, chunk) row per lane and multi_count over T thresholds in place of the two
// counters.  Both instantiations are launched over all the rows: T = 1 takes the workgroups whose rows hold one threshold
// at the most (with one positive per user that is every workgroup, at the registers and occupancy of the single-positive
// scan), T = kPC the others; a workgroup that is not this kernel's, or whose rows are all idle, leaves at once.
template <int RP, int T>
__global__ __launch_bounds__(kMultiNT) void rank_multi_scan_kernel(const MultiArgs g) {
    constexpr int NT = kMultiNT, TI = kTileFloats / RP;
    float *tile = topk_smem;
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * NT + tid;
    int64_t q = 0, first = 0;
    int n = 0;
    if (r < g.rows) multi_row(r, g.U, g.Q, g.pos_rowptr, q, first, n);
    const bool many = __syncthreads_or(n > 1) != 0;
    if (T == 1 ? (many || !__syncthreads_or(n > 0)) : !many) return;
    float a[RP];
    load_half<RP>(g.A + q * RP, a);
    const float b2 = g.fc2_b[0];
    float thr[T];
    int hi[T], lo[T];
#pragma unroll
    for (int k = 0; k < T; ++k) {
        thr[k] = k < n ? g.thr[first + k] : 0.f;
        hi[k] = lo[k] = 0;
    }
    const int64_t i0 = (int64_t)blockIdx.y * g.span;
    const int64_t i1 = i0 + g.span < g.n_items ? i0 + g.span : g.n_items;
    for (int64_t t0 = i0; t0 < i1; t0 += TI) {
        const int nt = (int)(i1 - t0 < TI ? i1 - t0 : TI);
        __syncthreads();
        for (int x = tid; x < nt * (RP / 4); x += NT)
            reinterpret_cast<float4 *>(tile)[x] = ld4(g.B + t0 * RP + (int64_t)x * 4);
        __syncthreads();
        // rows past nt inside the tile are scored from stale LDS and ignored, as in topk_scan_kernel
        for (int j0 = 0; j0 < nt; j0 += 4) {
            float s4[4];
            pair_score4<RP>(a, tile + j0 * RP, g.w2, b2, s4);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (j0 + jj >= nt) break;
                multi_count<T>(s4[jj], thr, hi, lo);
            }
        }
    }
    if (n > 0) multi_store(g.part, blockIdx.y, kPC, g.rows, r, n, hi, lo);
}

// one wave per user: rank_multi_finish of topk_select.h with pair_score on the rows the scan compared (the same bits)
template <int RP>
__global__ __launch_bounds__(256) void rank_multi_finish_kernel(const MultiArgs g, const RankOut out) {
    const int lane = threadIdx.x % kWave;
    const int64_t q = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (q >= g.U) return;
    float a[RP];
    load_half<RP>(g.A + q * RP, a);
    const float b2 = g.fc2_b[0];
    rank_multi_finish(q, g.U, g.Q, g.rows, kPC, g.S, g.n_items, g.item_lo, g.pos_rowptr, g.pos_items, g.thr, g.excl_rowptr,
                      g.excl_items, g.part,
                      [&](int64_t node) { return pair_score<RP>(a, g.B + (node - g.item_lo) * RP, g.w2, b2); }, lane, out);
}

template <int RP>
int launch_multi(const MultiArgs &g, int R, const RankOut &out, hipStream_t stream) {
    const dim3 waves((unsigned)((g.U + 3) / 4));
    if (g.Q > 0) {
        {
            ProfScope ps("rank_multi_pos", stream, (double)g.Q * (4.0 * RP + 4.0));
            PEA_LAUNCH(rank_multi_pos_kernel<RP>, waves, dim3(256), 0, stream, g);
            PEA_HIP(hipGetLastError());
        }
        ProfScope ps("rank_multi_scan", stream, (double)g.rows * (double)g.n_items * (3.0 * R + 4.0 * kPC));
        const size_t lds = (size_t)kTileFloats * 4;
        const dim3 grid((unsigned)((g.rows + kMultiNT - 1) / kMultiNT), (unsigned)g.S);
        PEA_LAUNCH((rank_multi_scan_kernel<RP, 1>), grid, dim3(kMultiNT), lds, stream, g);
        PEA_LAUNCH((rank_multi_scan_kernel<RP, kPC>), grid, dim3(kMultiNT), lds, stream, g);
        PEA_HIP(hipGetLastError());
    }
    ProfScope ps("rank_multi_finish", stream, 8.0 * (double)g.Q * g.S);
    PEA_LAUNCH(rank_multi_finish_kernel<RP>, waves, dim3(256), 0, stream, g, out);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace
}  // namespace pea

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" size_t pea_topk_workspace_bytes(int64_t U, int64_t n_items, int K, int R) {
    if (U < 0 || n_items < 0 || K < 1 || K > 128 || R <= 0 || R > 64) return 0;
    return pea::make_layout(U, n_items, K, R).bytes;
}

extern "C" int pea_recommend_topk(int64_t U, int K, int R, int64_t num_nodes, const float *repr, const int64_t *unids,
                                  int64_t item_lo, int64_t n_items, const int64_t *excl_rowptr,
                                  const int64_t *excl_items, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                                  const float *fc2_b, int64_t *out_items, float *out_scores, void *workspace,
                                  size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(K >= 1 && K <= 128, PEA_ERR_ARG, "recommend_topk: K=%d (1..128)", K);
    PEA_TRY(check_r("recommend_topk", R));
    PEA_TRY(check_catalogue("recommend_topk", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(repr && unids && fc1_w && fc1_b && fc2_w && fc2_b && out_items && out_scores && workspace, PEA_ERR_ARG,
                "recommend_topk: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "recommend_topk: excl_rowptr without excl_items");
    const Layout L = make_layout(U, n_items, K, R);
    PEA_REQUIRE(workspace_bytes >= L.bytes, PEA_ERR_NOMEM, "recommend_topk: workspace too small (%zu < %zu)", workspace_bytes,
                L.bytes);
    if (U == 0) return PEA_OK;
    char *ws = (char *)workspace;
    PEA_MEMSET_ASYNC((int *)ws, 0, sizeof(int), stream);
    PEA_TRY(launch_prep(L.prep, U, 0, n_items, R, num_nodes, repr, unids, nullptr, item_lo, fc1_w, fc1_b, fc2_w, ws, stream));
    ScanArgs g;
    g.U = U; g.n_items = n_items; g.item_lo = item_lo; g.span = L.span; g.K = K;
    g.A = (const float *)(ws + L.prep.off_a); g.B = (const float *)(ws + L.prep.off_b); g.P = nullptr;
    g.w2 = (const float *)(ws + L.prep.off_w2); g.fc2_b = fc2_b;
    g.excl_rowptr = excl_rowptr; g.excl_items = excl_items;
    g.part_s = (float *)(ws + L.off_part);
    g.part_i = (int *)(ws + L.off_part + (size_t)L.S * K * U * 4);
    {
        ProfScope ps("topk_scan", stream, (double)U * (double)n_items * 3.0 * R);
        PEA_TRY(launch_scan<false>(L, g, stream));
    }
    {
        ProfScope ps("topk_merge", stream, 8.0 * (double)U * K * (L.S + 1.5));
        int p2 = 2;
        while (p2 < L.S * K) p2 <<= 1;      // <= kMaxMerge: make_layout keeps S K <= 2048
        PEA_LAUNCH(topk_merge_kernel, dim3((unsigned)U), dim3(p2 <= 128 ? 64 : 256), 0, stream, U, K, L.S, p2, item_lo,
                   (const float *)g.part_s, (const int *)g.part_i, out_items, out_scores);
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag((int *)ws, stream, "recommend_topk");
}

extern "C" int pea_rank_full(int64_t U, int R, int64_t num_nodes, const float *repr, const int64_t *unids,
                             const int64_t *pos_items, int64_t item_lo, int64_t n_items, const int64_t *excl_rowptr,
                             const int64_t *excl_items, const float *fc1_w, const float *fc1_b, const float *fc2_w,
                             const float *fc2_b, int32_t *rank, float *auc, float *pos_score, void *workspace,
                             size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r("rank_full", R));
    PEA_TRY(check_catalogue("rank_full", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(repr && unids && pos_items && fc1_w && fc1_b && fc2_w && fc2_b && workspace, PEA_ERR_ARG,
                "rank_full: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "rank_full: excl_rowptr without excl_items");
    const Layout L = make_layout(U, n_items, 1, R);
    PEA_REQUIRE(workspace_bytes >= L.bytes, PEA_ERR_NOMEM, "rank_full: workspace too small (%zu < %zu)", workspace_bytes, L.bytes);
    if (U == 0) return PEA_OK;
    char *ws = (char *)workspace;
    PEA_MEMSET_ASYNC((int *)ws, 0, sizeof(int), stream);
    PEA_TRY(launch_prep(L.prep, U, U, n_items, R, num_nodes, repr, unids, pos_items, item_lo, fc1_w, fc1_b, fc2_w, ws, stream));
    ScanArgs g;
    g.U = U; g.n_items = n_items; g.item_lo = item_lo; g.span = L.span; g.K = 0;
    g.A = (const float *)(ws + L.prep.off_a); g.B = (const float *)(ws + L.prep.off_b); g.P = (const float *)(ws + L.prep.off_p);
    g.w2 = (const float *)(ws + L.prep.off_w2); g.fc2_b = fc2_b;
    g.excl_rowptr = nullptr; g.excl_items = nullptr;
    g.part_s = nullptr;
    g.part_i = (int *)(ws + L.off_part);
    {
        ProfScope ps("rank_full", stream, (double)U * (double)n_items * 3.0 * R);
        PEA_TRY(launch_scan<true>(L, g, stream));
#define PEA_RANK_FINISH(rp)                                                                                              \
    PEA_LAUNCH(rank_full_kernel<rp>, dim3((unsigned)((U + 63) / 64)), dim3(64), 0, stream, U, L.S, n_items, item_lo, g.A, \
               g.B, g.P, g.w2, fc2_b, pos_items, excl_rowptr, excl_items, (const int *)g.part_i, rank, auc, pos_score)
        if (L.prep.RP == 16) PEA_RANK_FINISH(16);
        else if (L.prep.RP == 32) PEA_RANK_FINISH(32);
        else PEA_RANK_FINISH(64);
#undef PEA_RANK_FINISH
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag((int *)ws, stream, "rank_full");
}

// include/peahip_eval.h
extern "C" size_t pea_rank_multi_workspace_bytes(int64_t U, int64_t Q, int64_t n_items, int R) {
    if (U < 0 || Q < 0 || n_items < 0 || n_items >= ((int64_t)1 << 31) - 1 || R <= 0 || R > 64 || R % 4 != 0) return 0;
    return pea::make_multi_layout(U, Q, n_items, R).bytes;
}

extern "C" int pea_rank_full_multi(int64_t U, int R, int64_t num_nodes, const float *repr, const int64_t *unids,
                                   const int64_t *pos_rowptr, const int64_t *pos_items, int64_t Q, int64_t item_lo,
                                   int64_t n_items, const int64_t *excl_rowptr, const int64_t *excl_items, const float *fc1_w,
                                   const float *fc1_b, const float *fc2_w, const float *fc2_b, int32_t *above, int32_t *below,
                                   float *pos_score, int32_t *n_neg, void *workspace, size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_r("rank_full_multi", R));
    PEA_TRY(check_catalogue("rank_full_multi", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(Q >= 0, PEA_ERR_ARG, "rank_full_multi: Q=%lld", (long long)Q);
    PEA_REQUIRE(repr && unids && pos_rowptr && pos_items && fc1_w && fc1_b && fc2_w && fc2_b && above && below && pos_score &&
                    n_neg && workspace,
                PEA_ERR_ARG, "rank_full_multi: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "rank_full_multi: excl_rowptr without excl_items");
    const MultiLayout L = make_multi_layout(U, Q, n_items, R);
    PEA_REQUIRE(workspace_bytes >= L.bytes, PEA_ERR_NOMEM, "rank_full_multi: workspace too small (%zu < %zu)", workspace_bytes,
                L.bytes);
    if (U == 0) return PEA_OK;
    char *ws = (char *)workspace;
    PEA_MEMSET_ASYNC((int *)ws, 0, sizeof(int), stream);
    PEA_TRY(launch_prep(L.prep, U, Q, n_items, R, num_nodes, repr, unids, pos_items, item_lo, fc1_w, fc1_b, fc2_w, ws, stream));
    MultiArgs g;
    g.U = U; g.Q = Q; g.rows = L.rows; g.n_items = n_items; g.item_lo = item_lo; g.span = L.span; g.S = L.S;
    g.A = (const float *)(ws + L.prep.off_a); g.B = (const float *)(ws + L.prep.off_b); g.P = (const float *)(ws + L.prep.off_p);
    g.w2 = (const float *)(ws + L.prep.off_w2); g.fc2_b = fc2_b;
    g.pos_rowptr = pos_rowptr; g.pos_items = pos_items; g.excl_rowptr = excl_rowptr; g.excl_items = excl_items;
    g.thr = (float *)(ws + L.off_thr);
    g.part = (int *)(ws + L.off_part);
    const RankOut out = {above, below, pos_score, n_neg, nullptr};
    if (L.prep.RP == 16) PEA_TRY(launch_multi<16>(g, R, out, stream));
    else if (L.prep.RP == 32) PEA_TRY(launch_multi<32>(g, R, out, stream));
    else PEA_TRY(launch_multi<64>(g, R, out, stream));
    return read_err_flag((int *)ws, stream, "rank_full_multi");
}
