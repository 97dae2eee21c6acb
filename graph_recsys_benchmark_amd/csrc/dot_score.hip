// Inner-product scoring for gfx950: the scorer of the KGAT / KGCN / NGCF baselines (graph_recsys_benchmark/models/
// kgat.py, kgcn.py, ngcf.py: predict = sum(repr[u] * repr[i])) and of every embedding model (MF, LightGCN, two-tower).
//   s(u, i) = fma chain over d = 0 .. D-1 ascending of repr[u, d] * repr[i, d], from +0                       (dot_pair)
//   predict / rank_eval   one pair per thread / one user per wave, plain fmaf (the build has -ffp-contract=off)
//   recommend_topk / rank_full / rank_full_multi   the catalogue scan is a GEMM: v_mfma_f32_16x16x4_f32, k-steps ascending, accumulator
//     from zero.  A step's four k values are d = 4t .. 4t+3 (lane group g holds d = 4t + g), so the tile's accumulation
//     order is the order of dot_pair; the f32-input MFMA rounds like an fmaf chain, which makes a pair's score the same
//     bits in every entry point (tests/test_gpu_dot_score.py checks that on the hardware).  rank_full is rank_full_multi
//     without a row pointer: one positive per user.
// No float atomics; every reduction has a fixed order.
#include <algorithm>

#include "score_common.h"
#include "topk_select.h"
#include "../../include/peahip_eval.h"

namespace pea {
namespace {

constexpr int kTI = 32;             // items of one LDS tile: two 16-row MFMA operands
constexpr int kUW = 32;             // users of one wave: two 16-column MFMA operands, one list per (lane, half)
constexpr int kMaxScanLds = 160 * 1024;     // a CU's LDS
constexpr int kListLdsBudget = 78 * 1024;   // lists + tile of one workgroup: two workgroups fit a CU's 160 KB

// the one definition of a pair's score outside the MFMA tiles
__device__ __forceinline__ float dot_pair(const float *__restrict__ u, const float *__restrict__ v, int D) {
    float o = 0.f;
    for (int d = 0; d < D; d += 4) {
        const float4 a = ld4(u + d), b = ld4(v + d);
        o = fmaf(a.x, b.x, o);
        o = fmaf(a.y, b.y, o);
        o = fmaf(a.z, b.z, o);
        o = fmaf(a.w, b.w, o);
    }
    return o;
}

// ---------------------------------------------------------------------------------------------- pair kernels
__global__ __launch_bounds__(256) void dot_predict_kernel(int64_t B, int D, int64_t N, const float *__restrict__ repr,
                                                          const int64_t *__restrict__ unids,
                                                          const int64_t *__restrict__ inids, float *pred, int *err) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t u = unids[b], i = inids[b];
    if (u < 0 || u >= N || i < 0 || i >= N) {
        atomicOr(err, 1);
        return;
    }
    pred[b] = dot_pair(repr + u * D, repr + i * D, D);
}

// one wave per user: rank_one_user of score_common.h with the inner-product scorer
__global__ __launch_bounds__(256) void dot_rank_kernel(int64_t U, int C, int D, int64_t N, const float *__restrict__ repr,
                                                       const int64_t *__restrict__ unids,
                                                       const int64_t *__restrict__ cand, float *scores, int32_t *rank,
                                                       float *auc, float *loss, int *err) {
    const int lane = threadIdx.x % kWave;
    const int64_t uidx = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (uidx >= U) return;
    const int64_t u = unids[uidx];
    if (u < 0 || u >= N) {
        if (lane == 0) atomicOr(err, 1);
        return;
    }
    rank_one_user([&](int64_t i) { return dot_pair(repr + u * D, repr + i * D, D); },
                  [&](int, int c) { return cand[uidx * C + c]; }, C, N, lane, uidx, scores, rank, auc, loss, err);
}

// ---------------------------------------------------------------------------------------------- catalogue scan
struct Layout {
    int DP = 32, NW = 4, S = 1, LD = 8;
    int64_t span = 0;
    size_t off_part = 0, bytes = 0, lds = 0;
};

// LDS row stride of the item tile in floats: D + 4 or D + 8, whichever makes LD / 4 odd, so that the sixteen rows one
// MFMA operand load touches start in sixteen different 4-bank groups
int tile_ld(int D) { return 4 * ((D / 4 + 1) | 1); }

// How a call is cut.  A wave owns kUW users; a workgroup has NW waves that share the item tile; the catalogue is cut in S
// ranges of `span` items so that few users still fill the machine.  Depends on (U, n_items, K, D) only, so the workspace
// query and the call agree.
Layout make_layout(int64_t U, int64_t n_items, int K, int D) {
    Layout L;
    L.DP = D <= 32 ? 32 : (D <= 64 ? 64 : (D <= 128 ? 128 : 256));
    L.LD = tile_ld(D);
    const size_t tile_bytes = (size_t)kTI * L.LD * 4;
    const size_t list_wave = (size_t)kWave * 2 * K * 8;                 // two lists per lane
    L.NW = 4;
    while (L.NW > 1 && L.NW * list_wave + tile_bytes > (size_t)kListLdsBudget) L.NW >>= 1;
    L.lds = L.NW * list_wave + tile_bytes;
    if (L.lds > (size_t)kMaxScanLds) {          // K > 126 at D = 256 only: give up the conflict-free row stride to fit the CU's LDS
        L.LD = D;
        L.lds = L.NW * list_wave + (size_t)kTI * D * 4;
    }
    const int cols_per_split = 4;                                       // the four lane groups of a user keep own lists
    catalogue_split(std::max<int64_t>((U + kUW * L.NW - 1) / (kUW * L.NW), 1), n_items, cols_per_split * std::max(K, 1), kTI,
                    &L.S, &L.span);
    L.off_part = 256;                                                   // after the error flag
    L.bytes = align256(L.off_part + (size_t)L.S * cols_per_split * std::max(K, 1) * std::max<int64_t>(U, 1) * 8);
    return L;
}

struct ScanArgs {
    int64_t U, N, n_items, item_lo, span;
    int K, D, LD;
    const float *repr;
    const int64_t *unids;
    const int64_t *excl_rowptr, *excl_items;
    float *part_s;        // [S * 4, K, U] scores
    int *part_i;          // [S * 4, K, U] catalogue index
    int *err;
};

// the item tile at the base is written as float4
extern __shared__ __attribute__((aligned(16))) float dot_smem[];

// One step of a catalogue scan, the same in the top-K and the rank kernel.  The workgroup stages the 32 item rows from
// t0 into the LDS tile (two 16-row A operands; rows past the end i1 of the range are zero rows: they score 0 and the
// caller skips them), then every wave runs D / 4 steps of four independent MFMA chains (2 item halves x 2 user halves)
// against its two 16-column B operands ub, held in registers (lane (n, g) = (lane & 15, lane >> 4) holds
// repr[user n, 4t + g] for every step t).  That leaves lane (n, g) with the scores of user n (of either half) against items
// 4g .. 4g + 3 of either item half: acc[item half][user half][j].
template <int DP>
__device__ __forceinline__ void dot_tile_scores(const float *__restrict__ repr, int64_t item_lo, int64_t t0, int64_t i1, int D, int LD,
                                                float *tile, const float (&ub)[2][DP / 4], f32x4 (&acc)[2][2]) {
    const int NT = blockDim.x, tid = threadIdx.x, d4 = D / 4;
    const int lane = tid % kWave, n = lane & 15, grp = lane >> 4;
    const float *a_row0 = tile + n * LD + grp, *a_row1 = tile + (16 + n) * LD + grp;
    __syncthreads();
    for (int x = tid; x < kTI * d4; x += NT) {
        const int r = x / d4, c4 = x - r * d4;
        const float4 v = t0 + r < i1 ? ld4(repr + (item_lo + t0 + r) * D + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(tile + r * LD + 4 * c4) = v;
    }
    __syncthreads();
#pragma unroll
    for (int is = 0; is < 2; ++is)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[is][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < DP / 4; ++t) {
        if (4 * t >= D) break;
        const float a0 = a_row0[4 * t], a1 = a_row1[4 * t];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, ub[0][t], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, ub[1][t], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, ub[0][t], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, ub[1][t], acc[1][1], 0, 0, 0);
    }
}

// Workgroup = NW waves that share the item tile; wave w owns users [32 (NW blockIdx.x + w), + 32), a lane one user of
// either half (dot_tile_scores).  Selection is per lane, with the list of topk_select.h (the lane's items arrive in
// ascending id); the four lane groups of a user keep separate columns (each over its own quarter of the items) and
// topk_merge_kernel folds them with the item ranges'.
// (DP = 256 allocates 194 VGPRs where the version with a rank variant took 193, at the same two waves per SIMD: that is
// ScanArgs without its pos_s pointer, not the call of dot_tile_scores; profiles/r18/rank_one_scan.md.)
template <int DP>
__global__ __launch_bounds__(256) void dot_scan_kernel(const ScanArgs g) {
    const int NT = blockDim.x;
    float *tile = dot_smem;
    float *ls = dot_smem + kTI * g.LD;                         // [2][K][NT]
    int *li = reinterpret_cast<int *>(ls + 2 * g.K * NT);
    const int tid = threadIdx.x;
    const int lane = tid % kWave, n = lane & 15, grp = lane >> 4;
    const int D = g.D, K = g.K;
    const int64_t q0 = ((int64_t)blockIdx.x * (NT / kWave) + tid / kWave) * kUW + n;
    int64_t q[2];
    bool valid[2];
    float ub[2][DP / 4];
    float thr[2];
    int wslot[2] = {0, 0};
    int64_t ex_lo[2] = {0, 0}, ex_hi[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        q[h] = q0 + 16 * h;
        valid[h] = q[h] < g.U;
        // a slot past the last user rides along in the MFMA on a copy of user U - 1; no score passes its threshold, so it
        // keeps no list and searches no exclusions
        thr[h] = valid[h] ? -INFINITY : INFINITY;
        const int64_t qr = valid[h] ? q[h] : g.U - 1;
        int64_t node = g.unids[qr];
        if (node < 0 || node >= g.N) {
            if (grp == 0) atomicOr(g.err, 1);
            node = 0;
        }
        const float *row = g.repr + node * D + grp;
#pragma unroll
        for (int t = 0; t < DP / 4; ++t) ub[h][t] = 4 * t < D ? row[4 * t] : 0.f;
        if (valid[h]) {
            list_init(ls + (h * K) * NT, li + (h * K) * NT, NT, tid, K);
            if (g.excl_rowptr) {
                ex_lo[h] = g.excl_rowptr[qr];
                ex_hi[h] = g.excl_rowptr[qr + 1];
            }
        }
    }
    const int64_t i0 = (int64_t)blockIdx.y * g.span;
    const int64_t i1 = i0 + g.span < g.n_items ? i0 + g.span : g.n_items;
    for (int64_t t0 = i0; t0 < i1; t0 += kTI) {
        f32x4 acc[2][2];
        dot_tile_scores<DP>(g.repr, g.item_lo, t0, i1, D, g.LD, tile, ub, acc);
#pragma unroll
        for (int is = 0; is < 2; ++is) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t it = t0 + 16 * is + 4 * grp + j;
                if (it >= i1) continue;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float s = acc[is][h][j];
                    if (s > thr[h]) {
                        if (ex_lo[h] < ex_hi[h] && in_sorted(g.excl_items, ex_lo[h], ex_hi[h], g.item_lo + it)) continue;
                        int ws = wslot[h];     // a local, so that the rescan does not index wslot[] by h
                        list_insert(ls + (h * K) * NT + tid, li + (h * K) * NT + tid, NT, 0, K, s, (int)it, ws, thr[h]);
                        wslot[h] = ws;
                    }
                }
            }
        }
    }
    const int64_t col = (int64_t)blockIdx.y * 4 + grp;
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (valid[h]) list_store(ls + (h * K) * NT, li + (h * K) * NT, NT, tid, K, col, g.U, q[h], g.part_s, g.part_i);
}

template <int DP>
int launch_scan_dp(const Layout &L, const ScanArgs &g, hipStream_t stream) {
    // raised once per instantiation, to the most any layout asks for
    if (L.lds > 64 * 1024) PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&dot_scan_kernel<DP>), kMaxScanLds));
    const int users_wg = kUW * L.NW;
    const dim3 grid((unsigned)((g.U + users_wg - 1) / users_wg), (unsigned)L.S);
    PEA_LAUNCH(dot_scan_kernel<DP>, grid, dim3(kWave * L.NW), L.lds, stream, g);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

int launch_scan(const Layout &L, const ScanArgs &g, hipStream_t stream) {
    if (L.DP == 32) return launch_scan_dp<32>(L, g, stream);
    if (L.DP == 64) return launch_scan_dp<64>(L, g, stream);
    if (L.DP == 128) return launch_scan_dp<128>(L, g, stream);
    return launch_scan_dp<256>(L, g, stream);
}

int check_d(const char *what, int D) {
    PEA_REQUIRE(D >= 4 && D % 4 == 0 && D <= 256, PEA_ERR_ARG, "%s: width %d must be a multiple of 4 in 4..256", what, D);
    return PEA_OK;
}

// ---------------------------------------------------------------------------------------------- the all-item rank
// pea_dot_rank_full_multi (include/peahip_eval.h) and pea_dot_rank_full: the rows, counters and finish of topk_select.h
// with dot_pair and the MFMA tiles of dot_tile_scores.
struct RankLayout {
    int DP = 32, S = 1, LD = 8, pc = kPC;
    int64_t span = 0, rows = 0;
    size_t off_thr = 0, off_part = 0, off_cnt = 0, bytes = 0, lds = 0;
};

constexpr int kMultiNW = 4;         // waves of one workgroup of the scan: 128 rows share an item tile (<= 34 KB of LDS)

// Depends on (U, Q, n_items, D) and on whether the call has a row pointer only: the rows are the bound multi_rows, not the
// rows in use.  The four lane groups of a row add their counters up in the wave, so an item range leaves one column.
// off_cnt: two [Q] counters for a caller of pea_dot_rank_full who passes no rank or no auc.
RankLayout make_rank_layout(int64_t U, int64_t Q, int64_t n_items, int D, bool row_pointer) {
    RankLayout L;
    L.DP = D <= 32 ? 32 : (D <= 64 ? 64 : (D <= 128 ? 128 : 256));
    L.LD = tile_ld(D);
    L.lds = (size_t)kTI * L.LD * 4;
    L.rows = multi_rows(U, Q, row_pointer);
    L.pc = multi_chunk(row_pointer);
    const int rows_wg = kUW * kMultiNW;
    catalogue_split(std::max<int64_t>((L.rows + rows_wg - 1) / rows_wg, 1), n_items, 1, kTI, &L.S, &L.span);
    size_t o = 256;                                                     // error flag
    L.off_thr = o;  o = align256(o + (size_t)std::max<int64_t>(Q, 1) * 4);
    L.off_part = o; o = align256(o + (size_t)L.S * 2 * L.pc * std::max<int64_t>(L.rows, 1) * 4);
    L.off_cnt = o;
    if (!row_pointer) o = align256(o + (size_t)std::max<int64_t>(Q, 1) * 8);
    L.bytes = o;
    return L;
}

struct MultiArgs {
    int64_t U, Q, rows, N, n_items, item_lo, span;
    int S, pc, D, LD;
    const float *repr;
    const int64_t *unids, *pos_rowptr, *pos_items, *excl_rowptr, *excl_items;
    float *thr;      // [Q] the positives' scores
    int *part;       // [S, 2, pc, rows] counts of (s > t), (s < t)
    int *err;
};

// one team (pos_team) per user: multi_thresholds with dot_pair; the one place the ids of the call are checked
__global__ __launch_bounds__(256) void dot_multi_pos_kernel(const MultiArgs g) {
    int64_t q;
    int lane, team;
    pos_team(g.pos_rowptr, q, lane, team);
    if (q >= g.U) return;
    const int64_t u = g.unids[q];
    const bool u_ok = u >= 0 && u < g.N;
    if (!u_ok && lane == 0) atomicOr(g.err, 1);
    multi_thresholds(q, g.Q, g.pos_rowptr, lane, team,
                     [&](int64_t j) {
                         const int64_t p = g.pos_items[j];
                         if (p < 0 || p >= g.N) {
                             atomicOr(g.err, 1);
                             return 0.f;
                         }
                         return u_ok ? dot_pair(g.repr + u * g.D, g.repr + p * g.D, g.D) : 0.f;
                     },
                     g.thr);
}

// dot_scan_kernel's tiles with a (user, chunk) row per (lane, half) column and multi_count in place of the lists: the
// same MFMA steps in the same order, so the same bits.  T = kPC serves a call with a row pointer: a wave whose rows all
// hold one threshold runs the chain at length 1; a workgroup of idle rows leaves at once.  T = 1 serves a call without
// one, where every row holds one threshold: no room for eight, which is a wave per SIMD more at D <= 128.
template <int DP, int T>
__global__ __launch_bounds__(256) void dot_multi_scan_kernel(const MultiArgs g) {
    const int NT = blockDim.x;
    float *tile = dot_smem;
    const int tid = threadIdx.x;
    const int lane = tid % kWave, n = lane & 15, grp = lane >> 4;
    const int D = g.D;
    const int64_t r0 = ((int64_t)blockIdx.x * (NT / kWave) + tid / kWave) * kUW + n;
    int64_t r[2];
    int cnt[2];
    float ub[2][DP / 4];
    float thr[2][T];
    int hi[2][T], lo[2][T];
    int64_t first[2];
    int64_t node[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        r[h] = r0 + 16 * h;
        int64_t q = 0;
        first[h] = 0;
        cnt[h] = 0;
        if (r[h] < g.rows) multi_row(r[h], g.U, g.Q, g.pos_rowptr, q, first[h], cnt[h]);
        node[h] = g.unids[q];
        if (node[h] < 0 || node[h] >= g.N) node[h] = 0;        // reported by dot_multi_pos_kernel
    }
    if (!__syncthreads_or(cnt[0] > 0 || cnt[1] > 0)) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // an idle column rides along in the MFMA on user 0's row; its counters are never stored
        const float *row = g.repr + node[h] * D + grp;
#pragma unroll
        for (int t = 0; t < DP / 4; ++t) ub[h][t] = 4 * t < D ? row[4 * t] : 0.f;
#pragma unroll
        for (int k = 0; k < T; ++k) {
            thr[h][k] = k < cnt[h] ? g.thr[first[h] + k] : 0.f;
            hi[h][k] = lo[h][k] = 0;
        }
    }
    const bool one = T == 1 || __ballot(cnt[0] > 1 || cnt[1] > 1) == 0;
    const int64_t i0 = (int64_t)blockIdx.y * g.span;
    const int64_t i1 = i0 + g.span < g.n_items ? i0 + g.span : g.n_items;
    for (int64_t t0 = i0; t0 < i1; t0 += kTI) {
        f32x4 acc[2][2];
        dot_tile_scores<DP>(g.repr, g.item_lo, t0, i1, D, g.LD, tile, ub, acc);
#pragma unroll
        for (int is = 0; is < 2; ++is) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t it = t0 + 16 * is + 4 * grp + j;
                if (it >= i1) continue;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (one) multi_count<1>(acc[is][h][j], thr[h], hi[h], lo[h]);
                    else multi_count<T>(acc[is][h][j], thr[h], hi[h], lo[h]);
                }
            }
        }
    }
    // the four lane groups of a column each saw a quarter of the items: integer sums, any order gives the same
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int k = 0; k < T; ++k) {
            hi[h][k] += __shfl_xor(hi[h][k], 16);
            hi[h][k] += __shfl_xor(hi[h][k], 32);
            lo[h][k] += __shfl_xor(lo[h][k], 16);
            lo[h][k] += __shfl_xor(lo[h][k], 32);
        }
        if (grp == 0 && cnt[h] > 0) multi_store(g.part, blockIdx.y, g.pc, g.rows, r[h], cnt[h], hi[h], lo[h]);
    }
}

// one wave per user: rank_multi_finish of topk_select.h with dot_pair (the bits the scan compared)
__global__ __launch_bounds__(256) void dot_multi_finish_kernel(const MultiArgs g, const RankOut out) {
    const int lane = threadIdx.x % kWave;
    const int64_t q = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (q >= g.U) return;
    int64_t u = g.unids[q];
    if (u < 0 || u >= g.N) u = 0;        // reported by dot_multi_pos_kernel
    rank_multi_finish(q, g.U, g.Q, g.rows, g.pc, g.S, g.n_items, g.item_lo, g.pos_rowptr, g.pos_items, g.thr, g.excl_rowptr,
                      g.excl_items, g.part, [&](int64_t node) { return dot_pair(g.repr + u * g.D, g.repr + node * g.D, g.D); },
                      lane, out);
}

// one thread per user: rank_finish of topk_select.h, for a call without a row pointer over very many users (its part is
// [S, 2, U], the columns rank_finish sums)
__global__ __launch_bounds__(64) void dot_one_finish_kernel(const MultiArgs g, const RankOut out) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= g.U) return;
    int64_t u = g.unids[q];
    if (u < 0 || u >= g.N) u = 0;        // reported by dot_multi_pos_kernel
    rank_finish(q, g.U, g.S, g.n_items, g.item_lo, g.thr[q], g.pos_items[q], g.excl_rowptr, g.excl_items, g.part,
                [&](int64_t node) { return dot_pair(g.repr + u * g.D, g.repr + node * g.D, g.D); }, out.above, out.auc,
                out.pos_score);
}

template <int DP>
int launch_multi_scan(const RankLayout &L, const MultiArgs &g, hipStream_t stream) {
    const int rows_wg = kUW * kMultiNW;
    const dim3 grid((unsigned)((g.rows + rows_wg - 1) / rows_wg), (unsigned)L.S);
    if (g.pos_rowptr) {
        PEA_LAUNCH((dot_multi_scan_kernel<DP, kPC>), grid, dim3(kWave * kMultiNW), L.lds, stream, g);
    } else {
        PEA_LAUNCH((dot_multi_scan_kernel<DP, 1>), grid, dim3(kWave * kMultiNW), L.lds, stream, g);
    }
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

// the body of both rank entry points, once their arguments are checked; pos_rowptr null: one positive per user, Q = U
int rank_call(const char *what, const RankLayout &L, int64_t U, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
              const int64_t *pos_rowptr, const int64_t *pos_items, int64_t Q, int64_t item_lo, int64_t n_items,
              const int64_t *excl_rowptr, const int64_t *excl_items, const RankOut &out, char *ws, hipStream_t stream) {
    PEA_MEMSET_ASYNC((int *)ws, 0, sizeof(int), stream);
    MultiArgs g;
    g.U = U; g.Q = Q; g.rows = L.rows; g.N = num_nodes; g.n_items = n_items; g.item_lo = item_lo; g.span = L.span;
    g.S = L.S; g.pc = L.pc; g.D = D; g.LD = L.LD;
    g.repr = repr; g.unids = unids; g.pos_rowptr = pos_rowptr; g.pos_items = pos_items;
    g.excl_rowptr = excl_rowptr; g.excl_items = excl_items;
    g.thr = (float *)(ws + L.off_thr);
    g.part = (int *)(ws + L.off_part);
    g.err = (int *)ws;
    const dim3 waves((unsigned)((U + 3) / 4));
    {
        ProfScope ps("dot_rank_multi_pos", stream, (double)Q * (8.0 * D + 20.0));
        PEA_LAUNCH(dot_multi_pos_kernel, dim3(pos_blocks(U, pos_rowptr != nullptr)), dim3(256), 0, stream, g);
        PEA_HIP(hipGetLastError());
    }
    if (Q > 0) {
        ProfScope ps("dot_rank_multi_scan", stream, (double)L.rows * (double)n_items * (2.0 * D + 4.0 * L.pc));
        if (L.DP == 32) PEA_TRY(launch_multi_scan<32>(L, g, stream));
        else if (L.DP == 64) PEA_TRY(launch_multi_scan<64>(L, g, stream));
        else if (L.DP == 128) PEA_TRY(launch_multi_scan<128>(L, g, stream));
        else PEA_TRY(launch_multi_scan<256>(L, g, stream));
    }
    {
        ProfScope ps("dot_rank_multi_finish", stream, 8.0 * (double)Q * L.S);
        if (!pos_rowptr && U >= kThreadFinishUsers) {
            PEA_LAUNCH(dot_one_finish_kernel, dim3((unsigned)((U + 63) / 64)), dim3(64), 0, stream, g, out);
        } else {
            PEA_LAUNCH(dot_multi_finish_kernel, waves, dim3(256), 0, stream, g, out);
        }
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag((int *)ws, stream, what);
}

}  // namespace
}  // namespace pea

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int pea_dot_predict(int64_t B, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                               const int64_t *inids, float *pred, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_d("dot_predict", D));
    PEA_REQUIRE(B >= 0 && repr && unids && inids && pred, PEA_ERR_ARG, "dot_predict: bad argument");
    if (B == 0) return PEA_OK;
    int *err = err_flag_for_current_device();
    PEA_REQUIRE(err != nullptr, PEA_ERR_HIP, "dot_predict: no error-flag buffer on this device");
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    {
        ProfScope ps("dot_predict", stream, (double)B * (8.0 * D + 20.0));
        PEA_LAUNCH(dot_predict_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, D, num_nodes, repr, unids,
                   inids, pred, err);
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag(err, stream, "dot_predict");
}

extern "C" int pea_dot_rank_eval(int64_t U, int C, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                                 const int64_t *cand, float *scores, int32_t *rank, float *auc, float *loss,
                                 void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_d("dot_rank_eval", D));
    PEA_REQUIRE(U >= 0 && C >= 2 && repr && unids && cand, PEA_ERR_ARG, "dot_rank_eval: bad argument");
    if (U == 0) return PEA_OK;
    int *err = err_flag_for_current_device();
    PEA_REQUIRE(err != nullptr, PEA_ERR_HIP, "dot_rank_eval: no error-flag buffer on this device");
    PEA_MEMSET_ASYNC(err, 0, sizeof(int), stream);
    {
        ProfScope ps("dot_rank_eval", stream, (double)U * C * (4.0 * D + 12.0));
        PEA_LAUNCH(dot_rank_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, stream, U, C, D, num_nodes, repr, unids, cand,
                   scores, rank, auc, loss, err);
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag(err, stream, "dot_rank_eval");
}

// K = 1 sizes the workspace of pea_dot_rank_full as well (include/peahip.h)
extern "C" size_t pea_dot_topk_workspace_bytes(int64_t U, int64_t n_items, int K, int D) {
    if (U < 0 || n_items < 0 || K < 1 || K > 128 || D < 4 || D > 256 || D % 4 != 0) return 0;
    const size_t bytes = pea::make_layout(U, n_items, K, D).bytes;
    return K == 1 ? std::max(bytes, pea::make_rank_layout(U, U, n_items, D, false).bytes) : bytes;
}

extern "C" int pea_dot_recommend_topk(int64_t U, int K, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                                      int64_t item_lo, int64_t n_items, const int64_t *excl_rowptr,
                                      const int64_t *excl_items, int64_t *out_items, float *out_scores, void *workspace,
                                      size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_REQUIRE(K >= 1 && K <= 128, PEA_ERR_ARG, "dot_recommend_topk: K=%d (1..128)", K);
    PEA_TRY(check_d("dot_recommend_topk", D));
    PEA_TRY(check_catalogue("dot_recommend_topk", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(repr && unids && out_items && out_scores && workspace, PEA_ERR_ARG, "dot_recommend_topk: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "dot_recommend_topk: excl_rowptr without excl_items");
    const Layout L = make_layout(U, n_items, K, D);
    PEA_REQUIRE(workspace_bytes >= L.bytes, PEA_ERR_NOMEM, "dot_recommend_topk: workspace too small (%zu < %zu)",
                workspace_bytes, L.bytes);
    if (U == 0) return PEA_OK;
    char *ws = (char *)workspace;
    PEA_MEMSET_ASYNC((int *)ws, 0, sizeof(int), stream);
    const int cols = L.S * 4;
    ScanArgs g;
    g.U = U; g.N = num_nodes; g.n_items = n_items; g.item_lo = item_lo; g.span = L.span;
    g.K = K; g.D = D; g.LD = L.LD;
    g.repr = repr; g.unids = unids;
    g.excl_rowptr = excl_rowptr; g.excl_items = excl_items;
    g.part_s = (float *)(ws + L.off_part);
    g.part_i = (int *)(ws + L.off_part + (size_t)cols * K * U * 4);
    g.err = (int *)ws;
    {
        ProfScope ps("dot_topk_scan", stream, 2.0 * (double)U * (double)n_items * D);
        PEA_TRY(launch_scan(L, g, stream));
    }
    {
        ProfScope ps("dot_topk_merge", stream, 8.0 * (double)U * K * (cols + 1.5));
        int p2 = 2;
        while (p2 < cols * K) p2 <<= 1;      // <= kMaxMerge: make_layout keeps 4 S K <= 2048
        PEA_LAUNCH(topk_merge_kernel, dim3((unsigned)U), dim3(p2 <= 128 ? 64 : 256), 0, stream, U, K, cols, p2, item_lo,
                   (const float *)g.part_s, (const int *)g.part_i, out_items, out_scores);
        PEA_HIP(hipGetLastError());
    }
    return read_err_flag((int *)ws, stream, "dot_recommend_topk");
}

extern "C" int pea_dot_rank_full(int64_t U, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                                 const int64_t *pos_items, int64_t item_lo, int64_t n_items, const int64_t *excl_rowptr,
                                 const int64_t *excl_items, int32_t *rank, float *auc, float *pos_score, void *workspace,
                                 size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_d("dot_rank_full", D));
    PEA_TRY(check_catalogue("dot_rank_full", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(repr && unids && pos_items && workspace, PEA_ERR_ARG, "dot_rank_full: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "dot_rank_full: excl_rowptr without excl_items");
    const RankLayout L = make_rank_layout(U, U, n_items, D, false);
    const size_t need = pea_dot_topk_workspace_bytes(U, n_items, 1, D);
    PEA_REQUIRE(workspace_bytes >= need, PEA_ERR_NOMEM, "dot_rank_full: workspace too small (%zu < %zu)", workspace_bytes, need);
    if (U == 0) return PEA_OK;
    char *ws = (char *)workspace;
    int32_t *cnt = (int32_t *)(ws + L.off_cnt);
    const RankOut out = {rank ? rank : cnt, cnt + U, pos_score, nullptr, auc};
    return rank_call("dot_rank_full", L, U, D, num_nodes, repr, unids, nullptr, pos_items, U, item_lo, n_items, excl_rowptr,
                     excl_items, out, ws, stream);
}

// include/peahip_eval.h
extern "C" size_t pea_dot_rank_multi_workspace_bytes(int64_t U, int64_t Q, int64_t n_items, int D) {
    if (U < 0 || Q < 0 || n_items < 0 || n_items >= ((int64_t)1 << 31) - 1 || D < 4 || D > 256 || D % 4 != 0) return 0;
    return pea::make_rank_layout(U, Q, n_items, D, true).bytes;
}

extern "C" int pea_dot_rank_full_multi(int64_t U, int D, int64_t num_nodes, const float *repr, const int64_t *unids,
                                       const int64_t *pos_rowptr, const int64_t *pos_items, int64_t Q, int64_t item_lo,
                                       int64_t n_items, const int64_t *excl_rowptr, const int64_t *excl_items, int32_t *above,
                                       int32_t *below, float *pos_score, int32_t *n_neg, void *workspace,
                                       size_t workspace_bytes, void *stream_) {
    using namespace pea;
    hipStream_t stream = (hipStream_t)stream_;
    PEA_TRY(check_d("dot_rank_full_multi", D));
    PEA_TRY(check_catalogue("dot_rank_full_multi", U, num_nodes, item_lo, n_items));
    PEA_REQUIRE(Q >= 0, PEA_ERR_ARG, "dot_rank_full_multi: Q=%lld", (long long)Q);
    PEA_REQUIRE(repr && unids && pos_rowptr && pos_items && above && below && pos_score && n_neg && workspace, PEA_ERR_ARG,
                "dot_rank_full_multi: null pointer");
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "dot_rank_full_multi: excl_rowptr without excl_items");
    const RankLayout L = make_rank_layout(U, Q, n_items, D, true);
    PEA_REQUIRE(workspace_bytes >= L.bytes, PEA_ERR_NOMEM, "dot_rank_full_multi: workspace too small (%zu < %zu)",
                workspace_bytes, L.bytes);
    if (U == 0) return PEA_OK;
    const RankOut out = {above, below, pos_score, n_neg, nullptr};
    return rank_call("dot_rank_full_multi", L, U, D, num_nodes, repr, unids, pos_rowptr, pos_items, Q, item_lo, n_items,
                     excl_rowptr, excl_items, out, (char *)workspace, stream);
}
