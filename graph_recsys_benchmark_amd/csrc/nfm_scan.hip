// The full-catalogue scan over the NFM fold for gfx950 (include/peahip_fm_eval.h): top-K recommendation, the all-item rank
// and the all-item rank with several positives per user, without the [users, items] logit matrix.
//
// A workgroup (kThreads threads, 4 waves) owns kUB = 8 users and one item range of catalogue_split (topk_select.h).  It
// keeps the image of W' and its users' embedding rows in LDS for its whole life, stages a tile of 64 consecutive item rows
// (consecutive catalogue items are consecutive table rows: a coalesced load) with their linear terms ONCE, and reuses it
// for each of its users in turn: x = e_u (.) e_i from LDS to LDS, the tile body of nfm_tile.h -- the one nfm_score_kernel
// calls, so a pair's logit has the scorer's bits --, then wave 0 selects from the 64 logits its lanes hold while the other
// waves form the next user's x.  Item-row traffic per pair falls by kUB; per (user, tile) there are two barriers.
//   top-K   one K-entry list per (user, range) in LDS (sentinel (-inf, kEmpty) and worst-entry rule of topk_select.h).  The
//           wave ballots y > threshold; the survivors, in ascending item order, are looked up in the user's exclusion row
//           (in_sorted) and replace the worst entry, which the wave finds again in parallel.  The columns go through
//           topk_merge_kernel unchanged: S K <= kMaxMerge.
//   rank    the thresholds are the positives' logits, scored first by nfm_thr_kernel through the same tile body.  What is no
//           negative is taken out IN the scan: a user's exclusion row and positive row ascend and so do the tiles, so a cursor
//           per row walks along; at each tile the next 64 entries of either row are read (coalesced) and those inside the
//           tile mark their lanes.  The wave counts y > t and y < t over the unmarked lanes by ballot and popcount, looping over
//           the user's thresholds: the first 64 have their counters in LDS, a longer row's tail adds into the (zeroed)
//           workspace, which only this workgroup touches.  The marked lanes are counted for n_neg.
// pea_nfm_rank_full is the multi call with one positive per user.  The only atomic is the atomicOr on the error flag; every
// grid and split is a function of the arguments; sums are integers.
#include <algorithm>

#include "../../include/peahip_fm.h"
#include "../../include/peahip_fm_eval.h"
#include "nfm_tile.h"
#include "topk_select.h"

namespace pea {
namespace {

constexpr int kUB = PEA_NFM_SCAN_USERS;
constexpr int kHead = kWave;                  // thresholds of a user whose counters live in LDS
constexpr int kThrMaxWg = 1024;
constexpr int kNone = kSP;                    // mark of a row entry that lies past the tile

// floats ahead of the per-user state: W', the item tile, x, the waves' partials, the users' rows, the tile's linear terms
size_t scan_float_words(int E, int H) {
    const int ep = ceil16(E), hp = ceil16(H), ld = ep + 4;
    return (size_t)hp * ld + 2 * (size_t)kSP * ld + kWaves * kSP + (size_t)kUB * ld + kSP;
}
// per user: 6 int64 (row, the two cursors and ends, the positives' base), 6 words (ok, lin, gone, threshold, worst slot, P)
constexpr size_t kUserState = 6 * 8 + 6 * 4;
size_t scan_lds_bytes(int E, int H, int K) {
    const size_t sel = K > 0 ? (size_t)kUB * K * 8 : (size_t)kUB * kHead * 5 * 4;
    return sizeof(float) * scan_float_words(E, H) + kUB * kUserState + sel;
}
size_t thr_lds_bytes(int E, int H) {
    const int ep = ceil16(E), hp = ceil16(H), ld = ep + 4;
    return sizeof(float) * ((size_t)hp * ld + (size_t)kSP * ld + kWaves * kSP) + 2 * kSP * 8 + kSP * 4;
}

bool scan_supported(int E, int H, int K) {
    return pea_nfm_supported(E, H) && K >= 0 && K <= 128 && scan_lds_bytes(E, H, K) <= kLdsBudget && thr_lds_bytes(E, H) <= kLdsBudget;
}

int64_t user_blocks(int64_t n_users) { return std::max<int64_t>((n_users + kUB - 1) / kUB, 1); }

// the most item ranges any K gives a catalogue of n_items
int64_t split_cap(int64_t n_items) { return std::min<int64_t>(kMaxSplits, std::max<int64_t>(n_items / 512, 1)); }

// Workspace [256 (unused head) | top-K columns: scores, indices | thr [Q] | counters [S, 2, Q] | gone [S, n_users]].  The
// parts are sized by bounds on S that do not fall when an argument grows (S itself does, with more users), so the query is
// non-decreasing: S <= split_cap, S K <= kMaxMerge, and S user_blocks <= 1024 + user_blocks.
struct WsLayout {
    int S = 1;
    int64_t span = 0;
    size_t off_s = 0, off_i = 0, off_thr = 0, off_cnt = 0, off_gone = 0, cnt_bytes = 0, total = 0;
};
WsLayout ws_layout(int64_t n_users, int64_t Q, int64_t n_items, int K) {
    WsLayout l;
    catalogue_split(user_blocks(n_users), n_items, std::max(K, 1), kSP, &l.S, &l.span);
    const size_t nu = (size_t)std::max<int64_t>(n_users, 1), cap = (size_t)split_cap(n_items);
    const size_t cols_users = std::min(nu * cap, (size_t)kUB * (1024 + (size_t)user_blocks(n_users)));
    const size_t entries = std::min(nu * std::min<size_t>(cap * K, kMaxMerge), cols_users * K);
    size_t at = 256;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += align256(bytes);
        return here;
    };
    l.off_s = take(entries * 4);
    l.off_i = take(entries * 4);
    l.off_thr = take((size_t)Q * 4);
    l.cnt_bytes = (size_t)l.S * 2 * Q * 4;
    l.off_cnt = take(cap * 2 * Q * 4);
    l.off_gone = take(cols_users * 4);
    l.total = at;
    return l;
}

struct ScArgs {
    int64_t n_users, Q, U, I, ld_emb, item_lo, n_items, node0, span;
    int K, E, H, EP, HP, LD;
    const float *emb, *lin, *wf, *bf, *w2, *bias;
    const int64_t *uid, *pos_rowptr, *pos_items, *excl_rowptr, *excl_items;
    float *thr;              // [Q] the positives' logits
    float *part_s;           // top-K: [S, K, n_users]
    int *part_i;
    int *cnt;                // rank: [S, 2, Q] counts of (y > t), (y < t)
    int *gone;               // rank: [S, n_users] catalogue items of the range that are no negative
    int *err;
};

extern __shared__ __attribute__((aligned(16))) float sc_smem[];

// the first position of the ascending row[b, e) whose entry is >= node
__device__ __forceinline__ int64_t lower_bound(const int64_t *__restrict__ row, int64_t b, int64_t e, int64_t node) {
    while (b < e) {
        const int64_t mid = b + ((e - b) >> 1);
        if (row[mid] < node) b = mid + 1; else e = mid;
    }
    return b;
}

// entry cur + l of a row against the tile that starts at node t0: its lane, -1 if it lies before the tile (consumed all the
// same), kNone if it lies past it or past the row's end
__device__ __forceinline__ int tile_mark(const int64_t *__restrict__ row, int64_t cur, int64_t end, int l, int64_t t0) {
    if (cur + l >= end) return kNone;
    const int64_t rel = row[cur + l] - t0;
    return rel >= kSP ? kNone : (rel < 0 ? -1 : (int)rel);
}

// the lanes that the marks of one row name, and how many entries the tile consumed
__device__ __forceinline__ unsigned long long marked_lanes(int mark, int &consumed) {
    unsigned long long in = __ballot(mark < kNone), lanes = 0;
    consumed = __popcll(in);
    for (; in != 0; in &= in - 1) {
        const int r = __shfl(mark, __ffsll((long long)in) - 1);
        if (r >= 0) lanes |= 1ull << r;
    }
    return lanes;
}

// `live` lanes' y against the n thresholds the lanes 0 .. n-1 hold: lane j leaves with the two counts of threshold j
__device__ __forceinline__ void count_against(float y, bool live, float t_lane, int n, int lane, int &hi, int &lo) {
    hi = lo = 0;
    for (int j = 0; j < n; ++j) {
        const float t = __shfl(t_lane, j);
        const int ch = __popcll(__ballot(live && y > t)), cl = __popcll(__ballot(live && y < t));
        if (lane == j) {
            hi = ch;
            lo = cl;
        }
    }
}

template <bool RANK>
__global__ __launch_bounds__(kThreads) void nfm_scan_kernel(const ScArgs a) {
    const int LD = a.LD, E = a.E, H = a.H, e4 = E / 4, K = a.K;
    float *Ws = sc_smem;                                   // [HP][LD] W'
    float *It = Ws + (size_t)a.HP * LD;                    // [64][LD] the tile's item rows
    float *Xt = It + kSP * LD;                             // [64][LD] x of the current user
    float *part = Xt + kSP * LD;                           // [4 waves][64]
    float *Ut = part + kWaves * kSP;                       // [kUB][LD] the users' rows
    float *Il = Ut + kUB * LD;                             // [64] lin of the tile's items
    int64_t *urow = reinterpret_cast<int64_t *>(Il + kSP); // [kUB] each: 16-byte aligned, every part above is whole float4s
    int64_t *ex_b = urow + kUB, *ex_e = ex_b + kUB;        // the exclusion row: [cursor (RANK) or begin, end)
    int64_t *ps_b = ex_e + kUB, *ps_e = ps_b + kUB;        // RANK: the positive row's cursor and end
    int64_t *pbase = ps_e + kUB;                           // RANK: flat index of the user's first positive
    int *uok = reinterpret_cast<int *>(pbase + kUB);
    float *ulin = reinterpret_cast<float *>(uok + kUB);
    int *gone = reinterpret_cast<int *>(ulin + kUB);
    float *lthr = reinterpret_cast<float *>(gone + kUB);   // top-K: the worst entry's score
    int *lws = reinterpret_cast<int *>(lthr + kUB);        // top-K: its slot
    int *np = lws + kUB;                                   // RANK: positives of the user
    float *sel = reinterpret_cast<float *>(np + kUB);
    float *cs = sel;                                       // top-K: [kUB][K] scores, [kUB][K] indices
    int *ci = reinterpret_cast<int *>(cs + kUB * K);
    float *thrL = sel;                                     // RANK: [kUB][kHead] thresholds, counters (hi, lo), marks (excl, pos)
    int *chi = reinterpret_cast<int *>(thrL + kUB * kHead), *clo = chi + kUB * kHead;
    int *exl = clo + kUB * kHead, *pxl = exl + kUB * kHead;

    const int tid = threadIdx.x, lane = tid % kWave;
    const int64_t q0 = (int64_t)blockIdx.x * kUB;
    const int64_t i0 = (int64_t)blockIdx.y * a.span;
    const int64_t i1 = i0 + a.span < a.n_items ? i0 + a.span : a.n_items;
    const int64_t cat_node0 = a.node0 + a.item_lo;         // node id of catalogue index 0
    const float bias = a.bias[0];

    stage_weight<4>(a.wf, H, E, 0, Ws, a.HP, a.EP, LD);
    if (tid < kUB) {
        const int64_t q = q0 + tid;
        bool ok = q < a.n_users;
        int64_t u = 0;
        if (ok) {
            u = a.uid[q];
            if (u < 0 || u >= a.U) {
                atomicOr(a.err, 1);
                ok = false;
                u = 0;
            }
        }
        uok[tid] = ok ? 1 : 0;
        urow[tid] = u;
        ulin[tid] = ok ? a.lin[u] : 0.f;
        gone[tid] = 0;
        lthr[tid] = -INFINITY;
        lws[tid] = 0;
        int64_t eb = 0, ee = 0, pb = 0, pe = 0;
        if (ok && a.excl_rowptr) {
            eb = a.excl_rowptr[q];
            ee = a.excl_rowptr[q + 1];
            if (ee < eb) ee = eb;
        }
        if (RANK && ok) {
            pos_span(a.pos_rowptr, q, a.Q, pb, pe);
            pbase[tid] = pb;
            np[tid] = pe - pb < 0x7fffffff ? (int)(pe - pb) : 0x7fffffff;
            eb = lower_bound(a.excl_items, eb, ee, cat_node0 + i0);
            pb = lower_bound(a.pos_items, pb, pe, cat_node0 + i0);
        } else {
            pbase[tid] = 0;
            np[tid] = 0;
        }
        ex_b[tid] = eb;
        ex_e[tid] = ee;
        ps_b[tid] = pb;
        ps_e[tid] = pe;
    }
    __syncthreads();
    for (int i = tid; i < kUB * e4; i += kThreads) {
        const int u = i / e4, c = 4 * (i - u * e4);
        st4(Ut + u * LD + c, uok[u] ? ld4(a.emb + urow[u] * a.ld_emb + c) : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    if (RANK) {
        for (int i = tid; i < kUB * kHead; i += kThreads) {
            const int u = i / kHead, l = i - u * kHead;
            chi[i] = clo[i] = 0;
            thrL[i] = l < np[u] ? a.thr[pbase[u] + l] : 0.f;
        }
    } else {
        for (int i = tid; i < kUB * K; i += kThreads) {
            cs[i] = -INFINITY;
            ci[i] = kEmpty;
        }
    }

    for (int64_t t0 = i0; t0 < i1; t0 += kSP) {
        __syncthreads();                       // the last user's selection is over: the tile and the cursors may move
        // rows past the end of the range are zero rows: their logits are computed and never looked at
        for (int i = tid; i < kSP * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            st4(It + rr * LD + c,
                t0 + rr < i1 ? ld4(a.emb + (a.U + a.item_lo + t0 + rr) * a.ld_emb + c) : make_float4(0.f, 0.f, 0.f, 0.f));
        }
        if (tid < kSP) Il[tid] = t0 + tid < i1 ? a.lin[a.U + a.item_lo + t0 + tid] : 0.f;
        if (RANK) {
            for (int i = tid; i < kUB * kSP; i += kThreads) {
                const int u = i / kSP, l = i - u * kSP;
                exl[i] = uok[u] ? tile_mark(a.excl_items, ex_b[u], ex_e[u], l, cat_node0 + t0) : kNone;
                pxl[i] = uok[u] ? tile_mark(a.pos_items, ps_b[u], ps_e[u], l, cat_node0 + t0) : kNone;
            }
        }
        __syncthreads();
        for (int u = 0; u < kUB; ++u) {
            if (!uok[u]) continue;             // the same for every thread: the barriers below stay matched
            for (int i = tid; i < kSP * e4; i += kThreads) {
                const int rr = i / e4, c = 4 * (i - rr * e4);
                st4(Xt + rr * LD + c, nfm_x4(ld4(Ut + u * LD + c), ld4(It + rr * LD + c)));
            }
            __syncthreads();
            const float d = nfm_tile_dots(Ws, Xt, part, a.bf, a.w2, H, a.HP, LD, e4);
            if (tid >= kSP) continue;          // wave 0 selects; the others go on to the next user's x
            const bool live = t0 + lane < i1;
            const float y = nfm_logit(ulin[u], Il[lane], bias, d);
            if (RANK) {
                int used_e, used_p;
                const unsigned long long out = marked_lanes(exl[u * kSP + lane], used_e) | marked_lanes(pxl[u * kSP + lane], used_p);
                const bool neg = live && ((out >> lane) & 1ull) == 0;
                const int taken = __popcll(out & __ballot(live));
                const int P = np[u];
                int hi, lo;
                count_against(y, neg, thrL[u * kHead + lane], P < kHead ? P : kHead, lane, hi, lo);
                chi[u * kHead + lane] += hi;
                clo[u * kHead + lane] += lo;
                for (int jb = kHead; jb < P; jb += kHead) {            // the tail of a long positive row
                    const int n = P - jb < kHead ? P - jb : kHead;
                    const int64_t j = pbase[u] + jb + lane;
                    count_against(y, neg, lane < n ? a.thr[j] : 0.f, n, lane, hi, lo);
                    if (lane < n) {
                        a.cnt[((int64_t)blockIdx.y * 2) * a.Q + j] += hi;
                        a.cnt[((int64_t)blockIdx.y * 2 + 1) * a.Q + j] += lo;
                    }
                }
                // every lane writes the same values: the wave reads them back at the next tile
                gone[u] += taken;
                ex_b[u] += used_e;
                ps_b[u] += used_p;
            } else {
                float thr = lthr[u];
                unsigned long long m = __ballot(live && y > thr);
                if (m == 0) continue;
                int ws = lws[u];
                const int64_t eb = ex_b[u], ee = ex_e[u];
                float *us = cs + u * K;
                int *ui = ci + u * K;
                for (; m != 0; m &= m - 1) {
                    const int l = __ffsll((long long)m) - 1;
                    const float s = __shfl(y, l);
                    if (!(s > thr)) continue;
                    const int idx = (int)(t0 + l);
                    if (eb < ee && in_sorted(a.excl_items, eb, ee, cat_node0 + idx)) continue;
                    us[ws] = s;                // every lane stores the same entry and then reads its own share of the list
                    ui[ws] = idx;
                    // the new worst: lowest score, highest index among equals, lowest slot among the empty entries
                    float w = INFINITY;
                    int wi = -1, wsl = 0;
                    for (int j = lane; j < K; j += kWave) {
                        const float sc = us[j];
                        const int id = ui[j];
                        if (sc < w || (sc == w && id > wi)) {
                            w = sc;
                            wi = id;
                            wsl = j;
                        }
                    }
                    for (int off = kWave / 2; off > 0; off >>= 1) {
                        const float ow = __shfl_xor(w, off);
                        const int oi = __shfl_xor(wi, off), osl = __shfl_xor(wsl, off);
                        if (ow < w || (ow == w && (oi > wi || (oi == wi && osl < wsl)))) {
                            w = ow;
                            wi = oi;
                            wsl = osl;
                        }
                    }
                    ws = wsl;
                    thr = w;
                }
                lthr[u] = thr;
                lws[u] = ws;
            }
        }
    }
    __syncthreads();
    if (RANK) {
        for (int i = tid; i < kUB * kHead; i += kThreads) {
            const int u = i / kHead, l = i - u * kHead;
            if (!uok[u] || l >= np[u]) continue;
            a.cnt[((int64_t)blockIdx.y * 2) * a.Q + pbase[u] + l] = chi[i];
            a.cnt[((int64_t)blockIdx.y * 2 + 1) * a.Q + pbase[u] + l] = clo[i];
        }
        if (tid < kUB && q0 + tid < a.n_users) a.gone[(int64_t)blockIdx.y * a.n_users + q0 + tid] = gone[tid];
    } else {
        for (int i = tid; i < kUB * K; i += kThreads) {
            const int u = i / K, j = i - u * K;
            const int64_t q = q0 + u;
            if (q >= a.n_users) continue;
            const int64_t o = ((int64_t)blockIdx.y * K + j) * a.n_users + q;
            a.part_s[o] = cs[i];
            a.part_i[o] = ci[i];
        }
    }
}

// The thresholds: the logits of the Q flat positives, 64 to a tile, through the tile body the scan calls.  The owner of
// flat positive j is the last user whose row starts at or before j.  A positive outside the table's items sets the flag.
__global__ __launch_bounds__(kThreads) void nfm_thr_kernel(const ScArgs a) {
    const int LD = a.LD, E = a.E, H = a.H, e4 = E / 4;
    float *Ws = sc_smem;
    float *Xt = Ws + (size_t)a.HP * LD;
    float *part = Xt + kSP * LD;
    int64_t *ids = reinterpret_cast<int64_t *>(part + kWaves * kSP);
    int *valid = reinterpret_cast<int *>(ids + 2 * kSP);
    const int64_t n_tiles = (a.Q + kSP - 1) / kSP;
    stage_weight<4>(a.wf, H, E, 0, Ws, a.HP, a.EP, LD);
    for (int64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < kSP) {
            const int64_t j = T * kSP + threadIdx.x;
            int64_t u = 0, it = 0;
            bool ok = j < a.Q;
            if (ok) {
                int64_t q = j;
                if (a.pos_rowptr) {
                    int64_t lo = 0, hi = a.n_users;
                    while (lo < hi) {
                        const int64_t mid = lo + ((hi - lo) >> 1);
                        if (a.pos_rowptr[mid] <= j) lo = mid + 1; else hi = mid;
                    }
                    q = lo - 1;
                }
                ok = q >= 0 && q < a.n_users;
                if (ok) {
                    u = a.uid[q];
                    ok = u >= 0 && u < a.U;               // reported by the scan
                    it = a.pos_items[j] - a.node0;
                    if (it < 0 || it >= a.I) {
                        atomicOr(a.err, 1);
                        ok = false;
                    }
                }
            }
            valid[threadIdx.x] = ok ? 1 : 0;
            ids[threadIdx.x] = ok ? u : 0;
            ids[kSP + threadIdx.x] = ok ? a.U + it : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kSP * e4; i += kThreads) {
            const int rr = i / e4, c = 4 * (i - rr * e4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid[rr]) v = nfm_x4(ld4(a.emb + ids[rr] * a.ld_emb + c), ld4(a.emb + ids[kSP + rr] * a.ld_emb + c));
            st4(Xt + rr * LD + c, v);
        }
        __syncthreads();
        const float d = nfm_tile_dots(Ws, Xt, part, a.bf, a.w2, H, a.HP, LD, e4);
        if (threadIdx.x < kSP) {
            const int64_t j = T * kSP + threadIdx.x;
            if (j < a.Q)
                a.thr[j] = valid[threadIdx.x] ? nfm_logit(a.lin[ids[threadIdx.x]], a.lin[ids[kSP + threadIdx.x]], a.bias[0], d) : 0.f;
        }
    }
}

// One wave per user: the ranges' counters summed in range order.  auc given: the single-positive outputs (above is rank).
__global__ __launch_bounds__(256) void nfm_rank_finish_kernel(const ScArgs a, int S, int32_t *above, int32_t *below, float *pos_score,
                                                              int32_t *n_neg, float *auc) {
    const int lane = threadIdx.x % kWave;
    const int64_t q = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
    if (q >= a.n_users) return;
    const int64_t u = a.uid[q];
    const bool ok = u >= 0 && u < a.U;
    int64_t b, e;
    pos_span(a.pos_rowptr, q, a.Q, b, e);
    int64_t taken = 0;
    for (int c = 0; c < S; ++c) taken += ok ? a.gone[(int64_t)c * a.n_users + q] : 0;
    const int64_t others = ok ? a.n_items - taken : 0;
    if (lane == 0 && n_neg) n_neg[q] = (int32_t)others;
    for (int64_t j = b + lane; j < e; j += kWave) {
        int hi = 0, lo = 0;
        for (int c = 0; c < S && ok; ++c) {
            hi += a.cnt[((int64_t)c * 2) * a.Q + j];
            lo += a.cnt[((int64_t)c * 2 + 1) * a.Q + j];
        }
        above[j] = hi;
        if (below) below[j] = lo;
        pos_score[j] = ok ? a.thr[j] : 0.f;
        if (auc) auc[j] = others > 0 ? (float)lo / (float)others : 0.f;
    }
}

int check_scalars(const char *what, int E, int H, int K, int64_t num_users, int64_t num_items, int64_t ld_emb, int64_t n_users,
                  int64_t Q, int64_t item_lo, int64_t n_items) {
    PEA_REQUIRE(pea_nfm_supported(E, H), PEA_ERR_ARG, "%s: emb_dim %d with hidden_size %d is not supported (pea_nfm_supported)", what, E,
                H);
    PEA_REQUIRE(scan_supported(E, H, K), PEA_ERR_ARG, "%s: K=%d with widths (%d, %d) is not supported (pea_nfm_scan_supported)", what, K,
                E, H);
    PEA_REQUIRE(num_users > 0 && Q >= 0, PEA_ERR_ARG, "%s: num_users=%lld Q=%lld", what, (long long)num_users, (long long)Q);
    PEA_TRY(check_catalogue(what, n_users, num_items, item_lo, n_items));
    PEA_REQUIRE(ld_emb >= E && ld_emb % 4 == 0, PEA_ERR_ARG, "%s: row stride %lld of emb (a multiple of 4, at least %d)", what,
                (long long)ld_emb, E);
    return PEA_OK;
}

int check_fold(const char *what, const float *emb, const float *lin, const float *w_fold, const float *b_fold, const float *w2,
               const float *bias_fold, const int64_t *uids, const int *err_flag, const void *workspace) {
    PEA_REQUIRE(emb && lin && w_fold && b_fold && w2 && bias_fold && uids && err_flag && workspace, PEA_ERR_ARG, "%s: null pointer", what);
    PEA_REQUIRE(aligned16(emb) && aligned16(w_fold) && aligned16(b_fold) && aligned16(w2) && aligned16(workspace), PEA_ERR_ARG,
                "%s: emb, w_fold, b_fold, w2 and the workspace must start on 16-byte boundaries", what);
    return PEA_OK;
}

template <bool RANK>
int launch_scan(const ScArgs &a, int S, hipStream_t stream) {
    const size_t lds = scan_lds_bytes(a.E, a.H, a.K);
    PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&nfm_scan_kernel<RANK>), lds_limit(lds)));
    const dim3 grid((unsigned)user_blocks(a.n_users), (unsigned)S);
    PEA_LAUNCH(nfm_scan_kernel<RANK>, grid, dim3(kThreads), lds, stream, a);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

// the rank forms: thresholds, scan, finish.  pos_rowptr null: one positive per user (Q = n_users)
int rank_call(ScArgs a, const WsLayout &l, void *workspace, int32_t *above, int32_t *below, float *pos_score,
              int32_t *n_neg, float *auc, hipStream_t stream) {
    char *ws = (char *)workspace;
    a.thr = (float *)(ws + l.off_thr);
    a.cnt = (int *)(ws + l.off_cnt);
    a.gone = (int *)(ws + l.off_gone);
    a.span = l.span;
    if (a.n_users == 0) return PEA_OK;
    if (a.Q > 0) {
        PEA_MEMSET_ASYNC(a.cnt, 0, l.cnt_bytes, stream);
        const size_t lds = thr_lds_bytes(a.E, a.H);
        PEA_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(&nfm_thr_kernel), lds_limit(lds)));
        ProfScope ps("nfm_scan_thr", stream, (double)a.Q * 2.0 * a.E * a.H, (double)a.Q * 8.0 * a.E);
        PEA_LAUNCH(nfm_thr_kernel, dim3((unsigned)std::min<int64_t>((a.Q + kSP - 1) / kSP, kThrMaxWg)), dim3(kThreads), lds, stream, a);
        PEA_HIP(hipGetLastError());
    }
    {
        ProfScope ps("nfm_rank_scan", stream, (double)a.n_users * (double)a.n_items * 2.0 * a.E * a.H);
        PEA_TRY(launch_scan<true>(a, l.S, stream));
    }
    {
        ProfScope ps("nfm_rank_finish", stream, 8.0 * (double)a.Q * l.S);
        PEA_LAUNCH(nfm_rank_finish_kernel, dim3((unsigned)((a.n_users + 3) / 4)), dim3(256), 0, stream, a, l.S, above, below, pos_score,
                   n_neg, auc);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

ScArgs fold_args(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb, const float *lin,
                 const float *w_fold, const float *b_fold, const float *w2, const float *bias_fold, const int64_t *uids, int64_t n_users,
                 int64_t item_lo, int64_t n_items, int64_t item_node0, const int64_t *excl_rowptr, const int64_t *excl_items,
                 int *err_flag) {
    ScArgs a = {};
    a.n_users = n_users; a.U = num_users; a.I = num_items; a.ld_emb = ld_emb; a.item_lo = item_lo; a.n_items = n_items;
    a.node0 = item_node0;
    a.E = E; a.H = H; a.EP = ceil16(E); a.HP = ceil16(H); a.LD = a.EP + 4;
    a.emb = emb; a.lin = lin; a.wf = w_fold; a.bf = b_fold; a.w2 = w2; a.bias = bias_fold; a.uid = uids;
    a.excl_rowptr = excl_rowptr; a.excl_items = excl_items; a.err = err_flag;
    return a;
}

}  // namespace
}  // namespace pea

using namespace pea;

extern "C" int pea_nfm_scan_supported(int E, int H, int K) { return scan_supported(E, H, K) ? 1 : 0; }

extern "C" int pea_nfm_scan_splits(int64_t n_users, int64_t n_items, int K) {
    if (n_users < 0 || n_items < 0 || K < 0 || K > 128) return 0;
    int S = 1;
    int64_t span = 0;
    catalogue_split(user_blocks(n_users), n_items, std::max(K, 1), kSP, &S, &span);
    return S;
}

extern "C" size_t pea_nfm_scan_workspace_bytes(int64_t n_users, int64_t Q, int64_t n_excl, int64_t n_items, int K, int E, int H) {
    if (!scan_supported(E, H, K) || n_users < 0 || Q < 0 || n_excl < 0 || n_items < 0 || n_items >= ((int64_t)1 << 31) - 1) return 0;
    return ws_layout(n_users, Q, n_items, K).total;
}

extern "C" int pea_nfm_recommend_topk(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb,
                                      const float *lin, const float *w_fold, const float *b_fold, const float *w2,
                                      const float *bias_fold, const int64_t *uids, int64_t n_users, int K, int64_t item_lo,
                                      int64_t n_items, int64_t item_node0, const int64_t *excl_rowptr, const int64_t *excl_items,
                                      int64_t *out_items, float *out_scores, int *err_flag, void *workspace, size_t workspace_bytes,
                                      void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "nfm_recommend_topk";
    PEA_REQUIRE(K >= 1 && K <= 128, PEA_ERR_ARG, "%s: K=%d (1..128)", what, K);
    PEA_TRY(check_scalars(what, E, H, K, num_users, num_items, ld_emb, n_users, 0, item_lo, n_items));
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "%s: excl_rowptr without excl_items", what);
    const WsLayout l = ws_layout(n_users, 0, n_items, K);
    PEA_REQUIRE(workspace_bytes >= l.total, PEA_ERR_NOMEM, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, l.total);
    PEA_TRY(check_fold(what, emb, lin, w_fold, b_fold, w2, bias_fold, uids, err_flag, workspace));
    PEA_REQUIRE(out_items && out_scores, PEA_ERR_ARG, "%s: null pointer", what);
    if (n_users == 0) return PEA_OK;
    ScArgs a = fold_args(E, H, num_users, num_items, emb, ld_emb, lin, w_fold, b_fold, w2, bias_fold, uids, n_users, item_lo, n_items,
                         item_node0, excl_rowptr, excl_items, err_flag);
    a.K = K;
    a.span = l.span;
    a.part_s = (float *)((char *)workspace + l.off_s);
    a.part_i = (int *)((char *)workspace + l.off_i);
    {
        ProfScope ps("nfm_topk_scan", stream, (double)n_users * (double)n_items * 2.0 * E * H);
        PEA_TRY(launch_scan<false>(a, l.S, stream));
    }
    {
        ProfScope ps("nfm_topk_merge", stream, 8.0 * (double)n_users * K * (l.S + 1.5));
        int p2 = 2;
        while (p2 < l.S * K) p2 <<= 1;       // <= kMaxMerge: catalogue_split keeps S K <= 2048
        PEA_LAUNCH(topk_merge_kernel, dim3((unsigned)n_users), dim3(p2 <= 128 ? 64 : 256), 0, stream, n_users, K, l.S, p2,
                   item_node0 + item_lo, (const float *)a.part_s, (const int *)a.part_i, out_items, out_scores);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

extern "C" int pea_nfm_rank_full(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb, const float *lin,
                                 const float *w_fold, const float *b_fold, const float *w2, const float *bias_fold,
                                 const int64_t *uids, int64_t n_users, const int64_t *pos_items, int64_t item_lo, int64_t n_items,
                                 int64_t item_node0, const int64_t *excl_rowptr, const int64_t *excl_items, int32_t *rank, float *auc,
                                 float *pos_score, int *err_flag, void *workspace, size_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "nfm_rank_full";
    PEA_TRY(check_scalars(what, E, H, 0, num_users, num_items, ld_emb, n_users, n_users, item_lo, n_items));
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "%s: excl_rowptr without excl_items", what);
    const WsLayout l = ws_layout(n_users, n_users, n_items, 0);
    PEA_REQUIRE(workspace_bytes >= l.total, PEA_ERR_NOMEM, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, l.total);
    PEA_TRY(check_fold(what, emb, lin, w_fold, b_fold, w2, bias_fold, uids, err_flag, workspace));
    PEA_REQUIRE(pos_items && rank && auc && pos_score, PEA_ERR_ARG, "%s: null pointer", what);
    ScArgs a = fold_args(E, H, num_users, num_items, emb, ld_emb, lin, w_fold, b_fold, w2, bias_fold, uids, n_users, item_lo, n_items,
                         item_node0, excl_rowptr, excl_items, err_flag);
    a.Q = n_users;
    a.pos_items = pos_items;
    return rank_call(a, l, workspace, rank, nullptr, pos_score, nullptr, auc, stream);
}

extern "C" int pea_nfm_rank_full_multi(int E, int H, int64_t num_users, int64_t num_items, const float *emb, int64_t ld_emb,
                                       const float *lin, const float *w_fold, const float *b_fold, const float *w2,
                                       const float *bias_fold, const int64_t *uids, int64_t n_users, const int64_t *pos_rowptr,
                                       const int64_t *pos_items, int64_t Q, int64_t item_lo, int64_t n_items, int64_t item_node0,
                                       const int64_t *excl_rowptr, const int64_t *excl_items, int32_t *above, int32_t *below,
                                       float *pos_score, int32_t *n_neg, int *err_flag, void *workspace, size_t workspace_bytes,
                                       void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *what = "nfm_rank_full_multi";
    PEA_TRY(check_scalars(what, E, H, 0, num_users, num_items, ld_emb, n_users, Q, item_lo, n_items));
    PEA_REQUIRE(!excl_rowptr || excl_items, PEA_ERR_ARG, "%s: excl_rowptr without excl_items", what);
    const WsLayout l = ws_layout(n_users, Q, n_items, 0);
    PEA_REQUIRE(workspace_bytes >= l.total, PEA_ERR_NOMEM, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, l.total);
    PEA_TRY(check_fold(what, emb, lin, w_fold, b_fold, w2, bias_fold, uids, err_flag, workspace));
    PEA_REQUIRE(pos_rowptr && pos_items && above && below && pos_score && n_neg, PEA_ERR_ARG, "%s: null pointer", what);
    ScArgs a = fold_args(E, H, num_users, num_items, emb, ld_emb, lin, w_fold, b_fold, w2, bias_fold, uids, n_users, item_lo, n_items,
                         item_node0, excl_rowptr, excl_items, err_flag);
    a.Q = Q;
    a.pos_rowptr = pos_rowptr;
    a.pos_items = pos_items;
    return rank_call(a, l, workspace, above, below, pos_score, n_neg, nullptr, stream);
}
