// Backward of the GAT aggregation for gfx950 (training; SURVEY.md section 8f rank 1: loss.backward() at reference
// solvers.py:215 runs autograd through GATConv's index_select / softmax / scatter).  Two gather passes, no atomics:
//
//   forward, per head:  z_ij = a_src_j + a_dst_i,  e_ij = leaky_relu(z_ij),  alpha_ij = exp(e_ij - m_i) / (S_i + 1e-16),
//                       out_i = sum_j alpha_ij T_j + b        (a_src_j = att_j . T_j,  a_dst_i = att_i . T_i)
//   given g_i = dL/d out_i:   c_i = g_i . (out_i - b)                      (= sum_j alpha_ij  g_i . T_j)
//                             d e_ij = alpha_ij (g_i . T_j - c_i),  d z_ij = d e_ij * leaky'(z_ij)
//   D pass (destination rows, forward CSR, gathers T_j):   d a_dst_i = sum_j d z_ij   (+ the side record
//                             [a_dst_i, m_i, 1/(S_i+eps), c_i] the S pass gathers)
//   S pass (source rows, REVERSED relation, gathers g_i):  d a_src_j = sum_i d z_ij
//                             dT_j = sum_i alpha_ij g_i + att_j d a_src_j + att_i d a_dst_j
// The softmax statistics (m_i in the log2 domain, S_i) were saved by the forward (AggGroup::stats); logits are
// recomputed from the rows exactly as in agg.hip (natural units; the weight is 2^(e log2(e) - m_i), agg_common.h: Soft).
// Same work decomposition as the forward: short rows per lane subgroup, long rows / hub chunks per wave, hub chunks
// folded in chunk order by a merge kernel -> bitwise reproducible gradients.
//
// Each pass (D, S, and the linear AGG_SUM_BWD_S) is one Pass<MODE, F4T>: what a lane keeps of its row, the 4-edge step, the
// hub chunk's record and the row's end.  bwd_short_rows, bwd_long_item and bwd_merge_kernel walk edges and records and know
// no mode.
#include <algorithm>

#include "agg_common.h"

namespace pea {
namespace {

// ------------------------------------------------------------------------------------------------ the lane, the flags
// What a lane is in a gather body: lane sl of the sub-th G-lane subgroup of its wave; it owns columns c4 .. c4 + 3, which
// belong to head k of nk, as lane pos of that head's F4 lanes.  Lanes past the group's width (and those of a subgroup
// without a row) are not `active`: they run along on column 0, because the head sums are cross-lane, and store nothing.
// wave_row: the wave's subgroups share one row (a long item, a hub row), so a test on the row is wave-uniform.
struct LaneView {
    int lane, sub, sl, c4, F4, pos, k, nk;
    bool active, pow2, wave_row, head_first;
    __device__ __forceinline__ LaneView(const AggGroup &P, int G, bool valid, bool wave_row_) : wave_row(wave_row_) {
        lane = (int)threadIdx.x % kWave;
        sub = lane / G;
        sl = lane % G;
        active = valid && sl * 4 < P.W;
        c4 = active ? sl * 4 : 0;
        F4 = P.F / 4;
        pos = sl % F4;
        pow2 = (F4 & (F4 - 1)) == 0;
        k = c4 / P.F;
        head_first = c4 - k * P.F == 0;   // the lane that reads and writes its head's scalars (one division for both)
        nk = P.W / P.F;
    }
    template <int F4T>
    __device__ __forceinline__ float head_sum(float v) const { return pea::head_sum<F4T>(v, lane, pos, F4, pow2); }
};

// row_active (optional): rows whose output gradient is exactly zero (every row outside the BPR batch, for the last
// layer) contribute nothing: the D pass writes d a_dst = 0 for them without gathering, the S pass skips their edges.
// SP: the launch has groups with row flags (the last layer of a training step).  The dense launches (SP = false: the first
// layer's x-space passes, 1.9 of the step's 5.6 ms) are compiled without the flag tests and the survivor queue: as run-time
// branches on a null pointer they cost the S pass 127 M scalar instructions per launch against 38 M of the D pass
// (SQ_INSTS_SALU, profiles/collect_sq_kind.sh gat train).
template <bool SP>
__device__ __forceinline__ bool row_flagged(const AggGroup &P, int row) {
    return !SP || !P.row_active || P.row_active[row] != 0;
}

// is the gathered row i live?  (bitmap when the host built one, else the byte flags)
__device__ __forceinline__ bool row_live(const AggGroup &P, int i) {
    if (P.row_active_bits) return (P.row_active_bits[(unsigned)i >> 5] >> ((unsigned)i & 31u)) & 1u;
    return P.row_active[i] != 0;
}

// The id at CSR slot e of a row that ends at `end`; -1 past the end and (FILTER: a pass over out-edges, in an SP launch) for a
// gathered row that is not flagged: rows known to be zero are not fetched.
template <bool FILTER>
__device__ __forceinline__ int live_id(const AggGroup &P, int e, int end) {
    int id = e < end ? P.col[e] : -1;
    if (FILTER && P.row_active && id >= 0 && !row_live(P, id)) id = -1;
    return id;
}

// ------------------------------------------------------------------------------------------------ the passes
// What a pass sums over the edges of a row (ACC: a row of W columns; DZ: one scalar per head), and how the sums travel:
// across the subgroups of a wave, into a hub chunk's partial record [acc (W) | per head: unused, dsum], out of the records.
template <bool ACC, bool DZ>
struct RowSums {
    const AggGroup &P;
    const LaneView &V;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float dsum = 0.f;
    __device__ __forceinline__ RowSums(const AggGroup &P_, const LaneView &V_) : P(P_), V(V_) {}

    template <int G>
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int off = G; off < kWave; off <<= 1) {
            if (DZ) dsum += __shfl_xor(dsum, off);
            if (ACC) acc = add4(acc, shfl_xor4(acc, off));
        }
    }
    __device__ __forceinline__ float *record(int slot) const { return P.partial + (size_t)slot * (size_t)(P.W + 2 * V.nk); }
    __device__ __forceinline__ void partial(int slot) const {
        float *rec = record(slot);
        if (ACC) st4(rec + V.c4, acc);
        if (DZ && V.head_first) rec[P.W + 2 * V.k + 1] = dsum;
    }
    // chunk order, every subgroup the same value; 8 records in flight per step (one dependent load per record made this
    // kernel 0.13 ms for a hub row of ~300 chunks): slots past the end re-read the last record and add zero, so the adds
    // stay unconditional and the compiler keeps the loads ahead of them
    __device__ __forceinline__ void merge(int first, int count) {
        constexpr int UM = 8;
        for (int c0 = 0; c0 < count; c0 += UM) {
            float4 a[UM];
            float dd[UM];
#pragma unroll
            for (int u = 0; u < UM; ++u) {
                const float *rec = record(first + (c0 + u < count ? c0 + u : count - 1));
                a[u] = ACC ? ld4(rec + V.c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                dd[u] = DZ ? rec[P.W + 2 * V.k + 1] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < UM; ++u) {
                const float f = c0 + u < count ? 1.f : 0.f;
                if (ACC) acc = fma4(f, a[u], acc);
                if (DZ) dsum = fmaf(f, dd[u], dsum);
            }
        }
    }
};

// A pass: load(row), step4(ids, ok) per 4 edges (ids of slots that are not ok are 0; every load of the step goes ahead of
// its arithmetic), fold / partial / merge from RowSums, close(row, row_on, store) at the row's end.  close<true> is the
// late-load form of the merge kernel: no load() went before.  kFiltered: the pass walks a source row's out-edges and drops
// those to unflagged rows; kSkipsDead: an unflagged row of its own gathers nothing and ends in dead().
template <int MODE, int F4T>
struct Pass;

template <int F4T>
struct Pass<AGG_GAT_BWD_D, F4T> : RowSums<false, true> {
    static constexpr bool kFiltered = false, kSkipsDead = true;
    float4 att_s, g, hself;
    float a_d, m, inv_s, c;
    using RowSums::RowSums;

    __device__ __forceinline__ void load(int row) {
        att_s = ld4(P.att_src + V.c4);
        hself = ld4(row_at(P.feat_self + V.c4, row, P.ld_self));
        a_d = V.head_sum<F4T>(dot4(hself, ld4(P.att_dst + V.c4)));
        g = ld4(row_at(P.g_self + V.c4, row, P.ld_g));
        float4 o = ld4(row_at(P.o_self + V.c4, row, P.ld_g));
        if (P.bias) {
            const float4 b = ld4(P.bias + V.c4);
            o = make_float4(o.x - b.x, o.y - b.y, o.z - b.z, o.w - b.w);
        }
        c = V.head_sum<F4T>(dot4(g, o));
        const float *sp = P.stats + (size_t)row * P.ld_stats + 2 * (V.c4 / P.F);
        m = sp[0];
        inv_s = 1.0f / (sp[1] + 1e-16f);
    }
    // d z of one edge as seen from the destination row (h = gathered T_j)
    __device__ __forceinline__ float dz_edge(float4 h) const {
        const float zl = V.head_sum<F4T>(dot4(h, att_s)) + a_d;
        const float alpha = __builtin_amdgcn_exp2f(fmaf(leaky(zl, P.neg_slope), kLog2e, -m)) * inv_s;
        const float dal = V.head_sum<F4T>(dot4(h, g));
        return alpha * (dal - c) * (zl > 0.f ? 1.f : P.neg_slope);
    }
    __device__ __forceinline__ void step4(const int (&ids)[4], const bool (&ok)[4]) {
        float4 h[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) h[u] = ld4(row_at(P.feat + V.c4, ids[u], P.ld_feat));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float dz = dz_edge(h[u]);
            dsum = ok[u] ? dsum + dz : dsum;   // a select: as a branch the compiler sinks each edge's arithmetic into it
        }
    }
    // d a_dst of an unflagged row (its side record is never read: the S pass does not fetch the row)
    __device__ __forceinline__ void dead(int row, bool store) const {
        if (store && V.head_first) P.ksum[(size_t)row * P.ld_k + V.k] = 0.f;
    }
    // row_on is lane-local (short rows: one row per subgroup), the head sum of the self loop is not: every lane runs it
    template <bool LATE = false>
    __device__ __forceinline__ void close(int row, bool row_on, bool store) {
        if (LATE) load(row);
        if (P.self_loop) {
            const float dz = dz_edge(hself);
            if (row_on) dsum += dz;
        }
        if (!row_on) return dead(row, store);
        if (!store || !V.head_first) return;
        P.ksum[(size_t)row * P.ld_k + V.k] = dsum;
        st4(P.side_out + (size_t)row * P.ld_side + 4 * V.k, make_float4(a_d, m, inv_s, c));
    }
};

template <int F4T>
struct Pass<AGG_GAT_BWD_S, F4T> : RowSums<true, true> {
    static constexpr bool kFiltered = true, kSkipsDead = false;
    float4 att_s, t;
    float a_s;
    using RowSums::RowSums;

    __device__ __forceinline__ void load(int row) {
        att_s = ld4(P.att_src + V.c4);
        t = ld4(row_at(P.feat_self + V.c4, row, P.ld_self));
        a_s = V.head_sum<F4T>(dot4(t, att_s));
    }
    // one out-edge as seen from the source row: g = gathered output-gradient row of the destination, sd = its side record
    __device__ __forceinline__ void edge(float4 g, float4 sd, bool ok) {
        const float zl = a_s + sd.x;
        const float alpha = __builtin_amdgcn_exp2f(fmaf(leaky(zl, P.neg_slope), kLog2e, -sd.y)) * sd.z;
        const float dal = V.head_sum<F4T>(dot4(g, t));
        const float dz = alpha * (dal - sd.w) * (zl > 0.f ? 1.f : P.neg_slope);
        if (ok) {
            acc = fma4(alpha, g, acc);
            dsum += dz;
        }
    }
    __device__ __forceinline__ void step4(const int (&ids)[4], const bool (&ok)[4]) {
        float4 g[4], sd[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            g[u] = ld4(row_at(P.feat + V.c4, ids[u], P.ld_feat));
            sd[u] = ld4(row_at(P.side + 4 * V.k, ids[u], P.ld_side));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) edge(g[u], sd[u], ok[u]);
    }
    // The self loop is an edge to the row's own side record, unless the row is `lone` (deg0_self: its forward softmax had
    // the self loop alone, alpha = 1 exactly and d z = 0; it has no side record).  Two forms, the same values.  One row per
    // wave (long items, hub rows): a branch on `lone`, the form these bodies have always had.  Short rows: lone and row_on
    // differ between the subgroups of a wave and the head sum inside edge() is cross-lane, so every lane runs edge() and
    // the flags only decide what is kept.
    template <bool LATE = false>
    __device__ __forceinline__ void close(int row, bool row_on, bool store) {
        if (LATE) load(row);
        if (P.self_loop) {
            const bool lone = P.deg0_self && P.deg0_self[row] != 0;
            if (V.wave_row) {
                if (!lone) edge(ld4(row_at(P.feat + V.c4, row, P.ld_feat)), ld4(row_at(P.side + 4 * V.k, row, P.ld_side)), row_on);
                else if (row_on) acc = add4(acc, ld4(row_at(P.feat + V.c4, row, P.ld_feat)));
            } else {
                const float4 gs = ld4(row_at(P.feat + V.c4, row, P.ld_feat));
                float4 sd = make_float4(0.f, 0.f, 1.f, 0.f);
                if (!lone) sd = ld4(row_at(P.side + 4 * V.k, row, P.ld_side));
                edge(gs, sd, row_on && !lone);
                if (row_on && lone) acc = add4(acc, gs);
            }
        }
        if (!store) return;
        const float dad = P.da_dst[(size_t)row * P.ld_k + V.k];
        const float4 at_d = ld4(P.att_dst + V.c4);
        const float ws = dsum, wd = dad;   // natural-unit logits and attention vectors: d z / d T_j = att_j
        float4 o;
        o.x = acc.x + ws * att_s.x + wd * at_d.x;
        o.y = acc.y + ws * att_s.y + wd * at_d.y;
        o.z = acc.z + ws * att_s.z + wd * at_d.z;
        o.w = acc.w + ws * att_s.w + wd * at_d.w;
        st4(P.out + (size_t)row * P.ld_out + V.c4, o);
        if (V.head_first) P.ksum[(size_t)row * P.ld_k + V.k] = dsum;
    }
};

template <int F4T>
struct Pass<AGG_SUM_BWD_S, F4T> : RowSums<true, false> {
    static constexpr bool kFiltered = true, kSkipsDead = false;
    float di;
    using RowSums::RowSums;

    __device__ __forceinline__ void load(int row) { di = P.dinv_self[row]; }
    __device__ __forceinline__ void step4(const int (&ids)[4], const bool (&ok)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!ok[u]) continue;                       // rows known to be zero are not fetched
            acc = fma4(P.dinv[ids[u]], ld4(row_at(P.feat + V.c4, ids[u], P.ld_feat)), acc);
        }
    }
    template <bool LATE = false>
    __device__ __forceinline__ void close(int row, bool row_on, bool store) {
        if (LATE) load(row);
        if (P.self_loop && row_on) acc = fma4(di, ld4(row_at(P.feat_self + V.c4, row, P.ld_self)), acc);
        if (store) st4(P.out + (size_t)row * P.ld_out + V.c4, scale4(acc, di));
    }
};

// ------------------------------------------------------------------------------------------------ short rows
// One G-lane subgroup per row, 4 edges in flight (ids, then rows, then the arithmetic), as in the forward's short_rows.
template <int G, int MODE, int F4T, bool SP>
__device__ __forceinline__ void bwd_short_rows(const AggGroup &P, const int blk) {
    using PassT = Pass<MODE, F4T>;
    const int item = blk * (kBlock / G) + (int)threadIdx.x / G;
    const bool valid = item < P.n_short;
    const int row = valid ? P.short_rows[item] : 0;
    const LaneView V(P, G, valid, false);
    const bool row_on = row_flagged<SP>(P, row);
    const int beg = P.rowptr[row];
    const int end = (valid && !(PassT::kSkipsDead && !row_on)) ? P.rowptr[row + 1] : beg;
    int len = end - beg;
    for (int off = G; off < kWave; off <<= 1) len = max(len, __shfl_xor(len, off));  // head sums are cross-lane
    PassT pass(P, V);
    pass.load(row);
    for (int t = 0; t < len; t += 4) {
        int ids[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int id = live_id<SP && PassT::kFiltered>(P, beg + t + u, end);
            ok[u] = id >= 0;
            ids[u] = ok[u] ? id : 0;
        }
        pass.step4(ids, ok);
    }
    pass.close(row, row_on, V.active);
}

// ------------------------------------------------------------------------------------------------ long rows / hub chunks
// 64 ids, one per lane (< 0: none), of which the first cnt slots count: 4 per subgroup and step, in slot order.
template <int G, class PassT>
__device__ __forceinline__ void walk_ids(PassT &pass, const LaneView &V, int id, int cnt) {
    constexpr int NSG = kWave / G;
    for (int t = 0; t < cnt; t += NSG * 4) {
        int ids[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = t + u * NSG + V.sub;
            const int j = __shfl(id, idx & (kWave - 1));
            ok[u] = idx < cnt && j >= 0;
            ids[u] = ok[u] ? j : 0;
        }
        pass.step4(ids, ok);
    }
}

// Batch-sparse S pass (the last layer: 2.5 % of the gathered rows carry a gradient): the surviving edges of SEVERAL batches
// of 64 are queued (edge order kept) and processed together.  Packing each batch on its own (round 2) still paid one
// whole 4-edges-per-subgroup iteration for the 1-2 survivors of nearly every batch: 0.32 ms to find and process the
// 0.6 M live edges among 24.8 M.
// The queue is the wave's row of LDS: up to 64 ids, oldest first.
struct LiveQueue {
    int *slot;
    int n = 0;
    __device__ __forceinline__ explicit LiveQueue(int *wave_row) : slot(wave_row) {}
    // `live`: the ballot of the lanes whose id of the batch survived
    __device__ __forceinline__ bool fits(unsigned long long live) const { return n + __popcll(live) <= kWave; }
    // appends the batch's survivors in lane (= edge) order
    __device__ __forceinline__ void offer(int id, unsigned long long live) {
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(live >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)live, 0));
        if (id >= 0) slot[n + before] = id;
        n += __popcll(live);
    }
    // hands the queue over, one id per lane, and empties it
    __device__ __forceinline__ int take(int lane, int &cnt) {
        const int id = lane < n ? slot[lane] : -1;
        cnt = n;
        n = 0;
        return id;
    }
};

template <int G, int MODE, int F4T, bool SP>
__device__ __forceinline__ void bwd_long_item(const AggGroup &P, const int blk) {
    using PassT = Pass<MODE, F4T>;
    constexpr bool kFilter = SP && PassT::kFiltered;
    const LongItem it = item_at(P, blk * (kBlock / kWave) + (int)threadIdx.x / kWave);
    if (it.slot == -2) return;
    const LaneView V(P, G, true, true);
    const bool store = V.sub == 0 && V.active;
    const bool row_on = row_flagged<SP>(P, it.row);
    PassT pass(P, V);
    if constexpr (PassT::kSkipsDead) {
        if (!row_on) {   // hub chunks of such a row leave their partial records alone: the merge kernel does not read them
            if (it.slot < 0) pass.dead(it.row, store);
            return;
        }
    }
    pass.load(it.row);
    __shared__ int live_rows[kBlock / kWave][kWave];
    LiveQueue queue(live_rows[(int)threadIdx.x / kWave]);
    const bool queued = kFilter && P.row_active != nullptr;
    // Unqueued, a batch of 64 ids is walked as it is.  Queued, its survivors join the queue and nothing is walked (collect and
    // continue) unless they no longer fit: then the queue is walked first and the batch starts the next one (a flush, mid-row
    // or on the last batch).  What is queued when the row ends is walked behind the loop: the whole row's survivors, the
    // second walk after a flush on the last batch, or nothing.  One walk_ids serves the batch and the flush: as two inlined
    // copies they cost eleven flagged S instantiations 5 to 13 VGPRs and a wave of occupancy.
    int id = live_id<kFilter>(P, it.beg + V.lane, it.end), cnt;
    for (int base = it.beg; base < it.end; base += kWave) {
        const int id_next = live_id<kFilter>(P, base + kWave + V.lane, it.end);
        int now = id;
        bool walk = true;
        cnt = min(kWave, it.end - base);
        if (queued) {
            const unsigned long long live = __ballot(id >= 0);
            walk = !queue.fits(live);                // (wave-uniform)
            if (walk) now = queue.take(V.lane, cnt);
            queue.offer(id, live);
        }
        if (walk) walk_ids<G>(pass, V, now, cnt);
        id = id_next;
    }
    if (queued) {
        id = queue.take(V.lane, cnt);
        walk_ids<G>(pass, V, id, cnt);
    }
    pass.template fold<G>();
    if (it.slot >= 0) {
        if (store) pass.partial(it.slot);
        return;
    }
    pass.close(it.row, row_on, store);
}

// One launch per pass and lane width, like the forward's agg_rows_kernel: workgroups [0, n_long_blocks) take the long rows
// and hub chunks, the rest the short rows (they fill the machine while the last long items drain).
template <int G, int MODE, int F4T, bool SP>
__global__ __launch_bounds__(kBlock) void bwd_rows_kernel(const AggLaunch L) {
    if ((int)blockIdx.x >= L.n_long_blocks) {
        const int b = (int)blockIdx.x - L.n_long_blocks;
        int gi = 0;
        while (gi + 1 < L.n_groups && b >= L.blk_short[gi + 1]) ++gi;
        bwd_short_rows<G, MODE, F4T, SP>(L.g[gi], b - L.blk_short[gi]);
        return;
    }
    const int gi = find_group(L);
    bwd_long_item<G, MODE, F4T, SP>(L.g[gi], (int)blockIdx.x - L.blk_start[gi]);
}

// ------------------------------------------------------------------------------------------------ hub rows
// One wave per hub row: its chunks' records in chunk order, then the row's end.
template <int G, int MODE, int F4T>
__global__ __launch_bounds__(kBlock) void bwd_merge_kernel(const AggLaunch L) {
    using PassT = Pass<MODE, F4T>;
    const int gi = find_group(L);
    const AggGroup &P = L.g[gi];
    const int item = ((int)blockIdx.x - L.blk_start[gi]) * (kBlock / kWave) + (int)threadIdx.x / kWave;
    if (item >= P.n_hub) return;
    // All three loads before anything that needs the row: read where they are used, or with hub_rows first (the compiler then
    // waits for the row before it issues the third), each late load cost the hub row a dependent round trip (+ 0.2 ... 1 us).
    const int first = P.hub_first[item], count = P.hub_count[item], row = P.hub_rows[item];
    const LaneView V(P, G, true, true);
    const bool store = V.sub == 0 && V.active;
    const bool row_on = row_flagged<true>(P, row);
    PassT pass(P, V);
    if constexpr (PassT::kSkipsDead) {
        if (!row_on) return pass.dead(row, store);
    }
    pass.merge(first, count);
    pass.template close<true>(row, row_on, store);
}

// ------------------------------------------------------------------------------------------------ host
// profile names as profiles/summarize.py derives them from rocprofv3's kernel names (bwd_rows_kernel<G, MODE, F4T>).
// Launches whose rows / gathered rows are filtered by row_active (the last layer: only the BPR batch's rows carry a
// gradient) get their own name, *_batch.  A function-local static table, as the forward's launch_name.
template <int MODE>
constexpr const char *bwd_pass_name() {
    return MODE == AGG_GAT_BWD_D ? "gat_bwd_dst" : MODE == AGG_SUM_BWD_S ? "sum_bwd_src" : "gat_bwd_src";
}
template <int MODE>
constexpr const char *bwd_merge_name() {
    return MODE == AGG_GAT_BWD_D ? "gat_bwd_dst_merge" : MODE == AGG_SUM_BWD_S ? "sum_bwd_src_merge" : "gat_bwd_src_merge";
}
template <int G, int MODE>
const char *bwd_rows_name(bool batch) {
    struct Names {
        char s[2][32];
        Names() {
            snprintf(s[0], sizeof(s[0]), "%s_g%d", bwd_pass_name<MODE>(), G);
            snprintf(s[1], sizeof(s[1]), "%s_g%d_batch", bwd_pass_name<MODE>(), G);
        }
    };
    static const Names names;
    return names.s[batch];
}

// bytes a dense launch pulls through the memory system per message, each once (bench.py's live roofline): the gathered
// row chunk (D: T_j; S: the output-gradient row g_i) + the 4-byte index (+ S: the 16-byte side record per head)
template <int MODE>
double bwd_msg_bytes(const AggGroup &g) {
    return 4.0 * g.W + 4.0 + (MODE == AGG_GAT_BWD_S ? 16.0 * (g.W / g.F) : 0.0);
}

template <int G, int MODE, int F4T>
int launch_bwd_g(const AggLaunch &base, const int *sel, int n_sel, hipStream_t stream) {
    // the live messages of a filtered launch are not known on the host, so no byte count is attributed to it
    bool sparse = false;
    for (int i = 0; i < n_sel; ++i) sparse = sparse || base.g[sel[i]].row_active != nullptr;
    AggLaunch L;
    // long rows + hub chunks first, short rows behind them, one launch
    L.n_groups = 0;
    int blocks = 0, sblocks = 0;
    double pulled = 0.0, table = 0.0;
    for (int i = 0; i < n_sel; ++i) {
        const AggGroup &g = base.g[sel[i]];
        if (g.n_short <= 0 && g.n_long <= 0) continue;
        if (!sparse) {
            pulled += bwd_msg_bytes<MODE>(g) * (g.msgs_short + g.msgs_long);
            table = std::max(table, table_bytes(g));
        }
        L.blk_short[L.n_groups] = sblocks;
        add_group(L, g, g.n_long, blocks);
        if (g.n_short > 0) sblocks += (g.n_short + (kBlock / G) - 1) / (kBlock / G);
    }
    L.blk_start[L.n_groups] = blocks;
    L.blk_short[L.n_groups] = sblocks;
    L.n_long_blocks = blocks;
    if (blocks + sblocks > 0) {
        ProfScope ps(bwd_rows_name<G, MODE>(sparse), stream, pulled, pulled, table);
        if (sparse) PEA_LAUNCH((bwd_rows_kernel<G, MODE, F4T, true>), dim3(blocks + sblocks), dim3(kBlock), 0, stream, L);
        else if constexpr (MODE != AGG_SUM_BWD_S)
            PEA_LAUNCH((bwd_rows_kernel<G, MODE, F4T, false>), dim3(blocks + sblocks), dim3(kBlock), 0, stream, L);
        else   // the linear pass exists for the flags and has no dense kernel (launch_gat_backward says so first)
            PEA_REQUIRE(false, PEA_ERR_ARG, "AGG_SUM_BWD_S: no row_active flags (AGG_GCN is the dense form of this sum)");
        PEA_HIP(hipGetLastError());
    }
    // hub merge
    L.n_groups = 0;
    blocks = 0;
    for (int i = 0; i < n_sel; ++i) {
        const AggGroup &g = base.g[sel[i]];
        if (g.n_hub <= 0) continue;
        L.blk_start[L.n_groups] = blocks;
        L.g[L.n_groups++] = g;
        blocks += (g.n_hub + 3) / 4;
    }
    L.blk_start[L.n_groups] = blocks;
    if (blocks > 0) {
        ProfScope ps(bwd_merge_name<MODE>(), stream, 0.0);
        PEA_LAUNCH((bwd_merge_kernel<G, MODE, F4T>), dim3(blocks), dim3(kBlock), 0, stream, L);
        PEA_HIP(hipGetLastError());
    }
    return PEA_OK;
}

template <int G, int MODE>
int launch_bwd_cls(const AggLaunch &base, int cls, const int *sel, int n, hipStream_t stream) {
    if (cls == G) return launch_bwd_g<G, MODE, G>(base, sel, n, stream);
    if (cls == 4) return launch_bwd_g<G, MODE, (G >= 4 ? 4 : 0)>(base, sel, n, stream);
    return launch_bwd_g<G, MODE, 0>(base, sel, n, stream);
}

template <int MODE>
int launch_bwd_mode(const AggLaunch &base, hipStream_t stream) {
    const int classes[3] = {0, 4, -1};
    for (int G = 4; G <= 64; G <<= 1)
        for (int ci = 0; ci < 3; ++ci) {
            const int cls = classes[ci] < 0 ? G : classes[ci];
            if (ci == 1 && G == 4) continue;
            int sel[kMaxAggGroups], n = 0;
            for (int i = 0; i < base.n_groups; ++i) {
                const int f4 = base.g[i].F / 4;
                const int c = f4 == G ? G : f4 == 4 ? 4 : 0;
                if (lanes_for(base.g[i].W) == G && c == cls) sel[n++] = i;
            }
            if (!n) continue;
            switch (G) {
                case 4: PEA_TRY((launch_bwd_cls<4, MODE>(base, cls, sel, n, stream))); break;
                case 8: PEA_TRY((launch_bwd_cls<8, MODE>(base, cls, sel, n, stream))); break;
                case 16: PEA_TRY((launch_bwd_cls<16, MODE>(base, cls, sel, n, stream))); break;
                case 32: PEA_TRY((launch_bwd_cls<32, MODE>(base, cls, sel, n, stream))); break;
                default: PEA_TRY((launch_bwd_cls<64, MODE>(base, cls, sel, n, stream))); break;
            }
        }
    return PEA_OK;
}

// out_k[c] = sum_n A[n, c] * (S_k ? S_k[n, c / F] : 1) for c < W (k = 0 and, optionally, 1: two scaled sums over ONE read
// of A: the att_j and att_i gradients of a GAT level both weight T_s), rows in a fixed order (two stages, no atomics).
// Stage 1: block b owns a contiguous row chunk; each of its 4 waves streams WHOLE rows -- lane l reads the float4
// chunks l, l + 64, l + 128, l + 192 of a row, 4 rows in flight -- and the 4 waves' sums are folded through LDS in wave
// order.  (Round 1 read 64-column pieces, one dword per lane: nine strided passes over a 2304-byte-row table at
// 2.7 TB/s.)  MAPPED = false: rows 0..N-1 in place (one GPU); true: the rows a rank owns (RowMap).
constexpr int kColsumT = 4;   // float4 chunks per lane: column blocks of up to 1024 columns
// T = chunks per lane (W > 256: every lane of a wave works on ONE row); T == 1 and W <= 256: a row needs only
// C = pow2ceil(W / 4) lanes, so a wave streams 64 / C rows side by side (the sub-rows are folded through LDS with the waves)
template <bool MAPPED, bool TWO, int T>
__global__ __launch_bounds__(256) void colsum_stage1(const RowMap M, int W, int F, int C, const float *__restrict__ A, int lda,
                                                     const float *__restrict__ S0, const float *__restrict__ S1, int lds,
                                                     float *__restrict__ part, size_t part_stride) {
    extern __shared__ float red[];  // [4 waves][NK][64 lanes * T] float4 slots
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = 64 / C;                    // rows per wave step (1 when T > 1)
    const int rsub = lane / C, cl = lane % C;
    const int64_t n_all = M.size();
    const int64_t rows_per = (n_all + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per, r1 = min(n_all, r0 + rows_per);
    constexpr int NK = TWO ? 2 : 1;
    for (int cb = 0; cb < W; cb += 256 * T) {
        const int wb = min(W - cb, 256 * T);
        float4 acc[NK][T];
        bool on[T];
        int hk[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int c = cb + 4 * (cl + 64 * t);
            on[t] = c < cb + wb;
            hk[t] = on[t] ? c / F : 0;
#pragma unroll
            for (int k = 0; k < NK; ++k) acc[k][t] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        constexpr int U = 4;
        for (int64_t q = r0 + (int64_t)wave * R + rsub; q < r1; q += (int64_t)4 * R * U) {
            float4 v[U][T];
            float s0[U][T], s1[U][T];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t qq = q + (int64_t)4 * R * u;
                int64_t rr = MAPPED ? (qq < r1 ? M.row(qq) : 0) : qq;
                const bool rv = qq < r1 && (!MAPPED || rr < M.N);
                if (!rv) rr = 0;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const bool ok = rv && on[t];
                    v[u][t] = ok ? ld4(A + rr * lda + cb + 4 * (cl + 64 * t)) : make_float4(0.f, 0.f, 0.f, 0.f);
                    s0[u][t] = (ok && S0) ? S0[rr * lds + hk[t]] : 1.f;
                    if (TWO) s1[u][t] = ok ? S1[rr * lds + hk[t]] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)     // row order inside a lane: fixed
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    acc[0][t] = fma4(s0[u][t], v[u][t], acc[0][t]);
                    if (TWO) acc[1][t] = fma4(s1[u][t], v[u][t], acc[1][t]);
                }
        }
        // every (wave, sub-row) stream parks its sums; lanes of wave 0 / sub-row 0 fold them in (wave, sub-row) order
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int t = 0; t < T; ++t)
                st4(red + (((size_t)wave * NK + k) * T + t) * 256 + 4 * lane, acc[k][t]);
        __syncthreads();
        if (wave == 0 && rsub == 0) {
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    if (!on[t]) continue;
                    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int w = 0; w < 4; ++w)
                        for (int rs = 0; rs < R; ++rs)
                            r = add4(r, ld4(red + (((size_t)w * NK + k) * T + t) * 256 + 4 * (rs * C + cl)));
                    st4(part + (size_t)k * part_stride + (size_t)blockIdx.x * W + cb + 4 * (cl + 64 * t), r);
                }
        }
        __syncthreads();
    }
}

// 16 columns per block; thread (g, cc) adds parts g, g + 16, ... of its column in order, then one thread per column adds
// the 16 sub-sums in order: fixed summation order, 32 dependent loads per thread instead of 512
__global__ __launch_bounds__(256) void colsum_stage2(int nparts, int W, const float *__restrict__ part, float scale,
                                                     float *__restrict__ out) {
    __shared__ float sub[16][17];
    const int g = threadIdx.x >> 4, cc = threadIdx.x & 15, c = blockIdx.x * 16 + cc;
    float s = 0.f;
    if (c < W)
        for (int p = g; p < nparts; p += 16) s += part[(size_t)p * W + c];
    sub[g][cc] = s;
    __syncthreads();
    if (g == 0 && c < W) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) t += sub[q][cc];
        out[c] = t * scale;
    }
}

// in place: G[n, c] = O[n, c] > 0 ? G[n, c] : 0   (relu between steps, reference models/base.py:138)
__global__ __launch_bounds__(256) void relu_mask_kernel(const RowMap M, int W4, float *__restrict__ G, int ldg,
                                                        const float *__restrict__ O, int ldo) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M.n * W4) return;
    int64_t q;
    int c;
    if (M.n * W4 < (int64_t)1 << 31) {   // 32-bit division (the usual case): the 64-bit one costs ~40 instructions per thread
        const unsigned qi = (unsigned)idx / (unsigned)W4;
        q = qi;
        c = (int)((unsigned)idx - qi * (unsigned)W4) * 4;
    } else {
        q = idx / W4;
        c = (int)(idx % W4) * 4;
    }
    const int64_t r = M.row(q);
    if (r >= M.N) return;
    float4 g = ld4(G + r * ldg + c);
    const float4 o = ld4(O + r * ldo + c);
    g.x = o.x > 0.f ? g.x : 0.f;
    g.y = o.y > 0.f ? g.y : 0.f;
    g.z = o.z > 0.f ? g.z : 0.f;
    g.w = o.w > 0.f ? g.w : 0.f;
    st4(G + r * ldg + c, g);
}

}  // namespace

int launch_gat_backward(AggMode mode, const AggGroup *groups, int n_groups, hipStream_t stream) {
    PEA_REQUIRE(n_groups >= 0 && n_groups <= kMaxAggGroups, PEA_ERR_ARG, "gat backward: %d groups", n_groups);
    AggLaunch base;
    base.n_groups = n_groups;
    for (int i = 0; i < n_groups; ++i) base.g[i] = groups[i];
    if (mode == AGG_SUM_BWD_S) {
        for (int i = 0; i < n_groups; ++i)
            PEA_REQUIRE(groups[i].row_active != nullptr, PEA_ERR_ARG,
                        "AGG_SUM_BWD_S: group %d has no row_active flags (AGG_GCN is the dense form of this sum)", i);
        return launch_bwd_mode<AGG_SUM_BWD_S>(base, stream);
    }
    return mode == AGG_GAT_BWD_D ? launch_bwd_mode<AGG_GAT_BWD_D>(base, stream) : launch_bwd_mode<AGG_GAT_BWD_S>(base, stream);
}

template <bool MP, bool TW>
static void colsum_dispatch(int T, size_t lds_bytes, hipStream_t stream, const RowMap &rows, int W, int F, int C, const float *A,
                            int lda, const float *S0, const float *S1, int lds, float *part, size_t part_stride) {
#define PEA_COLSUM(TT)                                                                                                        \
    PEA_LAUNCH((colsum_stage1<MP, TW, TT>), dim3(kColsumParts), dim3(256), lds_bytes, stream, rows, W, F, C, A, lda, S0, \
                       S1, lds, part, part_stride)
    if (T == 1) PEA_COLSUM(1);
    else if (T == 2) PEA_COLSUM(2);
    else if (T == 3) PEA_COLSUM(3);
    else PEA_COLSUM(4);
#undef PEA_COLSUM
}

int launch_colsum2(const RowMap &rows, int W, int F, const float *A, int lda, const float *S0, const float *S1, int lds,
                   float scale, float *part, float *out0, float *out1, hipStream_t stream) {
    if (W <= 0) return PEA_OK;
    PEA_REQUIRE(W % 4 == 0 && lda % 4 == 0 && F % 4 == 0, PEA_ERR_ARG, "colsum: widths / strides must be multiples of 4");
    ProfScope ps("colsum", stream, 0.0);
    const bool two = S1 != nullptr;
    const size_t part_stride = (size_t)kColsumParts * W;   // second output's partials follow the first's
    const int w4 = W / 4;
    const int T = std::min(kColsumT, (w4 + 63) / 64);
    int C = 64;
    if (T == 1) {
        C = 1;
        while (C < w4) C <<= 1;
    }
    const size_t lds_bytes = (size_t)4 * (two ? 2 : 1) * T * 256 * sizeof(float);
    const bool mapped = rows.world > 1 || rows.list != nullptr;
    if (mapped && two) colsum_dispatch<true, true>(T, lds_bytes, stream, rows, W, F, C, A, lda, S0, S1, lds, part, part_stride);
    else if (mapped) colsum_dispatch<true, false>(T, lds_bytes, stream, rows, W, F, C, A, lda, S0, S1, lds, part, part_stride);
    else if (two) colsum_dispatch<false, true>(T, lds_bytes, stream, rows, W, F, C, A, lda, S0, S1, lds, part, part_stride);
    else colsum_dispatch<false, false>(T, lds_bytes, stream, rows, W, F, C, A, lda, S0, S1, lds, part, part_stride);
    PEA_LAUNCH(colsum_stage2, dim3((unsigned)((W + 15) / 16)), dim3(256), 0, stream, kColsumParts, W, part, scale, out0);
    if (two)
        PEA_LAUNCH(colsum_stage2, dim3((unsigned)((W + 15) / 16)), dim3(256), 0, stream, kColsumParts, W,
                           part + part_stride, scale, out1);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

int launch_colsum(const RowMap &rows, int W, int F, const float *A, int lda, const float *S, int lds, float scale, float *part,
                  float *out, hipStream_t stream) {
    return launch_colsum2(rows, W, F, A, lda, S, nullptr, lds, scale, part, out, nullptr, stream);
}

int launch_relu_mask(const RowMap &rows, int W, float *G, int ldg, const float *O, int ldo, hipStream_t stream) {
    if (W <= 0 || rows.n <= 0) return PEA_OK;
    ProfScope ps("relu_mask", stream, 0.0);
    const int64_t total = rows.n * (W / 4);
    PEA_LAUNCH(relu_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, rows, W / 4, G, ldg, O, ldo);
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

}  // namespace pea
