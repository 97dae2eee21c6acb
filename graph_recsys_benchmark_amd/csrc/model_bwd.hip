// Backward of one level of the PEA schedule (training; reference solvers.py:215 loss.backward()).
// The sparse half -- gradient gathers over the reversed relations, relu masks, bias / attention-vector gradient
// reductions -- runs here; the dense half (dW = In^T dT, dIn = dT W: plain GEMMs) is done by the host mirror with
// rocBLAS through torch.mm on views of the same workspace (graph_recsys_benchmark_amd/autograd.py).
//
// Workspace regions (model.h): dX [N, ld_x] gradient of the last-layer outputs (internal column order), per level
// dO_s [N, ld_o] gradient of the relu(conv) outputs, dT_s [N, ld_t] gradient of the transformed features (SAGE: of the
// neighbour means), side_s / dad_s / das_s GAT per-head records, gpack: bias / att gradients at the SAME offsets as
// their values in the weight pack.
#include "agg_build.h"

namespace pea {
namespace {

__global__ void fill_kernel(int64_t n, float v, float *p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// bits[w] = bit b set where flags[32 w + b] != 0
__global__ void flags_to_bits_kernel(int64_t N, const unsigned char *__restrict__ flags, unsigned *__restrict__ bits) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = n < N && flags[n] != 0;
    const unsigned long long b = __ballot(on);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && n < N) bits[n >> 5] = (unsigned)b;
    if (lane == 32 && n < N) bits[n >> 5] = (unsigned)(b >> 32);
}

__global__ void invdeg_kernel(int64_t N, const int *__restrict__ rowptr, float *__restrict__ out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int d = rowptr[v + 1] - rowptr[v];
    out[v] = 1.0f / (float)(d < 1 ? 1 : d);
}

int ensure_sage_arrays(pea_plan *plan, int rel, hipStream_t stream) {
    const int64_t N = plan->N;
    if (!plan->ones) {
        PEA_HIP(hipMalloc((void **)&plan->ones, (size_t)N * sizeof(float)));
        PEA_LAUNCH(fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, 1.0f, plan->ones);
    }
    Relation &R = plan->rels[(size_t)rel];
    if (!R.invdeg) {
        PEA_HIP(hipMalloc((void **)&R.invdeg, (size_t)N * sizeof(float)));
        PEA_LAUNCH(invdeg_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, R.rowptr, R.invdeg);
    }
    PEA_HIP(hipGetLastError());
    return PEA_OK;
}

// What every schedule of the backward of one level reads, derived once per call.
struct Bwd {
    pea_model *m;
    pea_plan *plan;
    const Level &L;
    int level;
    hipStream_t stream;
    float *wsf, *pack, *gpack, *colsum_part, *partial;
    float *T, *O, *X, *dT, *dO, *dX;
    bool loops, sharded;
    RowMap own;            // the rows this rank owns: what every row-wise reduction walks
    LevelOut grads, outs;  // the level's output gradients (dX | dO_s) and outputs (X | O_s), split like the forward's outputs

    Bwd(pea_model *model, int lvl, float *ws, hipStream_t s)
        : m(model), plan(const_cast<pea_plan *>(model->plan)), L(model->levels[(size_t)lvl]), level(lvl), stream(s), wsf(ws),
          pack(ws), gpack(ws + model->off_gpack), colsum_part(ws + model->off_colsum), partial(ws + model->off_partial),
          T(ws + L.off_t), O(ws + L.off_o), X(ws + model->off_x), dT(ws + L.off_dt), dO(ws + L.off_do), dX(ws + model->off_dx),
          loops((plan->flags & PEA_PLAN_SELF_LOOPS) != 0), sharded(plan->shard_world > 1),
          own(make_rowmap(plan->N, plan->shard_tile, plan->shard_world, plan->shard_rank)),
          grads{dX, model->ld_x, dO, L.ld_o, 0}, outs{X, model->ld_x, O, L.ld_o, 0} {}
    // level 0 of the two-step schedule: the rows whose gradient is not identically zero, when the host listed them
    RowMap live_rows() const {
        return m->active0_list ? make_rowmap_list(plan->N, m->active0_list, m->active0_count, plan->N) : own;
    }
    int bias_gradient(const RowMap &rows, int W, const float *G, int ldg, size_t bias_off) const {
        return launch_colsum(rows, W, W, G, ldg, nullptr, 0, 1.0f, colsum_part, gpack + bias_off, stream);
    }
};

// The batch's row flags (pea_model_set_active_rows) as a bitmap: the gathers over the reversed relation test one flag
// per GATHERED row, and as a bitmap the flags of all nodes fit a CU's L1 (AggGroup::row_active_bits)
int build_active_bits(const Bwd &b, const unsigned **bits) {
    pea_model *m = b.m;
    const int64_t N = b.plan->N;
    if (!m->active_bits) PEA_HIP(hipMalloc((void **)&m->active_bits, (size_t)((N + 63) / 64) * 2 * sizeof(unsigned)));
    PEA_LAUNCH(flags_to_bits_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b.stream, N, m->active_rows, m->active_bits);
    PEA_HIP(hipGetLastError());
    *bits = m->active_bits;
    return PEA_OK;
}

// Two-step training schedule, SAGE (forward: model.hip two_step_stage0 / mlp2_sage_kernel).  Layer 2 is transform
// first -- out = mean_j T_1[j] + R_1[i], T_1 = H lin_rel1^T, R_1 = H lin_root1^T + bias1 -- so its backward is a
// 16-wide gather:   level 1:  d bias1 = colsum dX;  dT_1[j] = sum_{i: j -> i} dX[i] / deg_i  (reversed relation).
// Level 0 (x space; the host mirror has run csrc/mlp2_bwd.hip: dZ_0 in dO_0, dM_0 = dZ_0 lin_rel0 per channel in the
// dT_0 region, the root term's gradient dZ_0 lin_root0 per channel in the side region):  d bias0 = colsum dZ_0 over
// the live rows;  per channel  dXp_j = sum_{i: j -> i} dM_0[i] / deg_i + (dZ_0 lin_root0)[j]  written over A_0 (dead
// once the weight gradients have read the means); the host sums the channel blocks into dx.
int sage_two_step_1(const Bwd &b) {
    const pea_model *m = b.m;
    const Level &L = b.L;
    PEA_TRY(b.bias_gradient(b.own, L.n_cols, b.dX, m->ld_x, L.bias_off));
    const unsigned *active_bits = nullptr;   // only the batch's rows of dX are non-zero: the others are not fetched (csrc/agg_bwd.hip)
    if (m->active_rows) PEA_TRY(build_active_bits(b, &active_bits));
    std::vector<AggGroup> gs;
    for (const GroupPlan &g : L.groups) {
        const Relation *Rr;
        PEA_TRY(reverse_relation(m, g.rel, g.partial_off, g.W, g.F, &Rr, nullptr));
        PEA_REQUIRE(g.last && g.out_col == g.col, PEA_ERR_ARG, "backward: two-step SAGE expects X in the T_1 column order");
        PEA_TRY(ensure_sage_arrays(b.plan, g.rel, b.stream));
        // weights: 1 / max(deg_i, 1) of the gathered (forward destination) node
        AggGroup a = reverse_wsum(*Rr, g.W, g.W, b.dX + g.out_col, m->ld_x, b.plan->rels[(size_t)g.rel].invdeg, b.plan->ones,
                                  b.dT + g.col, L.ld_t);
        a.row_active = m->active_rows;
        a.row_active_bits = active_bits;
        a.partial = b.partial + g.partial_off;
        set_traffic(a, *Rr, 0.0, 1.0, table_rows(*Rr, b.plan, false));
        gs.push_back(a);
    }
    // with the batch's row flags: the batch-sparse walk of the backward kernels (only flagged rows are fetched)
    return launch_groups(m->active_rows ? AGG_SUM_BWD_S : AGG_GCN, gs, b.stream);
}

int sage_two_step_0(const Bwd &b) {
    const pea_model *m = b.m;
    const Level &L = b.L;
    const int E0 = m->d.emb_dim;
    PEA_TRY(b.bias_gradient(b.live_rows(), L.n_cols, b.dO, L.ld_o, L.bias_off));
    std::vector<AggGroup> gs;
    size_t part_off = 0, span = 0;
    for (size_t ui = 0; ui < L.units.size(); ++ui) {
        const Unit &u = L.units[ui];
        const Relation *Rr;
        PEA_TRY(reverse_relation(m, u.rel, part_off, E0, E0, &Rr, &span));
        PEA_TRY(ensure_sage_arrays(b.plan, u.rel, b.stream));
        AggGroup a = reverse_wsum(*Rr, E0, E0, b.dT + ui * E0, L.ld_t, b.plan->rels[(size_t)u.rel].invdeg, b.plan->ones,
                                  b.T + ui * E0, L.ld_t);
        a.feat_self = b.wsf + L.off_side + ui * E0;   // the root term's gradient rides as the row's own term (weight 1)
        a.self_loop = 1;
        a.partial = b.partial + part_off;
        part_off += span;
        set_traffic(a, *Rr, 0.0, 1.0, table_rows(*Rr, b.plan, false));
        gs.push_back(a);
    }
    return launch_groups(AGG_GCN, gs, b.stream);
}

// SAGE in the reference's order.  phase 0: relu masks + bias gradients; phase 1: reverse mean aggregation of dM_s
// (written by the host into the dT_s region) -> side_s region
int sage_level(const Bwd &b, int phase) {
    const Level &L = b.L;
    if (phase == 0) {
        for (const Unit &u : L.units) {
            const Dest G = b.grads.at(u.last, u.o_col);
            if (!u.last) PEA_TRY(launch_relu_mask(b.own, u.HF, G.ptr, G.ld, b.outs.at(u.last, u.o_col).ptr, G.ld, b.stream));
            PEA_TRY(b.bias_gradient(b.own, u.HF, G.ptr, G.ld, u.bias_off));
        }
        return PEA_OK;
    }
    std::vector<AggGroup> gs;
    for (const GroupPlan &g : L.groups) {
        const Relation *Rr;
        PEA_TRY(reverse_relation(b.m, g.rel, g.partial_off, g.W, g.W, &Rr, nullptr));
        PEA_TRY(ensure_sage_arrays(b.plan, g.rel, b.stream));
        // dM columns of this group -> gradient wrt the gathered input columns, M_s column layout
        AggGroup a = reverse_wsum(*Rr, g.W, g.W, b.dT + g.out_col, L.ld_t, b.plan->rels[(size_t)g.rel].invdeg, b.plan->ones,
                                  b.wsf + L.off_side + g.out_col, L.ld_t);
        a.partial = b.partial + g.partial_off;
        gs.push_back(a);
    }
    return launch_groups(AGG_GCN, gs, b.stream);
}

// Two-step training schedule, first layer of GAT / GCN, in x space.  Inputs (host mirror: autograd.py): dO_0 = dZ_0, the
// gradient of the first transform's pre-activations (relu mask applied by the gated product that wrote it); dA_0 = dZ_0 W_0
// in the dT_0 region; A_0 (the aggregates of the rows with incoming edges) in the T_0 region; the forward's softmax
// statistics.  Here: the bias gradient, the D pass (destination rows, gathers x rows, c_i = dA_i . A_i), the S pass (source
// rows over the reversed relation, gathers dA_i and the side records; per channel
// dXp_j = sum_i alpha_ij dA_i + ws d a_src_j + wd d a_dst_j  with ws / wd = W_0^T att_j / att_i) -- written over A_0, which
// is dead once the D pass has read it.  The host then sums the channel blocks into dx and reduces d ws / d wd (d a_src /
// d a_dst against x).
// GCN: the aggregation is linear, its backward is the same weighted sum over the REVERSED relation, in x space:
// dXp_j = sum_i dinv_j dinv_i dA_i + dinv_j^2 dA_j (norm of the forward relation: GCNConv)
int two_step_0(const Bwd &b) {
    const pea_model *m = b.m;
    const pea_model_desc &d = m->d;
    const Level &L = b.L;
    PEA_REQUIRE(m->last_x != nullptr, PEA_ERR_ARG, "backward: no training forward ran on this model");
    const float *xin = m->last_x;
    const int ldx = (int)m->last_ldx;
    const int E0 = d.emb_dim;
    float *wsf = b.wsf, *A0 = b.T, *dA0 = b.dT;
    PEA_MEMSET_ASYNC(wsf + L.off_dad, 0, (size_t)b.plan->N * (size_t)L.ld_k * sizeof(float), b.stream);
    PEA_TRY(b.bias_gradient(b.live_rows(), L.n_cols, b.dO, L.ld_o, L.bias_off));
    std::vector<AggGroup> gd, gs;
    size_t part_off = 0, span = 0;
    for (size_t ui = 0; ui < L.units.size(); ++ui) {
        const Unit &u = L.units[ui];
        const Relation *Rr;
        PEA_TRY(reverse_relation(m, u.rel, part_off, E0, E0, &Rr, &span));
        Relation &R = b.plan->rels[(size_t)u.rel];
        float *dA = dA0 + ui * E0, *A = A0 + ui * E0;   // the channel's blocks
        if (d.kind == PEA_KIND_GCN) {
            const bool fc = d.gcn_deg_from_col != 0;
            PEA_TRY(ensure_dinv(b.plan, u.rel, fc, b.stream));
            const float *dinv = fc ? R.dinv_col : R.dinv_row;
            AggGroup a = reverse_wsum(*Rr, E0, E0, dA, L.ld_t, dinv, dinv, A, L.ld_t);
            a.self_loop = 1;
            a.partial = b.partial + part_off;
            part_off += span;
            set_traffic(a, *Rr, 0.0, 1.0, table_rows(*Rr, b.plan, false));
            gs.push_back(a);
            continue;
        }
        AggGroup a{};
        a.W = E0;
        a.F = E0;
        a.neg_slope = d.negative_slope;
        a.self_loop = 1;
        a.partial = b.partial + part_off;
        part_off += span;
        a.att_src = b.pack + m->mlp2_att_off + (size_t)2 * ui * E0;   // ws = W_0^T att_j (mlp2_pack_kernel)
        a.att_dst = a.att_src + E0;                                  // wd = W_0^T att_i
        a.ld_side = L.ld_side;
        a.ld_k = L.ld_k;
        a.ld_g = L.ld_t;
        a.row_active = m->active0;   // D: rows with a zero gradient are not gathered for; S: their rows are not gathered
        AggGroup D = agg_over(R, a);
        skip_edgeless(D, R);         // edge-less rows: not visited (no side record, d a_dst = 0)
        D.feat = xin;
        D.ld_feat = ldx;
        D.feat_self = xin;
        D.ld_self = ldx;
        D.g_self = dA;
        D.o_self = A;
        D.stats = wsf + L.off_stats + 2 * (int)ui;
        D.ld_stats = L.ld_stats;
        D.side_out = wsf + L.off_side + 4 * (int)ui;
        D.ksum = wsf + L.off_dad + (int)ui;
        set_traffic(D, R, 0.0, 0.0, table_rows(R, b.plan, false));
        gd.push_back(D);
        AggGroup S = agg_over(*Rr, a);
        S.feat = dA;
        S.ld_feat = L.ld_t;
        S.feat_self = xin;
        S.ld_self = ldx;
        S.side = wsf + L.off_side + 4 * (int)ui;
        S.da_dst = wsf + L.off_dad + (int)ui;
        S.ksum = wsf + L.off_das + (int)ui;
        S.out = A;
        S.ld_out = L.ld_t;
        S.deg0_self = R.deg0;
        set_traffic(S, *Rr, 0.0, 0.0, table_rows(*Rr, b.plan, false));
        gs.push_back(S);
    }
    PEA_TRY(launch_groups(AGG_GAT_BWD_D, gd, b.stream));
    return launch_groups(d.kind == PEA_KIND_GCN ? AGG_GCN : AGG_GAT_BWD_S, gs, b.stream);
}

// relu between the steps (reference models/base.py:138): the output gradient of the channels that continue is masked
// in place, one launch per run of groups whose columns are contiguous in dO (a 2-step model's first level: the whole row)
int mask_continuing(const Bwd &b) {
    const Level &L = b.L;
    size_t ri = 0;
    while (ri < L.groups.size()) {
        const GroupPlan &g0 = L.groups[ri];
        size_t rj = ri + 1;
        int W = g0.W;
        while (!g0.last && rj < L.groups.size() && !L.groups[rj].last && L.groups[rj].out_col == g0.out_col + W) W += L.groups[rj++].W;
        if (!g0.last) PEA_TRY(launch_relu_mask(b.own, W, b.dO + g0.out_col, L.ld_o, b.O + g0.out_col, L.ld_o, b.stream));
        ri = rj;
    }
    return PEA_OK;
}

// Gradient reductions of a GAT / GCN level, one launch per run of groups whose columns (and heads) are contiguous:
//   d bias[c] = sum_n g[n, c];   d att_j[c] = sum_n d a_src[n, head(c)] T[n, c];   d att_i likewise with d a_dst
int reduce_level(const Bwd &b, bool part_a, bool part_b) {
    const Level &L = b.L;
    size_t gi = 0;
    while (gi < L.groups.size()) {
        const GroupPlan &g0 = L.groups[gi];
        size_t gj = gi + 1;
        int W = g0.W;
        while (gj < L.groups.size() && L.groups[gj].last == g0.last && L.groups[gj].F == g0.F &&
               L.groups[gj].col == g0.col + W && L.groups[gj].out_col == g0.out_col + W)
            W += L.groups[gj++].W;
        const Dest G = b.grads.at(g0.last, g0.out_col);
        if (part_a) PEA_TRY(b.bias_gradient(b.own, W, G.ptr, G.ld, g0.bias_off));
        if (b.m->d.kind == PEA_KIND_GAT) {
            const float *Tg = b.T + g0.col;
            float *das = b.wsf + L.off_das + g0.a_k, *dad = b.wsf + L.off_dad + g0.a_k;
            float *d_att_src = b.gpack + L.att_src_off + g0.col, *d_att_dst = b.gpack + L.att_dst_off + g0.col;
            if (part_a && part_b) {  // one GPU: both attention-vector gradients weight T_s: one pass over it
                PEA_TRY(launch_colsum2(b.own, W, g0.F, Tg, L.ld_t, das, dad, L.ld_k, 1.0f, b.colsum_part, d_att_src, d_att_dst, b.stream));
            } else {
                if (part_b) PEA_TRY(launch_colsum(b.own, W, g0.F, Tg, L.ld_t, das, L.ld_k, 1.0f, b.colsum_part, d_att_src, b.stream));
                if (part_a) PEA_TRY(launch_colsum(b.own, W, g0.F, Tg, L.ld_t, dad, L.ld_k, 1.0f, b.colsum_part, d_att_dst, b.stream));
            }
        }
        gi = gj;
    }
    return PEA_OK;
}

// A GAT / GCN level, level-wise.  On one GPU phase 0 runs both parts; sharded, phase 0 = part a and phase 2 = part b
// (see pea_model_backward_level):
//   part a: masks, D pass, reductions over what own rows already hold
//   part b: gathers over the reversed relation, reductions of their results
int level_wise(const Bwd &b, bool part_a, bool part_b, bool premasked) {
    const pea_model *m = b.m;
    const pea_model_desc &d = m->d;
    const Level &L = b.L;
    float *wsf = b.wsf;
    const bool via_slots = b.sharded && b.level > 0;  // the gather sources of this level sit in the forward's exchange buffer (slot order)
    if (d.kind == PEA_KIND_GAT && part_a) {
        // rows whose softmax is their self loop alone are skipped by the D pass (alpha = 1, d z = 0): their d a_dst reads 0
        PEA_MEMSET_ASYNC(wsf + L.off_dad, 0, (size_t)b.plan->N * (size_t)L.ld_k * sizeof(float), b.stream);
    }
    if (part_a && !premasked) PEA_TRY(mask_continuing(b));
    // only the final outputs' gradient is known to be batch-sparse
    // (GCN: the reverse aggregation skips the gathered rows known to be zero, csrc/agg_bwd.hip: AGG_SUM_BWD_S)
    const unsigned *active_bits = nullptr;
    if (m->active_rows && part_b && std::any_of(L.groups.begin(), L.groups.end(), [](const GroupPlan &g) { return g.last; }))
        PEA_TRY(build_active_bits(b, &active_bits));
    std::vector<AggGroup> gd, gsrc, gsrc_batch;
    for (const GroupPlan &g : L.groups) {
        const Relation *Rr;
        PEA_TRY(reverse_relation(m, g.rel, g.partial_off, g.W, g.F, &Rr, nullptr));
        Relation &R = b.plan->rels[(size_t)g.rel];
        const Dest G = b.grads.at(g.last, g.out_col);
        float *partial = b.partial + g.partial_off;  // every group its own region (sized for the relation and its reverse: slots_of)
        if (d.kind == PEA_KIND_GCN) {
            const bool fc = d.gcn_deg_from_col != 0;
            PEA_TRY(ensure_dinv(b.plan, g.rel, fc, b.stream));
            const float *dinv = fc ? R.dinv_col : R.dinv_row;
            AggGroup a = reverse_wsum(*Rr, g.W, g.F, G.ptr, G.ld, dinv, dinv, b.dT + g.col, L.ld_t);
            a.neg_slope = d.negative_slope;
            a.self_loop = b.loops ? 1 : 0;
            a.partial = partial;
            if (g.last && active_bits) {   // only the batch's rows of dX are non-zero: the batch-sparse walk (agg_bwd.hip)
                a.row_active = m->active_rows;
                a.row_active_bits = active_bits;
                if (part_b) gsrc_batch.push_back(a);
            } else if (part_b) {
                gsrc.push_back(a);
            }
            continue;
        }
        AggGroup a{};
        a.W = g.W;
        a.F = g.F;
        a.neg_slope = d.negative_slope;
        a.self_loop = b.loops ? 1 : 0;
        a.partial = partial;
        a.att_src = b.pack + L.att_src_off + g.col;
        a.att_dst = b.pack + L.att_dst_off + g.col;
        a.bias = b.pack + g.bias_off;
        a.ld_side = L.ld_side;
        a.ld_k = L.ld_k;
        a.ld_g = G.ld;
        a.row_active = g.last ? m->active_rows : nullptr;
        a.row_active_bits = g.last ? active_bits : nullptr;
        // D pass: destination rows of the forward relation, gathers T_j
        AggGroup D = agg_over(R, a);
        D.feat = b.T + g.col;
        D.ld_feat = L.ld_t;
        D.feat_self = D.feat;
        D.ld_self = L.ld_t;
        D.g_self = G.ptr;
        D.o_self = b.outs.at(g.last, g.out_col).ptr;
        D.stats = wsf + L.off_stats + 2 * g.a_k;
        D.ld_stats = L.ld_stats;
        D.side_out = wsf + L.off_side + 4 * g.a_k;
        D.ksum = wsf + L.off_dad + g.a_k;
        if (via_slots) {
            PEA_REQUIRE(R.col_slot != nullptr && g.xch_ld > 0, PEA_ERR_ARG, "backward: relation %d has no exchange layout", g.rel);
            gather_from_exchange(D, R, wsf + g.xch_off, g.xch_ld);
        }
        if (b.loops) skip_edgeless(D, R);  // edge-less rows: not visited (no side record, d a_dst = 0)
        set_traffic(D, R, 0.0, 0.0, table_rows(R, b.plan, via_slots));   // bookkeeping for the live roofline (agg_bwd.hip: launch_bwd_g)
        if (part_a) gd.push_back(D);
        // S pass: source rows = destination rows of the reversed relation, gathers g_i and the side records
        AggGroup S = agg_over(*Rr, a);
        S.feat = G.ptr;
        S.ld_feat = G.ld;
        S.feat_self = b.T + g.col;
        S.ld_self = L.ld_t;
        S.side = wsf + L.off_side + 4 * g.a_k;
        S.da_dst = wsf + L.off_dad + g.a_k;
        S.ksum = wsf + L.off_das + g.a_k;
        S.out = b.dT + g.col;
        S.ld_out = L.ld_t;
        S.deg0_self = b.loops ? R.deg0 : nullptr;
        set_traffic(S, *Rr, 0.0, 0.0, table_rows(*Rr, b.plan, false));
        if (part_b) gsrc.push_back(S);
    }
    // all groups of the level side by side in one set of launches per pass (the S pass of a group reads what the D pass
    // of the same group wrote: every D launch precedes every S launch on the stream)
    PEA_TRY(launch_groups(AGG_GAT_BWD_D, gd, b.stream));
    PEA_TRY(launch_groups(d.kind == PEA_KIND_GCN ? AGG_GCN : AGG_GAT_BWD_S, gsrc, b.stream));
    PEA_TRY(launch_groups(AGG_SUM_BWD_S, gsrc_batch, b.stream));   // GCN, last layer
    return reduce_level(b, part_a, part_b);
}

}  // namespace
}  // namespace pea

using namespace pea;

// Level 0 of the two-step training schedule: the rows whose input gradient of the first transform is not identically zero
// (pea_rows_nonzero of dT_1): the softmax passes skip the others (their dA_0 rows are never written), the bias gradient walks
// the list.  NULL flags: every row.
extern "C" int pea_model_set_active_rows0(pea_model *m, const unsigned char *flags, const int32_t *list, const int32_t *count_dev) {
    PEA_REQUIRE(m, PEA_ERR_ARG, "set_active_rows0: null model");
    PEA_REQUIRE((list == nullptr) == (count_dev == nullptr) && (flags == nullptr || list != nullptr), PEA_ERR_ARG,
                "set_active_rows0: a list comes with its count, flags with the list");
    m->active0 = flags;              // NULL with a list: the gathers run over every row (dA_0 is zero outside the list)
    m->active0_list = list;
    m->active0_count = count_dev;
    return PEA_OK;
}

extern "C" int pea_model_set_active_rows(pea_model *m, const unsigned char *row_active) {
    PEA_REQUIRE(m, PEA_ERR_ARG, "set_active_rows: null model");
    m->active_rows = row_active;
    return PEA_OK;
}

// phase 0: relu masks + bias gradients (all kinds); GAT/GCN: the aggregation backward -> dT_s (+ att gradients)
// phase 1: SAGE only: reverse mean aggregation of dM_s (written by the host into the dT_s region) -> side_s region
// Sharded plans (one rank's rows): the gradient gathers over the REVERSED relation read output-gradient rows (and GAT
// side records) of destination nodes other ranks own, so GAT/GCN phase 0 stops before them -- relu masks, GAT D pass,
// bias / att_i reductions over own rows -- the host fills those rows in from their owners (sharding.fill_in_rows on
// the node-indexed dX / dO_s / side_s buffers), and
// phase 2 runs the rest: GAT S pass / GCN reverse aggregation -> dT_s on own rows, att_j reduction.  (SAGE: the host
// fills in dM_s rows between phase 0 and phase 1.)  Every row-wise reduction walks the rank's own rows (RowMap).
// The four schedules are the ones the host mirror names (autograd.py: sage_two_step_*, sage_level, two_step_0, level).
extern "C" int pea_model_backward_level(pea_model *m, int level, int phase, void *workspace, size_t workspace_bytes,
                                        void *stream_) {
    PEA_REQUIRE(m && workspace && m->backward, PEA_ERR_ARG, "backward: model without enable_backward");
    const bool premasked = (phase & PEA_BWD_PREMASKED) != 0;   // the producer of this level's output gradients applied the relu mask
    phase &= ~PEA_BWD_PREMASKED;
    PEA_REQUIRE(level >= 0 && level < (int)m->levels.size() && phase >= 0 && phase <= 2, PEA_ERR_ARG, "backward: level %d phase %d", level, phase);
    PEA_REQUIRE(workspace_bytes >= pea_model_workspace_bytes(m), PEA_ERR_NOMEM, "backward: workspace too small");
    const Bwd b(m, level, aligned_ws(workspace), (hipStream_t)stream_);
    const bool sage = m->d.kind == PEA_KIND_SAGE;
    if (m->fused2_train && (sage || level == 0)) {
        PEA_REQUIRE(phase == 0 && !b.sharded && (!sage || level <= 1), PEA_ERR_ARG,
                    "backward: the two-step training schedule is single-GPU, phase 0");
        return !sage ? two_step_0(b) : level == 1 ? sage_two_step_1(b) : sage_two_step_0(b);
    }
    if (sage) {
        PEA_REQUIRE(phase <= 1, PEA_ERR_ARG, "backward: SAGE levels have phases 0 and 1");
        return sage_level(b, phase);
    }
    PEA_REQUIRE(phase == 0 || phase == 2, PEA_ERR_ARG, "backward: GAT/GCN levels have phases 0 and (sharded) 2");
    PEA_REQUIRE(phase == 0 || b.sharded, PEA_ERR_ARG, "backward: phase 2 is the second half of a SHARDED level");
    return level_wise(b, phase == 0, phase == 2 || !b.sharded, premasked);
}

// Flat description of the schedule for the host mirror (all offsets in floats from the 256-byte aligned workspace base):
//   [0] n_levels  [1] ld_x  [2] off_x  [3] off_dx  [4] off_gpack  [5] pack_floats  [6] two-step training schedule (0 / 1)
//   then per level  ld_t ld_o off_t off_o off_dt off_do off_side bias_off att_src_off att_dst_off off_dad off_das ld_k n_units,
//   then per unit
//   p s rel in_w heads F HF last in_col t_col o_col b_off ldb bias_off
extern "C" int pea_model_describe(const pea_model *m, int64_t *out, int max_len, int *needed) {
    PEA_REQUIRE(m && needed, PEA_ERR_ARG, "describe: null");
    std::vector<int64_t> v = {(int64_t)m->levels.size(), m->ld_x, (int64_t)m->off_x, (int64_t)m->off_dx,
                              (int64_t)m->off_gpack, (int64_t)m->pack_floats, m->fused2_train ? 1 : 0};
    for (const Level &L : m->levels) {
        const int64_t head[] = {L.ld_t, L.ld_o, (int64_t)L.off_t, (int64_t)L.off_o, (int64_t)L.off_dt, (int64_t)L.off_do,
                                (int64_t)L.off_side, (int64_t)L.bias_off, (int64_t)L.att_src_off, (int64_t)L.att_dst_off,
                                (int64_t)L.off_dad, (int64_t)L.off_das, (int64_t)L.ld_k, (int64_t)L.units.size()};
        v.insert(v.end(), head, head + 14);
        for (const Unit &u : L.units) {
            const int64_t un[] = {u.p, u.s, u.rel, u.in_w, u.heads, u.F, u.HF, u.last ? 1 : 0, u.in_col, u.t_col, u.o_col,
                                  (int64_t)u.b_off, u.ldb, (int64_t)u.bias_off};
            v.insert(v.end(), un, un + 14);
        }
    }
    *needed = (int)v.size();
    if (out && max_len >= (int)v.size()) std::copy(v.begin(), v.end(), out);
    return PEA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Weighted neighbour sum with caller-supplied per-edge weights (the message/aggregate half of the reference's own
// baseline convs: graph_recsys_benchmark/nn/kgat_conv.py:36-44, nn/kgcn_conv.py:32-37 `x_j * att_map`, and
// nn/ngcf_conv.py:42-45 with coff folded to a per-edge weight):   out_i = sum_{e: j -> i} w_e x_j.
// The plan must have been created with PEA_PLAN_EDGE_IDS (weights are in the caller's COO order).
// ---------------------------------------------------------------------------------------------------------------
extern "C" size_t pea_weighted_aggregate_workspace_bytes(const pea_plan *plan, int relation, int width) {
    if (!plan || relation < 0 || relation >= (int)plan->rels.size() || width <= 0) return 0;
    size_t fl = 0;
    for (int c = 0; c < width; c += 256) fl += (size_t)plan->rels[(size_t)relation].n_slots * partial_record_floats(std::min(256, width - c), std::min(256, width - c));
    return fl * sizeof(float) + 512;
}

extern "C" int pea_weighted_aggregate(const pea_plan *plan, int relation, int width, const float *x, int64_t ldx,
                                      const float *edge_weight, float *out, int64_t ldo, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    PEA_REQUIRE(plan && relation >= 0 && relation < (int)plan->rels.size(), PEA_ERR_ARG, "weighted_aggregate: bad relation");
    const Relation &R = plan->rels[(size_t)relation];
    PEA_REQUIRE(R.eid != nullptr || R.e_kept == 0, PEA_ERR_ARG, "weighted_aggregate: the plan was created without PEA_PLAN_EDGE_IDS");
    PEA_REQUIRE(x && out && (edge_weight || R.e_kept == 0), PEA_ERR_ARG, "weighted_aggregate: null argument");
    PEA_REQUIRE(width > 0 && width % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= width && ldo >= width, PEA_ERR_ARG,
                "weighted_aggregate: width %d and row strides must be multiples of 4", width);
    PEA_REQUIRE(workspace_bytes >= pea_weighted_aggregate_workspace_bytes(plan, relation, width), PEA_ERR_NOMEM,
                "weighted_aggregate: workspace too small");
    float *partial = aligned_ws(workspace);
    std::vector<AggGroup> gs;
    for (int c = 0; c < width; c += 256) {
        AggGroup a = agg_over(R);
        a.eid = R.eid;
        a.edge_w = edge_weight;
        a.W = std::min(256, width - c);
        a.F = a.W;
        a.feat = x + c;
        a.ld_feat = (int)ldx;
        a.feat_self = a.feat;
        a.ld_self = (int)ldx;
        a.out = out + c;
        a.ld_out = (int)ldo;
        a.partial = partial;
        partial += (size_t)R.n_slots * partial_record_floats(a.W, a.F);
        gs.push_back(a);
    }
    return launch_groups(AGG_WSUM, gs, (hipStream_t)stream);
}
