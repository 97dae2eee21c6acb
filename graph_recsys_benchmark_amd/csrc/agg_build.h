// Vocabulary of the schedule host code (model.hip, model_bwd.hip): how an AggGroup over a relation is put together and
// launched, and the small lookups both directions of the schedule share.  Host code only.
#pragma once
#include <algorithm>

#include "model.h"

namespace pea {

// `a` (default: an empty group) with the row lists and counts of relation R
inline AggGroup agg_over(const Relation &R, AggGroup a = AggGroup{}) {
    a.rowptr = R.rowptr;
    a.col = R.col;
    a.short_rows = R.short_rows;
    a.long_items = R.long_items;
    a.hub_rows = R.hub_rows;
    a.hub_first = R.hub_first;
    a.hub_count = R.hub_count;
    a.n_short = R.n_short;
    a.n_long = R.n_long;
    a.n_hub = R.n_hub;
    return a;
}

// rows without a kept edge come first in R's short-row list: leave them out
inline void skip_edgeless(AggGroup &a, const Relation &R) {
    a.short_rows = R.short_rows + R.n_short0;
    a.n_short = R.n_short - R.n_short0;
}

// sharded, level >= 1: the gather sources arrive through an exchange buffer, addressed by slot instead of node id
inline void gather_from_exchange(AggGroup &a, const Relation &R, const float *buf, int ld) {
    a.col = R.col_slot;
    a.feat = buf;
    a.ld_feat = ld;
}

// rows of the table a group's gathers read: the relation's source-id span, or every slot of its exchange buffer
inline double table_rows(const Relation &R, const pea_plan *plan, bool via_slots) {
    return via_slots ? (double)R.slots_per_rank * plan->shard_world : (double)R.src_span;
}

// Roofline bookkeeping of a group over R (the launch log carries it).  loops = 1.0 where every visited row also reduces
// its own self-loop message (forward GAT / GCN on a plan with self loops), else 0.0; call it AFTER skip_edgeless: the
// short launch counts the rows it visits.
inline void set_traffic(AggGroup &a, const Relation &R, double loops, double idx_share, double rows_of_table) {
    a.msgs_short = (double)R.edges_short + loops * a.n_short;
    a.msgs_long = (double)R.edges_long + loops * R.n_direct;
    a.idx_share = idx_share;
    a.table_rows = rows_of_table;
}

// every group of `gs`, at most kMaxAggGroups per launch; the backward modes go to the backward kernels' launcher
inline int launch_groups(AggMode mode, const std::vector<AggGroup> &gs, hipStream_t stream) {
    const bool bwd = mode == AGG_GAT_BWD_D || mode == AGG_GAT_BWD_S || mode == AGG_SUM_BWD_S;
    for (size_t b = 0; b < gs.size(); b += kMaxAggGroups) {
        const int n = (int)std::min<size_t>(kMaxAggGroups, gs.size() - b);
        PEA_TRY(bwd ? launch_gat_backward(mode, gs.data() + b, n, stream) : launch_aggregate(mode, gs.data() + b, n, stream));
    }
    return PEA_OK;
}

// The two buffers a level's columns live in: X for the channels that end at the level, O_s for those that continue
// (relu between the steps; on X only where the caller asks).  Values, their gradients (dX / dO_s) and the backward's
// view of the outputs all split the same way.
struct Dest {
    float *ptr;
    int ld, relu;
};
struct LevelOut {
    float *X;
    int ld_x;
    float *O;
    int ld_o;
    int relu_last;
    Dest at(bool last, int col) const { return last ? Dest{X + col, ld_x, relu_last} : Dest{O + col, ld_o, 1}; }
};

// the unit of channel p on level L (null: the channel has no step there)
inline const Unit *unit_of_channel(const Level &L, int p) {
    for (const Unit &u : L.units)
        if (u.p == p) return &u;
    return nullptr;
}

// The relation a backward gather of `rel` walks -- its reverse -- checked, together with the room of the group's hub
// partials: records of W columns (F per head) from float `partial_off` of the partial buffer, for whichever of the two
// relations has more hub chunks.  *span (optional): the floats they may take.
inline int reverse_relation(const pea_model *m, int rel, size_t partial_off, int W, int F, const Relation **reversed,
                            size_t *span) {
    const int rr = m->reverse_of[(size_t)rel];
    PEA_REQUIRE(rr >= 0, PEA_ERR_ARG, "backward: relation %d has no reversed relation in the plan", rel);
    const Relation &R = m->plan->rels[(size_t)rel], &Rr = m->plan->rels[(size_t)rr];
    const size_t floats = (size_t)std::max(R.n_slots, Rr.n_slots) * partial_record_floats(W, F);
    PEA_REQUIRE(partial_off + floats <= m->partial_floats, PEA_ERR_NOMEM,
                "backward: hub partial buffer too small for relation %d and its reverse", rel);
    *reversed = &Rr;
    if (span) *span = floats;
    return PEA_OK;
}

// Backward of a linear aggregation (GCN's normalised sum, SAGE's mean): the same weighted sum over the REVERSED relation,
//   out_j = dinv_self_j * sum_{i: j -> i} dinv_i feat_i   (+ the row's own term where the caller sets self_loop),
// dinv / dinv_self node-indexed weights of the gathered and of the written row.  The caller adds what differs: the own
// row (feat_self), self_loop, partial, the batch's row flags, bookkeeping.
inline AggGroup reverse_wsum(const Relation &Rr, int W, int F, const float *feat, int ld_feat, const float *dinv,
                             const float *dinv_self, float *out, int ld_out) {
    AggGroup a = agg_over(Rr);
    a.W = W;
    a.F = F;
    a.feat = feat;
    a.ld_feat = ld_feat;
    a.feat_self = feat;
    a.ld_self = ld_feat;
    a.dinv = dinv;
    a.dinv_self = dinv_self;
    a.out = out;
    a.ld_out = ld_out;
    return a;
}

}  // namespace pea
