"""loss.backward() through the HIP conv stack (reference training step solvers.py:213-216).

    PEAStackFunction.apply(engine, x, n_slots, options, *conv parameters) -> stack [N, P, R]
                                      (the per-metapath representations that models/base.py:193-196 concatenates)

forward  = pea_model_forward_train (all P x S conv layers, softmax statistics kept in the workspace)
backward = per level, last to first:
             pea_model_backward_level  -- the sparse half in HIP: relu masks, bias / attention-vector gradient
                                          reductions, gradient gathers over the reversed relations (csrc/agg_bwd.hip)
             pea_grad_weight / pea_dense_batch on workspace views -- the dense half: dW = In^T dT (row-part MFMA
                                          reduction, fixed order), dIn = dT W and the first layer's dx = dT_0 W_cat (one
                                          deep-K job) on the forward transform kernels: no library GEMM in the step
The fusion and the BPR scorer on top of `stack` are differentiated by torch autograd on the batch's rows only
(models/base.py here: `_loss_autograd`), which is also what lets the last layer's gradient gathers skip every row outside
the batch (StackOptions.read_ids).
"""
import ctypes as C
import os
from collections import Counter

import torch

from . import _lib
from .dense_ops import RowSet, block_sum, dense_batch, grad_weight, mlp2_backward_data, mlp2_backward_data_sage
from .engine import PARAM_SLOTS
from .losses import rows_scatter_sum


class _Layout:
    """Parsed pea_model_describe output (float offsets from the 256-byte aligned workspace base).  Every unit also carries
    its layer index `li` (into the per-layer parameter list); last_unit: {channel: the unit of its last layer, whose o_col is
    the channel's column in the X / dX regions}, in unit order."""

    def __init__(self, engine):
        lib = _lib.load()
        need = C.c_int()
        _lib.check(lib.pea_model_describe(engine._h, None, 0, C.byref(need)))
        buf = (C.c_int64 * need.value)()
        _lib.check(lib.pea_model_describe(engine._h, buf, need.value, C.byref(need)))
        v = list(buf)
        self.n_levels, self.ld_x, self.off_x, self.off_dx, self.off_gpack, self.pack_floats, two_step = v[:7]
        self.two_step_train = bool(two_step)      # csrc/model.h: pea_model::fused2_train
        first = [sum(engine.steps[:p]) for p in range(len(engine.steps))]      # layer index of each channel's first layer
        i = 7
        self.levels, self.last_unit = [], {}
        for _ in range(self.n_levels):
            names = ('ld_t', 'ld_o', 'off_t', 'off_o', 'off_dt', 'off_do', 'off_side', 'bias_off', 'att_src_off',
                     'att_dst_off', 'off_dad', 'off_das', 'ld_k', 'n_units')
            lv = dict(zip(names, v[i:i + 14]))
            i += 14
            units = []
            for _ in range(lv['n_units']):
                un = ('p', 's', 'rel', 'in_w', 'heads', 'F', 'HF', 'last', 'in_col', 't_col', 'o_col', 'b_off', 'ldb',
                      'bias_off')
                u = dict(zip(un, v[i:i + 14]))
                i += 14
                u['li'] = first[u['p']] + u['s']
                if u['last']:
                    self.last_unit[u['p']] = u
                units.append(u)
            lv['units'] = units
            self.levels.append(lv)


def layout_of(engine):
    """The engine's _Layout, parsed on first use."""
    lay = getattr(engine, '_layout', None)
    if lay is None:
        lay = engine._layout = _Layout(engine)
    return lay


def _view(wsf, off, n, ld):
    return wsf[off:off + n * ld].view(n, ld)


class _Slice:
    """Placeholder for a gradient that lives in the packed reduction buffer (materialised once at the end)."""

    def __init__(self, off, n, shape=None):
        self.off, self.n, self.shape = off, n, shape


def _bias(lv, u):
    return _Slice(lv['bias_off'] + u['t_col'], u['HF'])


class _RowSupport:
    """The two-step schedules' sparse backward walks the gradient's support (rows of dT_1 -- SAGE: or of the batch -- holding a
    non-zero, collected at level 1); the first layer's gradient gathers rely on the level-0 gradient regions (dA_0; SAGE: dM_0
    and the root blocks) being zero outside it.  `dirty`: the RowSet whose rows of those regions may be non-zero, None if
    unknown (clear() then zeroes the whole regions).  collect() fills the set that is not dirty; commit(live) runs once level 0
    has enqueued every write into the regions, so a backward aborted in between leaves `dirty` intact or None."""

    def __init__(self, n, device):
        self.n, self.device, self.sets, self.aux, self.dirty = n, device, None, None, None

    def collect(self, table, width, also=None):
        if self.sets is None:
            self.sets = (RowSet(self.n, self.device), RowSet(self.n, self.device))
        spare = self.sets[1] if self.dirty is self.sets[0] else self.sets[0]
        return spare.fill_from(table, width, also=also)

    def batch_flags(self, table, width):
        """Flags of the rows of table [N, ld] with a non-zero in their first `width` columns (a third RowSet)."""
        if self.aux is None:
            self.aux = RowSet(self.n, self.device)
        return self.aux.fill_from(table, width).flags

    def clear(self, regions, width):
        for region in regions:
            if self.dirty is None:
                region.zero_()
            else:
                self.dirty.zero_rows_of(region, width)
        self.dirty = None

    def commit(self, live):
        self.dirty = live


class _Backward:
    """One backward_conv_stack call: the state its level schedules share.  Each schedule method runs one level; its
    kernel-facing code (call order, job tuples) is the schedule's own."""

    def __init__(self, engine, x, layer_params, sparse):
        self.engine, self.x, self.layer_params, self.sparse = engine, x, layer_params, sparse
        self.lib = _lib.load()
        self.lay = layout_of(engine)
        self.kind, self.n, self.wsf = engine.kind, engine.plan.num_nodes, engine._wsf
        # sharded plan: every rank handles the rows it owns; gradient rows the gathers over a reversed relation read from
        # other ranks are filled in between the two halves of a level (sharding.fill_in_*), the row-wise reductions give this
        # rank's SHARE of the parameter gradients (summed over the ranks at the end), dx comes out row-sharded (all-gathered)
        self.plan, self.sharded = plan, sharded = engine.plan, engine.sharded
        self.shard, self.shard3, self.own32 = (plan.layout, plan.shard, plan.own_rows_i32) if sharded else (None, None, None)
        self.to_reduce = []
        self.grads = [[None] * len(PARAM_SLOTS[self.kind]) for _ in range(engine.n_layers)]
        self.dX = self.view(self.lay.off_dx, self.lay.ld_x)
        self.dx = None              # written whole by the level-0 input-gradient job(s)
        self.premasked = set()      # levels whose output gradients were written through a gated product (relu mask applied there)
        self.live = None            # two-step schedules: this step's gradient support (None: dense backward)
        self.rows = getattr(engine, '_row_support', None)
        if self.rows is None:
            self.rows = engine._row_support = _RowSupport(self.n, x.device)
        self.stream = _lib.current_stream()

    def view(self, off, ld):
        return _view(self.wsf, off, self.n, ld)

    def level_views(self, s):
        """Level s's layout, its T, dT and dO regions, its input (x at level 0) and that input's gradient (None at level 0)."""
        lv = self.lay.levels[s]
        T, dT, dO = self.view(lv['off_t'], lv['ld_t']), self.view(lv['off_dt'], lv['ld_t']), self.view(lv['off_do'], max(lv['ld_o'], 4))
        if s == 0:
            return lv, T, dT, dO, self.x, None
        prev = self.lay.levels[s - 1]
        return lv, T, dT, dO, self.view(prev['off_o'], prev['ld_o']), self.view(prev['off_do'], max(prev['ld_o'], 4))

    def level_call(self, level, phase):
        if level in self.premasked:
            phase |= _lib.BWD_PREMASKED
        _lib.check(self.lib.pea_model_backward_level(self.engine._h, level, phase, _lib.ptr(self.engine._ws),
                                                     self.engine.workspace_bytes, self.stream))

    def rev_layout(self, rel):
        return self.plan.source_layouts[self.plan.reverse_of[rel]]

    def write_dX(self, d_stack, active_ids, compact):
        """Gradient of the last-layer outputs, in the internal column order."""
        dX, last, P = self.dX, self.lay.last_unit, self.engine.P
        if compact is not None:
            # the batch's gradient rows go straight into the internal column order, duplicates summed in a fixed order, one launch
            dX.zero_()
            rows_scatter_sum(compact[0], compact[1], P, self.engine.repr_dim, [last[p]['o_col'] for p in range(P)], dX)
        elif active_ids is not None:
            # d_stack is zero outside the rows the loss read: clear once, then move those rows only
            dX.zero_()
            rows = d_stack[active_ids]                                              # [B', P, R]
            for p, u in last.items():
                dX[active_ids, u['o_col']:u['o_col'] + u['HF']] = rows[:, p, :]
        else:
            for p, u in last.items():
                dX[:, u['o_col']:u['o_col'] + u['HF']] = d_stack[:, p, :]

    def collect_support(self, table, width, also=None):          # level 1 of a two-step schedule
        if self.sparse:
            self.live = self.rows.collect(table, width, also=also)
        else:
            self.rows.commit(None)         # a dense step writes every row of the level-0 regions: the invariant starts over
        self.engine._live_rows = self.live

    def level0_call(self):
        """The level-0 HIP half of a two-step schedule over this step's support; then the support is the regions' dirty rows."""
        live = self.live
        ids, count = (None, None) if live is None else (_lib.ptr(live.ids), _lib.ptr(live.count))
        _lib.check(self.lib.pea_model_set_active_rows0(self.engine._h, None, ids, count))
        self.level_call(0, 0)
        self.rows.commit(live)

    def sage_two_step_1(self, batch_flags):
        """Two-step training schedule, SAGE, level 1 (csrc/model_bwd.hip, csrc/mlp2_bwd.hip; forward: mlp2_sage_kernel).  Layer 2
        ran transform first: out = mean_j T_1[j] + R_1[i] with T_1 = H lin_rel1^T, R_1 = H lin_root1^T + bias1."""
        lv, _, dT, _, In_all, _ = self.level_views(1)
        units, dX = lv['units'], self.dX
        self.level_call(1, 0)     # d bias1 = colsum dX;  dT_1 = dX spread over the reversed relations (1 / deg_i each)
        ncol = units[-1]['t_col'] + units[-1]['HF']
        # the rows whose hidden row received a gradient: in-neighbours of the batch's rows (dT_1) and, SAGE having no self
        # loops, the batch's rows themselves (the root term: dX)
        if self.sparse and batch_flags is None:
            batch_flags = self.rows.batch_flags(dX, ncol)
        self.collect_support(dT, ncol, also=batch_flags)
        pairs = []
        for u in units:
            In = In_all[:, u['in_col']:u['in_col'] + u['in_w']]                    # the channel's hidden rows H
            pairs += [(dT[:, u['t_col']:u['t_col'] + u['HF']], In), (dX[:, u['o_col']:u['o_col'] + u['HF']], In)]
        dWs = grad_weight(pairs, rows=self.live)
        for q, u in enumerate(units):
            self.grads[u['li']] = [dWs[2 * q], _bias(lv, u), dWs[2 * q + 1]]

    def sage_two_step_0(self):
        """Two-step training schedule, SAGE, level 0."""
        lv, T, dT, dO, x, _ = self.level_views(0)
        units, emb, n, plan, live = lv['units'], x.shape[1], self.n, self.plan, self.live
        nxt = self.lay.levels[1]
        dT1, H = self.view(nxt['off_dt'], nxt['ld_t']), self.view(lv['off_o'], lv['ld_o'])
        side = self.view(lv['off_side'], lv['ld_t'])                               # the root term's gradient blocks
        u1_of = {u1['p']: u1 for u1 in nxt['units']}
        # dM_0 and the root blocks are zero outside this step's list (_RowSupport): the reverse aggregation needs no per-row test
        if live is not None:
            self.rows.clear((dT, side), len(units) * emb)
        zeros = getattr(self.engine, '_zeros_n', None)
        if zeros is None:
            zeros = self.engine._zeros_n = torch.zeros(n, dtype=torch.float32, device=x.device)
        chans, pairs = [], []
        n_rel, prev_rel = 0, None
        for u in units:
            c, u1 = u['t_col'], u1_of[u['p']]
            if u['rel'] != prev_rel:           # one mean per distinct first relation, shared by its channels (model.hip)
                n_rel, prev_rel = n_rel + 1, u['rel']
            a0 = (n_rel - 1) * emb
            w_rel0, _b0, w_root0 = self.layer_params[u['li']]
            w_rel1, _b1, w_root1 = self.layer_params[u['li'] + 1]
            chans.append((w_rel0, w_root0, w_rel1, w_root1, u1['t_col'], u1['o_col'], u['o_col'], c, c, c))
            # d lin_rel0 = dZ_0^T M_0 (the mean of a row without incoming edges is 0: its stale A_0 row is swapped for
            # 0 * x), d lin_root0 = dZ_0^T x
            pairs += [(dO[:, c:c + u['HF']], T[:, a0:a0 + emb], plan.edgeless_mask(u['rel']), x, zeros),
                      (dO[:, c:c + u['HF']], x)]
        mlp2_backward_data_sage(chans, emb, units[0]['HF'], u1_of[units[0]['p']]['HF'], dT1, self.dX, H, dO, dT, side, rows=live)
        dWs = grad_weight(pairs, rows=live)
        self.level0_call()          # d bias0; per channel: dM_0 spread over the reversed relation + the root block -> over A_0
        self.dx = block_sum(T, len(units), emb)
        for q, u in enumerate(units):
            self.grads[u['li']] = [dWs[2 * q], _bias(lv, u), dWs[2 * q + 1]]

    def two_step_0(self):
        """Two-step training schedule, GAT (one head) / GCN, level 0 (csrc/model.h: fused2_train; single GPU).  dO_0 holds dZ_0,
        the gradient of the first transform's pre-activations (masked by the gated product above); A_0 (T_0 region) holds
        the aggregates of the rows with incoming edges (the others' input is x itself).  Dense half on views: dW_0 = dZ_0^T
        A_0 and dA_0 = dZ_0 W_0 per channel; then ONE call runs the softmax passes in x space (bias gradient, D pass, S pass
        -> per-channel dx parts over A_0).  Level 1 ran in `level`."""
        lv, T, dT, dO, x, _ = self.level_views(0)
        units, emb, plan, live, lp = lv['units'], x.shape[1], self.plan, self.live, self.layer_params
        # data path of the dense half in ONE launch (csrc/mlp2_bwd.hip): dZ_0 = (dT_1 W_1) masked by H > 0 -> dO_0 region,
        # dA_0 = dZ_0 W_0 -> dT_0 region, the hidden gradient tile staying in registers between the two products
        nxt = self.lay.levels[1]
        dT1, H = self.view(nxt['off_dt'], nxt['ld_t']), self.view(lv['off_o'], lv['ld_o'])
        u1_of = {u1['p']: u1 for u1 in nxt['units']}
        chans, pairs, gcn = [], [], self.kind == 'gcn'
        from_col = self.engine._gcn_from_col if gcn else False
        for u in units:
            c, u1 = u['t_col'], u1_of[u['p']]
            chans.append((lp[u['li']][0], lp[u['li'] + 1][0], u1['t_col'], u['o_col'], c, c))
            # dW_0 = dZ_0^T In ([HF, emb] = GAT lin.weight's layout; GCN's weight is its transpose); In = A_0 where the node
            # has incoming edges, x where not (GCN: x times the self-loop norm deg^-1)
            pair = (dO[:, c:c + u['HF']], T[:, c:c + emb], plan.edgeless_mask(u['rel']), x)
            pairs.append(pair + (plan.gcn_self_norm(u['rel'], from_col),) if gcn else pair)
        # dA_0 is zero on every row outside this step's list (_RowSupport), so the gradient gathers below need no per-edge
        # test: 3/4 of the rows they fetch are live, and a test per edge costs more than the quarter of the fetches it saves
        # -- GAT S pass 1.12 -> 1.23 ms, GCN reverse aggregation 1.47 -> 1.75, SAGE 0.82 -> 1.09 on the 25m-shaped graph
        # (profiles/r03/bwd0_filter_r03.txt; the filtered variant was removed)
        if live is not None:
            self.rows.clear((dT,), len(units) * emb)
        mlp2_backward_data(chans, emb, units[0]['HF'], u1_of[units[0]['p']]['HF'], dT1, H, dO, dT, rows=live, weights_in_out=gcn)
        dWs = grad_weight(pairs, rows=live)
        self.level0_call()
        n_ch = len(units)
        self.dx = block_sum(T, n_ch, emb)                                        # the S pass wrote the channels' parts over A_0
        if gcn:                      # no attention vectors: weight [in, out] = the transpose of the reduced block, bias
            for q, u in enumerate(units):
                self.grads[u['li']] = [dWs[q].t(), _bias(lv, u)]
            return
        das, dad = self.view(lv['off_das'], lv['ld_k']), self.view(lv['off_dad'], lv['ld_k'])
        d_ws, d_wd = grad_weight([(das, x), (dad, x)])                           # [ld_k, emb]: rows = channels in unit order
        d_ws, d_wd = d_ws[:n_ch], d_wd[:n_ch]
        # the logits came from x . ws, x . wd with ws = W_0^T att_j, wd = W_0^T att_i: chain rule, batched over the channels
        W = torch.stack([lp[u['li']][0] for u in units])                         # [P, HF, emb]
        att_i = torch.stack([lp[u['li']][1].reshape(-1) for u in units])          # [P, HF]
        att_j = torch.stack([lp[u['li']][2].reshape(-1) for u in units])
        d_att_j = torch.bmm(W, d_ws.unsqueeze(2)).squeeze(2)
        d_att_i = torch.bmm(W, d_wd.unsqueeze(2)).squeeze(2)
        dW0 = torch.stack(dWs)
        dW0.addcmul_(att_j.unsqueeze(2), d_ws.unsqueeze(1)).addcmul_(att_i.unsqueeze(2), d_wd.unsqueeze(1))
        for q, u in enumerate(units):
            shape = lp[u['li']][1].shape
            self.grads[u['li']] = [dW0[q], d_att_i[q].view(shape), d_att_j[q].view(shape), _bias(lv, u)]

    def sage_level(self, s):
        """Level-wise SAGE: phase 0 (relu masks, bias), the dense half, phase 1 (reverse mean aggregation of dM)."""
        lv, T, dT, dO, In_all, dIn_all = self.level_views(s)
        x, n, dX, lp, units = self.x, self.n, self.dX, self.layer_params, lv['units']
        self.level_call(s, 0)
        dT.zero_()
        pairs, jobs, root_jobs = [], [], []
        shared = Counter(u['t_col'] for u in units)
        for u in units:
            w_rel, _b, w_root = lp[u['li']]
            G = (dX if u['last'] else dO)[:, u['o_col']:u['o_col'] + u['HF']]
            M = T[:, u['t_col']:u['t_col'] + u['in_w']]
            In = In_all[:, u['in_col']:u['in_col'] + u['in_w']]
            pairs += [(G, M), (G, In)]
            self.grads[u['li']][1] = _Slice(u['bias_off'], u['HF'])
            if shared[u['t_col']] == 1:                                   # its own mean block: dM = G W_rel, written in place
                jobs.append((G, w_rel, dT[:, u['t_col']:u['t_col'] + u['in_w']]))
            else:                                                         # level 0: channels of one relation share M
                tmp = torch.empty((n, u['in_w']), dtype=torch.float32, device=x.device)
                jobs.append((G, w_rel, tmp))
                shared.setdefault('acc', []).append((u, tmp))
            if s > 0:
                root_jobs.append((G, w_root, dIn_all[:, u['in_col']:u['in_col'] + u['in_w']]))
        dWs = grad_weight(pairs, shard=self.shard3)
        self.to_reduce.extend(dWs)
        for q, u in enumerate(units):
            self.grads[u['li']][0], self.grads[u['li']][2] = dWs[2 * q], dWs[2 * q + 1]
        if s == 0:
            # dx = sum_u G_u W_root_u (+ the mean-path gradient below): one deep-K job when the G blocks are the
            # contiguous columns of dO (every 2-step model), else one job per channel and a sum
            cont = sorted((u for u in units if not u['last']), key=lambda u: u['o_col'])
            ocols = sum(u['HF'] for u in cont)
            contiguous = len(cont) == len(units) and all(
                cont[k]['o_col'] == sum(v['HF'] for v in cont[:k]) for k in range(len(cont)))
            self.dx = torch.empty_like(x)
            if contiguous:
                w_cat = torch.cat([lp[u['li']][2] for u in cont], dim=0)   # [ocols, emb]
                root_jobs.append((dO[:, :ocols], w_cat, self.dx))
            else:
                parts = torch.empty((len(units),) + tuple(x.shape), dtype=torch.float32, device=x.device)
                for q, u in enumerate(units):
                    G = (dX if u['last'] else dO)[:, u['o_col']:u['o_col'] + u['HF']]
                    root_jobs.append((G, lp[u['li']][2], parts[q]))
        dense_batch(jobs + root_jobs, rows=self.own32)
        if s == 0 and not contiguous:
            torch.sum(parts, dim=0, out=self.dx)
        for u, tmp in shared.get('acc', []):
            dT[:, u['t_col']:u['t_col'] + u['in_w']] += tmp
        if self.sharded:     # the reverse mean aggregation gathers dM rows of the forward relation's destinations
            seen, items = set(), []
            for u in units:
                if u['t_col'] not in seen:
                    seen.add(u['t_col'])
                    items.append((dT, u['t_col'], u['in_w'], self.rev_layout(u['rel'])))
            self.shard.fill_in_rows_batch(items)         # one exchange for the level
        self.level_call(s, 1)
        dagg = self.view(lv['off_side'], lv['ld_t'])
        done = set()
        for u in units:
            if s == 0:
                if u['t_col'] not in done:
                    self.dx += dagg[:, u['t_col']:u['t_col'] + u['in_w']]
                    done.add(u['t_col'])
            else:
                dIn_all[:, u['in_col']:u['in_col'] + u['in_w']] += dagg[:, u['t_col']:u['t_col'] + u['in_w']]

    def level(self, s, active_ids):
        """Level-wise GAT / GCN, sharded exchanges included; also level 1 of their two-step schedule."""
        lv, _, dT, dO, In_all, dIn_all = self.level_views(s)
        x, dX, lp, kind, shard, units = self.x, self.dX, self.layer_params, self.kind, self.shard, lv['units']
        two_step_1 = self.lay.two_step_train and s == 1
        self.level_call(s, 0)
        if self.sharded:
            # runs of adjacent channels on one relation: their output-gradient columns (and GAT side records) travel together
            side = self.view(lv['off_side'], 4 * max(sum(u['heads'] for u in units), 1)) if kind == 'gat' else None
            runs, a_k = [], 0
            for u in units:
                r = runs[-1] if runs else None
                if r and r['rel'] == u['rel'] and r['last'] == u['last'] and r['col'] + r['w'] == u['o_col']:
                    r['w'] += u['HF']
                    r['heads'] += u['heads']
                else:
                    runs.append(dict(rel=u['rel'], last=u['last'], col=u['o_col'], w=u['HF'], a_k=a_k, heads=u['heads']))
                a_k += u['heads']
            # rows every rank owns are complete rows: the batch's rows of the last level travel whole (one all-reduce per
            # buffer instead of one per run of channels), the other levels' runs in one batched exchange
            batch_items, ids_done = [], False
            for r in runs:
                G = dX if r['last'] else dO
                if r['last'] and active_ids is not None:       # only the batch's rows carry a gradient at the last layer
                    if not ids_done:
                        shard.fill_in_ids(dX, 0, dX.shape[1], active_ids)
                        if side is not None:
                            shard.fill_in_ids(side, 0, side.shape[1], active_ids)
                        ids_done = True
                else:
                    batch_items.append((G, r['col'], r['w'], self.rev_layout(r['rel'])))
                    if side is not None:
                        batch_items.append((side, 4 * r['a_k'], 4 * r['heads'], self.rev_layout(r['rel'])))
            shard.fill_in_rows_batch(batch_items)
            self.level_call(s, 2)
        if s == 0:
            # every first-layer channel reads x: one GEMM for all weight gradients, one for dx
            ncol = units[-1]['t_col'] + units[-1]['HF']
            dT0 = dT[:, :ncol]
            self.dx = torch.empty_like(x)
            if kind == 'gat':
                dW_all = grad_weight([(dT0, x)], shard=self.shard3)[0]           # [sum HF, emb]
                w_cat = torch.cat([lp[u['li']][0] for u in units], dim=0)
            else:
                dW_all = grad_weight([(x, dT0)], shard=self.shard3)[0]           # [emb, sum F]
                w_cat = torch.cat([lp[u['li']][0] for u in units], dim=1).t().contiguous()
            self.to_reduce.append(dW_all)
            dense_batch([(dT0, w_cat, self.dx)], rows=self.own32)                # dx = dT_0 W_cat: one deep-K job (K = sum HF)
        else:
            # weight gradients of the level in one launch pair, input gradients in one launch (dense_bwd.hip).
            # dIn = dT W is the output gradient of the level below BEFORE its relu mask; In (= that level's relu output)
            # is the mask: applied in the product's epilogue when every job qualifies (k <= 128, more than 16 outputs:
            # the persistent transform kernel), so that level's own mask pass over the buffer is skipped
            gated = all(u['HF'] <= 128 and u['in_w'] > 16 for u in units)
            pairs, dense = [], []
            for u in units:
                dTu = dT[:, u['t_col']:u['t_col'] + u['HF']]
                In = In_all[:, u['in_col']:u['in_col'] + u['in_w']]
                dIn = dIn_all[:, u['in_col']:u['in_col'] + u['in_w']]
                W = lp[u['li']][0] if kind == 'gat' else lp[u['li']][0].t().contiguous()      # dT @ W
                pairs.append((dTu, In) if kind == 'gat' else (In, dTu))                        # GAT [HF, in], GCN [in, F]
                dense.append((dTu, W, dIn) + ((In,) if gated else ()))
            if two_step_1:
                # Gradient support: the loss read the batch's rows only, so dT_1 is identically zero outside the batch rows and
                # their layer-2 in-neighbours (about 1/4 of the nodes on the 25m-shaped graph).  The dense half of both layers
                # and the first layer's gradient gathers walk that row set (built on the device, count never read by the host).
                self.collect_support(dT, units[-1]['t_col'] + units[-1]['HF'])      # all channels' columns of dT_1
            dWs = grad_weight(pairs, shard=self.shard3, rows=self.live)
            self.to_reduce.extend(dWs)
            if not two_step_1:      # two-step training: the level-0 schedule runs both products fused
                dense_batch(dense, rows=self.own32)
            if gated:
                self.premasked.add(s - 1)
        for q, u in enumerate(units):
            cols, g = slice(u['t_col'], u['t_col'] + u['HF']), self.grads[u['li']]
            g[0] = dWs[q] if s > 0 else dW_all[cols] if kind == 'gat' else dW_all[:, cols]
            g[-1] = _bias(lv, u)
            if kind == 'gat':
                shape = lp[u['li']][1].shape
                g[1], g[2] = (_Slice(lv['att_dst_off'] + u['t_col'], u['HF'], shape),
                              _Slice(lv['att_src_off'] + u['t_col'], u['HF'], shape))

    def finish(self):
        """The small (bias / attention-vector) gradients were reduced into the packed buffer level by level: one copy of it,
        then views (the workspace itself is overwritten by the next step)."""
        lay = self.lay
        packed = self.wsf[lay.off_gpack:lay.off_gpack + lay.pack_floats].clone()
        if self.sharded:
            self.shard.all_reduce_sum_(self.to_reduce + [packed])      # the ranks' shares of every parameter gradient, one collective
            self.shard.allgather_rows(self.dx)                         # dx rows are complete on their owners
        for g in self.grads:
            for q, item in enumerate(g):
                if isinstance(item, _Slice):
                    t = packed[item.off:item.off + item.n]
                    g[q] = t if item.shape is None else t.view(item.shape)
        return self.dx, self.grads


def backward_conv_stack(engine, d_stack, x, layer_params, active_ids=None, compact=None, batch_flags=None):
    """Gradients of sum(stack * d_stack) wrt x and every conv parameter.  Returns (dx, [tuple per layer]).
    compact = (ids, rows): d_stack given as the gradient rows [len(ids), P * R] of the stack rows `ids` (int64; duplicates
    are summed in position order, ids < 0 skipped) instead of a dense [N, P, R] tensor (PEALossFunction).
    batch_flags (uint8 [N], optional): 1 on the rows of the stack that can carry a gradient."""
    if not engine.enable_backward:
        raise RuntimeError('engine was built without enable_backward')
    b = _Backward(engine, x, layer_params, os.environ.get('PEA_SPARSE_BWD', '1') != '0')
    b.write_dX(d_stack, active_ids, compact)
    two_step, sage = b.lay.two_step_train, engine.kind == 'sage'
    for s in range(b.lay.n_levels - 1, -1, -1):
        if sage and two_step:
            b.sage_two_step_1(batch_flags) if s == 1 else b.sage_two_step_0()
        elif sage:
            b.sage_level(s)
        elif two_step and s == 0:
            b.two_step_0()
        else:
            b.level(s, active_ids)
    return b.finish()


def param_layers(flat, n_slots):
    """The flat parameter list of an autograd Function as one tuple per layer."""
    return [tuple(flat[i:i + n_slots]) for i in range(0, len(flat), n_slots)]


def save_params(ctx, x, flat):
    """Save x and the parameters that are present (None slots cannot be saved)."""
    ctx.save_for_backward(x, *[t for t in flat if t is not None])
    ctx.present = [t is not None for t in flat]


def saved_params(ctx):
    """(x, flat parameter list with its None slots) as save_params left them."""
    x, *rest = ctx.saved_tensors
    it = iter(rest)
    return x, [next(it) if p else None for p in ctx.present]


def param_grads(layer_params, grads):
    """backward_conv_stack's gradients, flat and shaped like their parameters (None for an absent one)."""
    return [None if t is None else g.reshape(t.shape) for lp, gl in zip(layer_params, grads) for t, g in zip(lp, gl)]


def _forward_options(engine, options, x):
    """The call's StackOptions and what the by-product fused table is fused with (zeros by default)."""
    options = options or StackOptions()
    return options, torch.zeros(engine.P, engine.repr_dim, device=x.device) if options.fuse_att is None else options.fuse_att


def _stack_backward(ctx, d_stack, active_ids, **kw):
    """(dx, flat parameter gradients) of backward_conv_stack, with ctx.active_rows set on the engine for its duration."""
    x, flat = saved_params(ctx)
    layer_params = param_layers(flat, ctx.n_slots)
    lib, mask = _lib.load(), ctx.active_rows        # uint8 [N] or None: rows of the final outputs that can carry a gradient
    with torch.no_grad():
        if mask is not None:
            _lib.check(lib.pea_model_set_active_rows(ctx.engine._h, _lib.ptr(mask)))
        try:
            dx, grads = backward_conv_stack(ctx.engine, d_stack, x, layer_params, active_ids, **kw)
        finally:
            if mask is not None:
                _lib.check(lib.pea_model_set_active_rows(ctx.engine._h, None))
    return dx, param_grads(layer_params, grads)


class StackOptions:
    """Per-call options of PEAStackFunction (a plain object: autograd passes it through untouched).
    fuse_att / fuse_masked: what the by-product fused table (`fused`, set by the forward) is fused with (None: zeros).
    read_ids: the only rows of the returned stack the caller will read (int64 ids, duplicates allowed): only they can
    carry a gradient, so the backward moves just those rows of d_stack and (GAT) lets the last layer's gradient gathers
    skip every other row."""

    def __init__(self, fuse_att=None, fuse_masked=None, read_ids=None):
        self.fuse_att, self.fuse_masked, self.read_ids = fuse_att, fuse_masked, read_ids
        self.fused = None


class PEAStackFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, x, n_slots, options, *flat):
        # the fused table of the same launch is a free by-product (not differentiated here: the caller fuses the rows
        # it needs with torch ops on the stack)
        options, att = _forward_options(engine, options, x)
        # sharded: each rank keeps the rows it owns (fused table and stack are defined there only); the caller exchanges
        # the rows it reads (models/base.py: _loss_autograd)
        options.fused, stack = engine.forward(param_layers(flat, n_slots), x, att=att, masked=options.fuse_masked,
                                              want_stack=True, train=True, gather=False)
        ctx.engine, ctx.n_slots = engine, n_slots
        ctx.active_ids, ctx.active_rows = options.read_ids, None
        if options.read_ids is not None:      # (every kind: the last layer's gradient gathers skip the rows not flagged)
            ctx.active_rows = torch.zeros(x.shape[0], dtype=torch.uint8, device=x.device).index_fill_(0, options.read_ids, 1)
        save_params(ctx, x, flat)
        return stack

    @staticmethod
    def backward(ctx, d_stack):
        dx, out = _stack_backward(ctx, d_stack.contiguous(), ctx.active_ids)
        return (None, dx, None, None, *out)


class PEALossFunction(torch.autograd.Function):
    """The whole training-step loss of a PEA model as ONE autograd node: conv stack forward (HIP), the batch's stack rows,
    fusion + scorer + BPR loss with their backward (csrc/bpr_train.hip), and in backward() the batch's gradient rows
    scattered straight into the output-gradient buffer (pea_rows_scatter_sum) before the conv stack's HIP backward.
    Compared with PEAStackFunction + torch ops on top, autograd never builds the dense [N, P, R] gradient of the stack
    (two 158 MB fills, a sort-based index backward and nine index_puts per step on the 25m-shaped graph).
    Reference: solvers.py:213-214 (loss = model.loss(batch); loss.backward())."""

    @staticmethod
    def forward(ctx, engine, x, n_slots, options, ids, att, fc1_w, fc1_b, fc2_w, fc2_b, *flat):
        from .engine import bpr_train_raw       # looked up per call: tests wrap it to see that the loss runs through it
        options, fuse_att = _forward_options(engine, options, x)
        # The loss reads the batch's stack rows only: they are picked from the workspace's X region (the last layer's outputs in
        # the schedule's own column order) instead of having the fusion launch write the whole [N, P, R] stack for them
        # (158 MB on the 25m-shaped graph: 0.083 -> 0.045 ms for that launch)
        options.fused = engine.forward(param_layers(flat, n_slots), x, att=fuse_att, masked=options.fuse_masked,
                                       want_stack=False, train=True, gather=False)
        lay = layout_of(engine)
        if getattr(engine, '_stack_cols', None) is None:
            engine._stack_cols = torch.tensor([lay.last_unit[p]['o_col'] + r for p in range(engine.P) for r in range(engine.repr_dim)],
                                              dtype=torch.int64, device=x.device)
        cols = engine._stack_cols
        table = _view(engine._wsf, lay.off_x, x.shape[0], lay.ld_x)
        if engine.sharded:
            # every rank holds the stack rows it owns: the batch's rows are summed from their owners (one all-reduce of
            # [3B, P * R], exact: x + 0); the head is computed replicated; only owned rows receive a gradient here
            layout = engine.plan.layout
            picked = layout.gather_rows(table, ids).index_select(1, cols)
            ids_b = torch.where(layout.owner(ids) == layout.rank, ids, torch.full_like(ids, -1))
        else:
            picked, ids_b = table.index_select(0, ids).index_select(1, cols), ids
        loss, grad_rows, head = bpr_train_raw(picked.view(-1, engine.P, engine.repr_dim), att, fc1_w, fc1_b, fc2_w, fc2_b)
        ctx.engine, ctx.n_slots, ctx.ids, ctx.ids_b = engine, n_slots, ids, ids_b
        ctx.grad_rows, ctx.head = grad_rows, head
        # the batch's rows: the only rows of the last layer's output gradient that are non-zero (GAT: D / S passes; GCN and
        # SAGE: the reverse aggregation does not fetch the others; two-step SAGE: part of the gradient's support)
        ctx.active_rows = torch.zeros(x.shape[0], dtype=torch.uint8, device=x.device).index_fill_(0, ids, 1)
        save_params(ctx, x, flat)
        return loss

    @staticmethod
    def backward(ctx, g):
        # the conv stack's backward is linear in the batch's gradient rows: the upstream gradient scales them once
        # ([3B, P * R]) instead of every one of the ~80 parameter gradients afterwards
        dx, out = _stack_backward(ctx, None, ctx.ids, compact=(ctx.ids_b, ctx.grad_rows * g), batch_flags=ctx.active_rows)
        head = tuple(None if t is None else t * g for t in ctx.head)
        return (None, dx, None, None, None) + head + tuple(out)
