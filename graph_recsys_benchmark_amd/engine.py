"""Host side of the HIP path: graph plan + whole-model schedule behind the reference's module surface.

    GraphPlan  <-  the P x S list of int64 COO tensors built by update_pea_graph_input
                   (reference graph_recsys_benchmark/utils/general_utils.py:280-395)
    PEAEngine  <-  PEABaseRecsysModel.forward (reference models/base.py:191-206) for one conv kind

PyTorch is used for device memory and streams only; all arithmetic runs in libpeahip.so.

Also the facade of the host side: callers reach errors.py, dense_ops.py, scoring.py, losses.py and walk_ops.py as engine.X.
"""
import ctypes as C

import torch

from . import _lib
from .dense_ops import (  # noqa: F401
    RowSet, _rows2d, block_sum, dense_batch, grad_weight, mlp2_backward_data, mlp2_backward_data_sage)
from .errors import _pending_err, _pending_what, check as check_pending_errors, defer as _defer_error  # noqa: F401
from .losses import (  # noqa: F401
    DOT_TRAIN_MAX_BLOCKS, HEREC_MAX_TABLES, ROWS_SCATTER_MAX, _block16, _BprTrainLoss, _CfkgLoss, _DotBprLoss, _herec_args,
    _HerecLoss, _int64_batch, _scatter_dense, _TransrLoss, bpr_train_loss, bpr_train_raw, bpr_train_supported, cfkg_loss,
    cfkg_supported, cfkg_train_raw, dot_bpr_loss, dot_bpr_supported, dot_bpr_train_raw, herec_mse_loss, herec_supported,
    herec_table, herec_train_raw, nfm_mse_loss, nfm_position_ids, nfm_supported, nfm_train_raw, rows_scatter_sum, transr_loss,
    transr_supported, transr_train_raw)
from .scoring import (  # noqa: F401
    _catalogue_args, _check_scored, _dot_table, _entity_launch, _EntityReg, _rank_io, bpr_score, dot_predict, dot_rank_eval,
    dot_rank_full, dot_rank_full_multi, dot_recommend_topk, entity_reg, fuse_ablate, predict, rank_eval, rank_eval_multi, rank_full,
    rank_full_multi, recommend_topk, NfmFolded, nfm_fold, nfm_fold_torch, nfm_predict, nfm_rank_eval, nfm_score_block,
    nfm_rank_full, nfm_rank_full_multi, nfm_recommend_topk, nfm_scan_splits, nfm_scan_supported)
from .sharding import ShardLayout
from .walk_ops import (  # noqa: F401
    _SkipgramLoss, _walk_rows, _walk_starts, metapath_walks, skipgram_loss, skipgram_supported, skipgram_train_raw, uniform_walks)

KINDS = {'gat': _lib.KIND_GAT, 'gcn': _lib.KIND_GCN, 'sage': _lib.KIND_SAGE}
GRAPHS_ENABLED = True     # bench.py clears it for its per-kernel HIP-event pass (events are not part of a captured graph)


def _shard_replay_mode():
    import os
    mode = os.environ.get('PEA_SHARD_REPLAY', 'tape')
    return mode if mode in ('tape', 'graph', 'eager') else 'tape'

# parameter slots per conv layer, in the order pea_model_forward expects (include/peahip.h)
PARAM_SLOTS = {
    'gat': ('lin.weight', 'att_i', 'att_j', 'bias'),
    'gcn': ('weight', 'bias'),
    'sage': ('lin_rel.weight', 'lin_rel.bias', 'lin_root.weight'),
}


def _fingerprint(ei):
    e = ei.shape[1]
    if e == 0:
        return (0, 0)
    idx = torch.arange(e, device=ei.device, dtype=torch.int64)
    h = (ei[0] * 1000003 + ei[1] * 998244353 + idx * 7919).sum()
    return (e, int(h.item()))


class GraphPlan:
    """Destination-sorted CSR + degree bins for every DISTINCT relation of a metapath list.

    Equal-content tensors are planned once: update_pea_graph_input creates a fresh
    torch.flip(user2item) copy per use (utils/general_utils.py:300-307), so dedupe is by content.
    """

    def __init__(self, num_nodes, meta_path_edge_index_list, self_loops, shard_rank=0, shard_world=1,
                 shard_tile=256, gather_row_bytes=256, with_reverse=False):
        lib = _lib.require_device()
        self.num_nodes = int(num_nodes)
        self.self_loops = bool(self_loops)
        self.shard = (int(shard_rank), int(shard_world), int(shard_tile))
        uniq, keys = [], {}
        self.relation_of = []
        for eil in meta_path_edge_index_list:
            row = []
            for ei in eil:
                if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64:
                    raise ValueError('edge_index must be an int64 [2, E] tensor, got %s %s' % (ei.dtype, tuple(ei.shape)))
                if not ei.is_cuda:
                    raise RuntimeError('edge_index must live on the GPU (the HIP path has no CPU fallback)')
                ei = ei.contiguous()
                fp = _fingerprint(ei)
                found = None
                for cand in keys.get(fp, []):
                    if torch.equal(uniq[cand], ei):
                        found = cand
                        break
                if found is None:
                    found = len(uniq)
                    uniq.append(ei)
                    keys.setdefault(fp, []).append(found)
                row.append(found)
            self.relation_of.append(row)
        # training: the backward gathers run over the REVERSED relations; add the ones the model does not use itself
        self.reverse_of = None
        if with_reverse:
            self.reverse_of = []
            for r in range(len(uniq)):
                flipped = torch.flip(uniq[r], dims=[0]).contiguous()
                fp = _fingerprint(flipped)
                found = None
                for cand in keys.get(fp, []):
                    if torch.equal(uniq[cand], flipped):
                        found = cand
                        break
                if found is None:
                    found = len(uniq)
                    uniq.append(flipped)
                    keys.setdefault(fp, []).append(found)
                self.reverse_of.append(found)
            # reversed relations appended above get their own entry too (reverse of a reverse is the original)
            for r in range(len(self.reverse_of), len(uniq)):
                self.reverse_of.append(next(i for i, rr in enumerate(self.reverse_of) if rr == r))
        self.num_relations = len(uniq)
        self._uniq = uniq
        ptrs = (C.c_void_p * len(uniq))(*[t.data_ptr() for t in uniq])
        nedge = (C.c_int64 * len(uniq))(*[t.shape[1] for t in uniq])
        handle = C.c_void_p()
        _lib.check(lib.pea_plan_create(self.num_nodes, len(uniq), ptrs, nedge,
                                       _lib.PLAN_SELF_LOOPS if self_loops else 0, int(gather_row_bytes), self.shard[0],
                                       self.shard[1], self.shard[2], _lib.current_stream(), C.byref(handle)))
        self._h = handle
        self.device = uniq[0].device
        self.layout = ShardLayout(self.num_nodes, *self.shard)
        self.source_layouts = {}
        if self.shard[1] > 1:
            lays = [self.layout.source_layout(ei) for ei in uniq]
            # owned rows, the ones OTHER ranks read first: the sources of the relations used at a step >= 1 (the exchanges
            # between the stages move exactly these rows).  A stage computes them first, the all-gather starts, and the rest
            # of the stage (rows only this rank reads) runs behind it (pea_model_forward_part).
            own64 = self.layout.owned_rows(self.device)
            later = sorted({r for row in self.relation_of for r in row[1:]})
            is_src = torch.zeros(self.num_nodes, dtype=torch.bool, device=self.device)
            for r in later:
                is_src[lays[r].src_nodes] = True
            first = is_src[own64]
            own = torch.cat([own64[first], own64[~first]]).to(torch.int32).contiguous()
            self.own_rows_i32 = own
            self.n_own_first = int(first.sum().item())
            _lib.check(lib.pea_plan_set_owned_rows(handle, _lib.ptr(own), own.numel(), _lib.current_stream()))
            _lib.check(lib.pea_plan_set_owned_split(handle, self.n_own_first))
            # relations with few source nodes (attribute -> item ...) share ONE first-layer row list: own rows + the
            # union of their sources, so their channels' transforms run as one wide job (a few extra rows, same results)
            small = [r for r, lay in enumerate(lays) if lay.src_nodes.numel() * 10 <= own.numel()]
            if len(small) > 1:
                shared = torch.unique(torch.cat([self.layout.owned_rows(self.device)] +
                                                [lays[r].src_nodes for r in small])).to(torch.int32)
                for r in small:
                    lays[r].need_rows = shared
            for r, lay in enumerate(lays):
                need = lay.need_rows.contiguous()
                _lib.check(lib.pea_plan_set_sources(handle, r, _lib.ptr(lay.slot_of_node.contiguous()), lay.slots_per_rank,
                                                    _lib.ptr(need), need.numel(), _lib.current_stream()))
                self.source_layouts[r] = lay

    def relation_info(self, r):
        info = (C.c_int64 * 9)()
        _lib.check(_lib.load().pea_plan_relation_info(self._h, r, info))
        names = ('edges', 'max_degree', 'short_rows', 'long_items', 'hub_rows', 'hub_chunks', 'rows_owned', 'edges_owned',
                 'slices')
        return dict(zip(names, [int(v) for v in info]))

    def gcn_self_norm(self, r, from_col=False):
        """float32 [N]: deg^-1 of GCNConv's normalisation under relation r (self loops dropped, one added per node; degree over
        the source index -- PyG 1.5.0 -- or the target index): the weight dinv_i^2 of a node's own row, which is ALL of the
        aggregate of a node without incoming edges.  Built once per relation and degree side."""
        cache = self.__dict__.setdefault('_self_norm', {})
        key = (r, bool(from_col))
        if key not in cache:
            ei = self._uniq[r]
            keep = ei[0] != ei[1]
            idx = ei[1 if from_col else 0][keep]
            deg = torch.bincount(idx, minlength=self.num_nodes).to(torch.float32) + 1.0
            cache[key] = (1.0 / deg).contiguous()
        return cache[key]

    def edgeless_mask(self, r):
        """uint8 [N]: 1 where node n has no kept incoming edge under relation r (GAT / GCN: its conv output is its own
        transformed row; the two-step schedules feed x[n] instead of an aggregate).  Built once per relation."""
        cache = self.__dict__.setdefault('_edgeless', {})
        if r not in cache:
            rowptr, _ = self.export_csr(r)
            cache[r] = (rowptr[1:] == rowptr[:-1]).to(torch.uint8).contiguous()
        return cache[r]

    def export_csr(self, r):
        info = self.relation_info(r)
        rowptr = torch.empty(self.num_nodes + 1, dtype=torch.int32, device=self.device)
        col = torch.empty(max(info['edges'], 1), dtype=torch.int32, device=self.device)
        _lib.check(_lib.load().pea_plan_export_csr(self._h, r, _lib.ptr(rowptr), _lib.ptr(col), _lib.current_stream()))
        return rowptr, col[:info['edges']]

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.load().pea_plan_destroy(h)
            except Exception:
                pass


class PEAEngine:
    """One scheduled PEA forward: P channels x S conv layers of one kind, then fusion."""

    def __init__(self, plan, kind, steps, emb_dim, hidden_size, repr_dim, heads=1, channel_aggr='att',
                 gcn_deg_from='row', negative_slope=0.2, enable_backward=False):
        if channel_aggr not in ('att', 'mean'):
            # 'concat' cannot work in the reference either (models/base.py:175 sizes fc1 for 'cat')
            raise NotImplementedError('Other aggr methods not implemeted!')
        if kind not in KINDS:
            raise ValueError(kind)
        if gcn_deg_from not in ('row', 'col'):
            raise ValueError(gcn_deg_from)
        lib = _lib.require_device()
        self.plan, self.kind = plan, kind
        self.steps = [int(s) for s in steps]
        if len(self.steps) != len(plan.relation_of) or any(len(r) != s for r, s in zip(plan.relation_of, self.steps)):
            raise AssertionError('meta_path_steps does not match the edge index lists')
        self.P = len(self.steps)
        self.repr_dim, self.emb_dim = int(repr_dim), int(emb_dim)
        self.channel_aggr = channel_aggr
        flat = [r for row in plan.relation_of for r in row]
        self._steps_c = (C.c_int * self.P)(*self.steps)
        self._rel_c = (C.c_int * len(flat))(*flat)
        self.enable_backward = bool(enable_backward)
        self._gcn_from_col = gcn_deg_from == 'col'
        self._rev_c = None
        if self.enable_backward:
            if plan.reverse_of is None:
                raise ValueError('training needs a GraphPlan built with with_reverse=True')
            self._rev_c = (C.c_int * len(plan.reverse_of))(*plan.reverse_of)
        desc = _lib.ModelDesc(KINDS[kind], self.P, self._steps_c, self._rel_c, int(emb_dim), int(hidden_size),
                              int(repr_dim), int(heads), _lib.FUSE_ATT if channel_aggr == 'att' else _lib.FUSE_MEAN,
                              1 if gcn_deg_from == 'col' else 0, float(negative_slope), 1 if self.enable_backward else 0,
                              self._rev_c)
        handle = C.c_void_p()
        _lib.check(lib.pea_model_create(plan._h, C.byref(desc), C.byref(handle)))
        self._h = handle
        self.workspace_bytes = int(lib.pea_model_workspace_bytes(handle))
        self._ws = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=plan.device)
        self.n_layers = sum(self.steps)
        self.slots = len(PARAM_SLOTS[kind])
        msgs, ab = C.c_int64(), C.c_double()
        _lib.check(lib.pea_model_stats(handle, C.byref(msgs), C.byref(ab)))
        self.messages, self.algorithmic_bytes = int(msgs.value), float(ab.value)
        self.compulsory_bytes = float(lib.pea_model_compulsory_bytes(handle))   # HBM floor of one forward (bench.py)
        self.sharded = plan.shard[1] > 1
        self.n_stages = int(lib.pea_model_num_stages(handle))
        # float32 view of the workspace from its 256-byte aligned base (the exchanges index into it)
        skew = (-self._ws.data_ptr()) % 256
        self._wsf = self._ws[skew:skew + (self.workspace_bytes - 256) // 4 * 4].view(torch.float32)
        self._exchanges = []            # per level >= 1: [(desc, source table view, exchange buffer view, layout)]
        if self.sharded:
            n, world = plan.num_nodes, plan.shard[1]
            for level in range(self.n_stages):
                row = []
                for k in range(int(lib.pea_model_num_exchanges(handle, level))):
                    d = _lib.ExchangeDesc()
                    _lib.check(lib.pea_model_exchange_desc(handle, level, k, C.byref(d)))
                    src = self._wsf[d.src_offset_bytes // 4:d.src_offset_bytes // 4 + n * d.src_ld].view(n, d.src_ld)
                    rows = world * d.slots_per_rank
                    dst = self._wsf[d.dst_offset_bytes // 4:d.dst_offset_bytes // 4 + rows * d.dst_ld].view(rows, d.dst_ld)
                    row.append((d, src, dst, plan.source_layouts[d.relation]))
                self._exchanges.append(row)
            # stages whose transform writes this rank's exchange rows itself (no pack launch before the all-gather)
            self._fills = [bool(lib.pea_model_stage_fills_exchange(handle, k)) for k in range(self.n_stages)]

    def forward(self, layer_params, x, att=None, masked=None, want_stack=False, train=False, gather=True, out=None,
                select_ids=None):
        """layer_params: list (channel-major, then step) of tuples of tensors in PARAM_SLOTS order
        (a missing bias may be None).  train=True keeps what backward() needs (single GPU).  gather=False (sharded
        plans only): skip the final all-gather; only the rows this rank owns are defined in the result.  select_ids
        (sharded, int64 [K]): also returns [K, repr_dim] rows = the fused rows of those nodes this rank owns, zeros for
        the others (one launch with the fusion; the caller all-reduces them: ShardLayout.reduce_rows)."""
        lib = _lib.load()
        n = self.plan.num_nodes
        ptrs, keep, att_t = self._launch_args(layer_params, x, att)
        if out is None:
            out = torch.empty((n, self.repr_dim), dtype=torch.float32, device=x.device)
        stack = torch.empty((n, self.P, self.repr_dim), dtype=torch.float32, device=x.device) if want_stack else None
        m = -1 if masked is None else int(masked)
        if not self.sharded:
            fn = lib.pea_model_forward_train if train else lib.pea_model_forward
            _lib.check(fn(self._h, ptrs, _lib.ptr(keep[0]), _lib.ptr(att_t), m, _lib.ptr(self._ws),
                          self.workspace_bytes, _lib.ptr(out), _lib.ptr(stack), _lib.current_stream()))
            return (out, stack) if want_stack else out
        # Sharded forward (train=True: the training schedule, stage by stage, same exchanges): stage k computes this rank's rows of level k (and the transform feeding level k+1); the
        # gather sources of level k+1 are then all-gathered from their owners; after the last stage the fused rows
        # (not the per-metapath stack) are all-gathered: the fusion is row-local under row ownership.
        shard = self.plan.layout
        picked = None
        if train:
            if select_ids is not None:
                raise ValueError('select_ids rides in the inference stages (the training step exchanges stack rows)')
            for k in range(self.n_stages):
                _lib.check(lib.pea_model_forward_stage_train(self._h, k, ptrs, _lib.ptr(keep[0]), _lib.ptr(att_t), m,
                                                             _lib.ptr(self._ws), self.workspace_bytes, _lib.ptr(out),
                                                             _lib.ptr(stack), _lib.current_stream()))
                if k + 1 < self.n_stages:
                    for d, src, dst, lay in self._exchanges[k + 1]:
                        shard.exchange_sources(dst, src, lay, d.src_col, d.width)
        else:
            # stage k in two parts: (1) everything the exchange after it needs -- the all-gathers of the next level's gather
            # sources then start (asynchronously under RCCL) -- (2) the rows only this rank reads, behind them; the stream
            # waits for the collectives just before the next stage.  The last stage's fusion launch also picks the batch's
            # rows for the loss all-reduce (select_ids).
            opts = _lib.StageOpts(_lib.PART_ALL, None, 1, 0, None, None)
            for k in range(self.n_stages):
                last = k + 1 == self.n_stages
                opts.part = _lib.PART_ALL if last else _lib.PART_SOURCES
                if last and select_ids is not None:
                    ids = select_ids if select_ids.dtype == torch.int64 else select_ids.to(torch.int64)
                    picked = torch.empty((ids.numel(), self.repr_dim), dtype=torch.float32, device=x.device)
                    keep.append(ids)
                    flag = shard._err_flag(x.device)
                    opts.sel_ids, opts.sel_stride, opts.n_sel = ids.data_ptr(), ids.stride(0) if ids.dim() == 1 else 1, ids.numel()
                    opts.sel_out, opts.err_flag = picked.data_ptr(), flag.data_ptr()
                _lib.check(lib.pea_model_forward_part(self._h, k, C.byref(opts), ptrs, _lib.ptr(keep[0]), _lib.ptr(att_t), m,
                                                      _lib.ptr(self._ws), self.workspace_bytes, _lib.ptr(out),
                                                      _lib.ptr(stack), _lib.current_stream()))
                if last:
                    break
                filled = self._fills[k]
                pending = [shard.exchange_sources(dst, src, lay, d.src_col, d.width, packed=filled, async_op=True)
                           for d, src, dst, lay in self._exchanges[k + 1]]
                opts.part = _lib.PART_REST
                _lib.check(lib.pea_model_forward_part(self._h, k, C.byref(opts), ptrs, _lib.ptr(keep[0]), _lib.ptr(att_t), m,
                                                      _lib.ptr(self._ws), self.workspace_bytes, _lib.ptr(out),
                                                      _lib.ptr(stack), _lib.current_stream()))
                shard.wait_all(pending)
        if gather:
            shard.allgather_rows(out)
            if want_stack:
                shard.allgather_rows(stack)
        if select_ids is not None:
            return out, picked
        return (out, stack) if want_stack else out

    def _launch_args(self, layer_params, x, att):
        """Checks x / the parameters / att and returns (parameter pointer table, tensors to keep alive with x first, att as
        [P, repr_dim] or None): what every pea_model_forward* call is handed."""
        n = self.plan.num_nodes
        if x.shape != (n, self.emb_dim) or x.dtype != torch.float32 or not x.is_cuda:
            raise ValueError('x must be a CUDA float32 [%d, %d] tensor' % (n, self.emb_dim))
        if len(layer_params) != self.n_layers:
            raise ValueError('expected %d conv layers, got %d' % (self.n_layers, len(layer_params)))
        keep = [x.contiguous()]
        # The pointer table is rebuilt only when a parameter's storage moved (optimizers update in place): the checks and
        # the ctypes stores below were 80 us of a 300 us step on the launch-bound presets.  A cached table is reused only if
        # every tensor was contiguous float32 when it was built, so the raw pointers are the tensors' own.
        sig = tuple(None if t is None else t.data_ptr() for lp in layer_params for t in lp)
        cached = getattr(self, '_ptr_cache', None)
        if cached is not None and cached[0] == sig:
            ptrs = cached[1]
        else:
            ptrs = (C.c_void_p * (self.n_layers * self.slots))()
            k, plain = 0, True
            for lp in layer_params:
                if len(lp) != self.slots:
                    raise ValueError('each %s layer needs %d parameter tensors' % (self.kind, self.slots))
                for t in lp:
                    if t is None:
                        ptrs[k] = None
                    else:
                        t = t.detach()
                        if t.dtype != torch.float32 or not t.is_cuda:
                            raise ValueError('parameters must be CUDA float32 tensors')
                        plain = plain and t.is_contiguous()
                        t = t.contiguous()
                        keep.append(t)
                        ptrs[k] = t.data_ptr()
                    k += 1
            self._ptr_cache = (sig, ptrs) if plain and len(sig) == self.n_layers * self.slots else None
        att_t = None
        if self.channel_aggr == 'att':
            if att is None:
                raise ValueError("att is required for channel_aggr='att'")
            att_t = att.detach().reshape(self.P, self.repr_dim).contiguous()
            keep.append(att_t)
        return ptrs, keep, att_t

    def forward_ablate(self, layer_params, x, att=None, want_att=False):
        """One forward, every ablation variant (include/peahip.h, pea_model_forward_ablate): returns tables
        [P + 1, N, repr_dim] -- tables[0] bitwise forward(masked=None), tables[1 + p] bitwise forward(masked=p) -- and, with
        want_att, the unmasked fusion weights [N, P] (1 / P under 'mean'), else None.  Single GPU."""
        if self.sharded:
            raise NotImplementedError('the ablation sweep is single-GPU (this engine is sharded)')
        lib = _lib.load()
        check_pending_errors()
        n = self.plan.num_nodes
        ptrs, keep, att_t = self._launch_args(layer_params, x, att)
        tables = torch.empty((self.P + 1, n, self.repr_dim), dtype=torch.float32, device=x.device)
        weights = torch.empty((n, self.P), dtype=torch.float32, device=x.device) if want_att else None
        _lib.check(lib.pea_model_forward_ablate(self._h, ptrs, _lib.ptr(keep[0]), _lib.ptr(att_t), _lib.ptr(self._ws),
                                                self.workspace_bytes, _lib.ptr(tables), _lib.ptr(weights),
                                                _lib.current_stream()))
        return tables, weights

    # ------------------------------------------------------------------ sharded loss step, launches replayed from hipGraphs
    def _param_table(self, layer_params):
        sig = tuple(None if t is None else t.data_ptr() for lp in layer_params for t in lp)
        cached = getattr(self, '_ptr_cache', None)
        if cached is None or cached[0] != sig:
            return None, sig
        return cached[1], sig

    def sharded_loss(self, layer_params, x, att, triples, fc1_w, fc1_b, fc2_w, fc2_b):
        """One rank's share of  loss = model.loss(batch)  without autograd (reference models/base.py:43-48 in training
        mode: full-graph forward, then the BPR term of the batch) on a sharded plan, with every launch sequence between two
        collectives recorded ONCE on a launch tape (csrc/tape.hip; or captured into a hipGraph, PEA_SHARD_REPLAY=graph) and
        replayed while the argument pointers stay the same (parameters and
        x are updated in place by an optimizer; the batch is copied into a static id buffer):

            graph[stage 0, rows other ranks read] -> all-gather(s) of the next level's sources, asynchronous
            graph[stage 0, remaining rows]        -> stream waits for the all-gathers
            graph[last stage + fusion + the batch's rows] -> all-reduce of [3B, repr_dim] -> graph[scorer + BPR sum]

        A rank of 8 on the 25m-shaped graph issues ~10 launches of 10-90 us each; enqueueing them one by one through
        ctypes took as long as running them.  Returns (loss, fused rows of this rank [N, repr_dim]); both are static
        buffers that the next call overwrites (the loss is cloned).  PEA_SHARD_REPLAY=eager or GRAPHS_ENABLED = False (bench.py's
        per-kernel event pass): the same sequence, eager."""
        lib = _lib.load()
        shard = self.plan.layout
        n, b = self.plan.num_nodes, triples.shape[0]
        dev = x.device
        st = getattr(self, '_sl', None)
        if st is None or st['b'] != b:
            st = self._sl = {
                'b': b, 'ids': torch.empty(3 * b, dtype=torch.int64, device=dev),
                'out': torch.empty((n, self.repr_dim), dtype=torch.float32, device=dev),
                'picked': torch.empty((3 * b, self.repr_dim), dtype=torch.float32, device=dev),
                'local': torch.arange(3 * b, dtype=torch.int64, device=dev).view(b, 3),
                'loss': torch.empty((), dtype=torch.float32, device=dev),
                'ws': torch.zeros(int(lib.pea_bpr_workspace_bytes(b)), dtype=torch.uint8, device=dev),
                'key': None, 'graphs': None}
            # (the scorer reads local positions 0 .. 3B-1 of `picked`; node ids are validated where they are used, in the
            # fusion launch's row selection: ShardLayout._err_flag, checked by check_pending_errors like a bad BPR triple)
        t3 = triples[:, :3]
        st['ids'].view(b, 3).copy_(t3)
        att_t = att.detach().reshape(self.P, self.repr_dim) if self.channel_aggr == 'att' else None
        if att_t is not None and not att_t.is_contiguous():
            att_t = att_t.contiguous()
        fc = [t.detach() for t in (fc1_w, fc1_b, fc2_w, fc2_b)]
        if any(not t.is_contiguous() for t in fc):
            fc = [t.contiguous() for t in fc]
        ptrs, sig = self._param_table(layer_params)
        if ptrs is None:         # first call / a parameter moved: the eager forward validates and rebuilds the pointer table
            self.forward(layer_params, x, att=att, gather=False, out=st['out'])
            ptrs, sig = self._param_table(layer_params)
            if ptrs is None:
                raise ValueError('sharded_loss needs contiguous float32 parameters')
            st['key'] = None
        xd = x.detach()
        flag = shard._err_flag(dev)
        stream = _lib.current_stream

        def part(k, which, select):
            opts = _lib.StageOpts(which, None, 1, 0, None, None)
            if select:
                opts.sel_ids, opts.sel_stride, opts.n_sel = st['ids'].data_ptr(), 1, 3 * b
                opts.sel_out, opts.err_flag = st['picked'].data_ptr(), flag.data_ptr()
            _lib.check(lib.pea_model_forward_part(self._h, k, C.byref(opts), ptrs, _lib.ptr(xd), _lib.ptr(att_t), -1,
                                                  _lib.ptr(self._ws), self.workspace_bytes, _lib.ptr(st['out']), None, stream()))

        def score():
            _lib.check(lib.pea_bpr_score(b, self.repr_dim, 3 * b, _lib.ptr(st['picked']), _lib.ptr(st['local']), 3,
                                         _lib.ptr(fc[0]), _lib.ptr(fc[1]), _lib.ptr(fc[2]), _lib.ptr(fc[3]), None, None,
                                         _lib.ptr(st['loss']), _lib.ptr(st['ws']), st['ws'].numel(), stream()))

        last = self.n_stages - 1
        steps = []                                   # (name, callable) of every launch sequence between two collectives
        for k in range(self.n_stages):
            if k < last:
                steps.append((('src', k), lambda k=k: part(k, _lib.PART_SOURCES, False)))
                steps.append((('rest', k), lambda k=k: part(k, _lib.PART_REST, False)))
            else:
                steps.append((('last', k), lambda k=k: part(k, _lib.PART_ALL, True)))
        steps.append((('score', 0), score))
        # replay mode: 'tape' (default: the library's launch tape, csrc/tape.hip), 'graph' (hipGraphs: slower on the GPU
        # side, kept for comparison), 'eager' (PEA_SHARD_REPLAY=eager, or while bench.py times every launch with events)
        mode = _shard_replay_mode() if GRAPHS_ENABLED else 'eager'
        key = (mode, sig, xd.data_ptr(), None if att_t is None else att_t.data_ptr(), tuple(t.data_ptr() for t in fc),
               self._ws.data_ptr())
        if mode != 'eager' and st['key'] != key:
            for _, fn in steps:                      # warm-up on the real stream: lazy plan state (GCN norms ...) is built here
                fn()
            torch.cuda.synchronize()
            recs = {}
            for name, fn in steps:
                if mode == 'graph':
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        fn()
                else:
                    g = _lib.Tape()
                    with g.record():
                        fn()
                recs[name] = g
            st['key'], st['graphs'] = key, recs
        run = (lambda name, fn: fn()) if mode == 'eager' else (lambda name, fn: st['graphs'][name].replay())
        it = iter(steps)
        for k in range(self.n_stages):
            if k < last:
                name, fn = next(it)
                run(name, fn)
                filled = self._fills[k]
                pending = [shard.exchange_sources(dst, src, lay, d.src_col, d.width, packed=filled, async_op=True)
                           for d, src, dst, lay in self._exchanges[k + 1]]
                name, fn = next(it)
                run(name, fn)
                shard.wait_all(pending)
            else:
                name, fn = next(it)
                run(name, fn)
        shard.reduce_rows_(st['picked'])
        name, fn = next(it)
        run(name, fn)
        return st['loss'].clone(), st['out']

    def forward_graphed(self, layer_params, x, att=None, masked=None):
        """forward() with the launches of the schedule captured ONCE into a hipGraph and replayed while the argument
        pointers stay the same (parameters are updated in place by the optimizer, so a training loop keeps replaying):
        for launch-bound sizes (MovieLens latest-small: ~13 launches of 10-40 us each).  Unsharded, no stack.  The
        returned tensor is a static buffer that the next call overwrites."""
        if self.sharded:
            raise NotImplementedError('the graphed forward is single-GPU')
        key = (x.data_ptr(), None if att is None else att.data_ptr(), masked,
               tuple(None if t is None else t.data_ptr() for lp in layer_params for t in lp))
        if getattr(self, '_graph_key', None) != key:
            self._graph_out = self.forward(layer_params, x, att=att, masked=masked).clone()   # warm-up: attributes, lazy state
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.forward(layer_params, x, att=att, masked=masked, out=self._graph_out)
            self._graph, self._graph_key = graph, key
        self._graph.replay()
        return self._graph_out

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.load().pea_model_destroy(h)
            except Exception:
                pass
