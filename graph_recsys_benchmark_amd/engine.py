"""Host side of the HIP path: graph plan + whole-model schedule behind the reference's module surface.

    GraphPlan  <-  the P x S list of int64 COO tensors built by update_pea_graph_input
                   (reference graph_recsys_benchmark/utils/general_utils.py:280-395)
    PEAEngine  <-  PEABaseRecsysModel.forward (reference models/base.py:191-206) for one conv kind

PyTorch is used for device memory and streams only; all arithmetic runs in libpeahip.so.
"""
import ctypes as C

import torch

from . import _lib
from .sharding import ShardLayout

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


def _rows2d(t):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
        raise ValueError('expected a CUDA float32 [rows, cols] view with unit column stride')
    return t


_gw_ws = {}


class RowSet:
    """Rows of a table that hold a non-zero, on the device: flags uint8 [N], ids int32 [N] (the first `count` valid, ascending),
    count int32 [1] -- the host never reads the count (csrc/rows.hip).  Buffers are allocated once and refilled."""

    def __init__(self, n, device):
        lib = _lib.require_device()
        self.n = int(n)
        self.flags = torch.zeros(self.n, dtype=torch.uint8, device=device)
        self.ids = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self._ws = torch.empty(int(lib.pea_rows_nonzero_workspace_bytes(self.n)), dtype=torch.uint8, device=device)

    def zero_rows_of(self, table, width):
        """table[ids[q], 0:width] = 0 for the listed rows."""
        table = _rows2d(table)
        _lib.check(_lib.load().pea_rows_zero(_lib.ptr(table), table.stride(0), int(width), _lib.ptr(self.ids), _lib.ptr(self.count),
                                             _lib.current_stream()))

    def fill_from(self, table, width, also=None):
        """flags / ids / count of the rows of table [N, ld] whose first `width` columns hold a non-zero -- or that are flagged
        in `also` (uint8 [N])."""
        table = _rows2d(table)
        _lib.check(_lib.load().pea_rows_nonzero_or(self.n, int(width), _lib.ptr(table), table.stride(0), _lib.ptr(also),
                                                   _lib.ptr(self.flags), _lib.ptr(self.ids), _lib.ptr(self.count),
                                                   _lib.ptr(self._ws), self._ws.numel(), _lib.current_stream()))
        return self


def grad_weight(pairs, shard=None, rows=None):
    """[a_q^T b_q for (a_q, b_q) in pairs]: a_q [N, ma], b_q [N, nb] float32 views (row strides free) over the same N
    rows -- the weight gradients of one level in one pair of launches (pea_grad_weight: fixed-order reduction).  A pair may
    carry (mask uint8 [N], alt [N, nb]): rows flagged in mask take their b operand from alt (include/peahip.h, pea_gw_job).
    shard = (rank, world, tile): this rank's SHARE (the sum over the rows it owns); the caller all-reduces."""
    lib = _lib.require_device()
    if not pairs:
        return []
    n = pairs[0][0].shape[0]
    dev = pairs[0][0].device
    jobs = (_lib.GwJob * len(pairs))()
    outs = []
    for q, item in enumerate(pairs):
        a, b = _rows2d(item[0]), _rows2d(item[1])
        mask, alt = (item[2], _rows2d(item[3])) if len(item) > 2 else (None, None)     # rows flagged in mask read alt instead of b
        alt_scale = item[4] if len(item) > 4 else None                                  # ... times alt_scale[row] (float32 [N])
        if a.shape[0] != n or b.shape[0] != n:
            raise ValueError('grad_weight: operands of one call must share the row count')
        out = torch.empty((a.shape[1], b.shape[1]), dtype=torch.float32, device=dev)
        outs.append(out)
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n or alt.shape != b.shape):
            raise ValueError('grad_weight: the row mask must be uint8 [N] and the alternative operand shaped like b')
        jobs[q] = _lib.GwJob(a.data_ptr(), a.stride(0), a.shape[1], b.data_ptr(), b.stride(0), b.shape[1],
                             out.data_ptr(), out.stride(0), None if mask is None else mask.data_ptr(),
                             None if alt is None else alt.data_ptr(), 0 if alt is None else alt.stride(0),
                             None if alt_scale is None else alt_scale.data_ptr())
    ws = _gw_ws.get(dev)
    if ws is None:
        ws = _gw_ws[dev] = torch.empty(int(lib.pea_grad_weight_workspace_bytes()), dtype=torch.uint8, device=dev)
    if rows is not None:        # RowSet: the reduction runs over the listed rows only (the others contribute exact zeros)
        _lib.check(lib.pea_grad_weight_rows(n, _lib.ptr(rows.ids), _lib.ptr(rows.count), rows.n, len(pairs), jobs, _lib.ptr(ws),
                                            ws.numel(), _lib.current_stream()))
    elif shard is not None and shard[1] > 1:
        _lib.check(lib.pea_grad_weight_sharded(n, int(shard[2]), int(shard[1]), int(shard[0]), len(pairs), jobs, _lib.ptr(ws),
                                               ws.numel(), _lib.current_stream()))
    else:
        _lib.check(lib.pea_grad_weight(n, len(pairs), jobs, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    return outs


def dense_batch(triples_, rows=None, route=None):
    """out_q = a_q @ w_q for (a_q [N, k], w_q [k, n_out], out_q [N, n_out] view) in triples_: one launch (the input
    gradients dIn = dT W of one level); k, n_out and a's row stride must be multiples of 4 (a w whose row stride is not,
    or that does not start on a 16-byte boundary, is copied first).  rows (int32 device tensor): only those rows are
    computed (the rows a rank owns in a sharded training step).  A fourth element gate_q [N, n_out] (k <= 128) zeroes the
    outputs where gate_q <= 0: the relu mask of the layer below, applied in the epilogue.  route: diagnostic only -- a list
    that receives the library's account of the launches this call makes (_lib.dense_route of the very job structs); the
    tests of the dispatch use it, nothing in the product does."""
    lib = _lib.require_device()
    if not triples_:
        return
    n = triples_[0][0].shape[0]
    jobs = (_lib.DenseJob * len(triples_))()
    keep = []
    for q, item in enumerate(triples_):
        a, w, out = item[:3]
        gate = item[3] if len(item) > 3 else None
        a, out = _rows2d(a), _rows2d(out)
        # the library reads w with 16-byte loads: unit column stride, row stride a multiple of 4 floats, 16-byte aligned
        ok = w.stride(1) == 1 and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0
        w = _rows2d(w if ok else w.clone(memory_format=torch.contiguous_format))
        keep.append(w)
        if a.shape != (n, w.shape[0]) or out.shape != (n, w.shape[1]):
            raise ValueError('dense_batch: shapes %s @ %s -> %s' % (tuple(a.shape), tuple(w.shape), tuple(out.shape)))
        g_ptr, g_ld = None, 0
        if gate is not None:
            gate = _rows2d(gate)
            if gate.shape != out.shape:
                raise ValueError('dense_batch: gate %s for output %s' % (tuple(gate.shape), tuple(out.shape)))
            g_ptr, g_ld = gate.data_ptr(), gate.stride(0)
        jobs[q] = _lib.DenseJob(a.data_ptr(), a.stride(0), w.shape[0], w.data_ptr(), w.stride(0), w.shape[1],
                                out.data_ptr(), out.stride(0), g_ptr, g_ld)
    if route is not None:
        route += _lib.dense_route(n if rows is None else rows.numel(), rows is not None, jobs)
    if rows is not None:
        _lib.check(lib.pea_dense_batch_rows(rows.numel(), _lib.ptr(rows), len(triples_), jobs, _lib.current_stream()))
    else:
        _lib.check(lib.pea_dense_batch(n, len(triples_), jobs, _lib.current_stream()))


_m2b_ws = {}


def mlp2_backward_data(chans, emb, hid, out, dt1, h, dz, da, rows=None, weights_in_out=False):
    """Both products of the first layer's backward data path in one launch (csrc/mlp2_bwd.hip): for every channel
    (w0 [hid, emb], w1 [out, hid], dt1_col, h_col, dz_col, da_col) of `chans`:  dz = (dt1 . w1) where h > 0 else 0;
    da = dz . w0.  dt1, h, dz, da: float32 [N, ld] views of the training workspace.  rows (RowSet): the listed rows only."""
    lib = _lib.require_device()
    n = dt1.shape[0]
    arr = (_lib.Mlp2BwdChan * len(chans))()
    keep = []
    for q, (w0, w1, c1, ch, cz, ca) in enumerate(chans):
        w0, w1 = w0.detach(), w1.detach()
        if not w0.is_contiguous():
            w0 = w0.contiguous()
        if not w1.is_contiguous():
            w1 = w1.contiguous()
        keep += [w0, w1]
        arr[q] = _lib.Mlp2BwdChan(w0.data_ptr(), w1.data_ptr(), int(c1), int(ch), int(cz), int(ca))
    need = int(lib.pea_mlp2_backward_data_workspace_bytes(len(chans), int(emb), int(hid), int(out)))
    if need == 0:
        raise ValueError('mlp2_backward_data: unsupported widths (%d, %d, %d)' % (emb, hid, out))
    key = (dt1.device, need)
    ws = _m2b_ws.get(key)
    if ws is None:
        ws = _m2b_ws[key] = torch.empty(need, dtype=torch.uint8, device=dt1.device)
    _lib.check(lib.pea_mlp2_backward_data(n, len(chans), arr, int(emb), int(hid), int(out), _lib.ptr(dt1), dt1.stride(0),
                                          _lib.ptr(h), h.stride(0), _lib.ptr(dz), dz.stride(0), _lib.ptr(da), da.stride(0),
                                          None if rows is None else _lib.ptr(rows.ids), None if rows is None else _lib.ptr(rows.count),
                                          1 if weights_in_out else 0, _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def mlp2_backward_data_sage(chans, emb, hid, out, dt1, dr1, h, dz, dm, dxr, rows=None):
    """SAGE form of mlp2_backward_data (pea_mlp2_backward_data_sage): per channel (w_rel0 [hid, emb], w_root0, w_rel1 [out, hid],
    w_root1, dt1_col, dr1_col, h_col, dz_col, dm_col, dxr_col):  dz = (dt1 . w_rel1 + dr1 . w_root1) where h > 0 else 0;
    dm = dz . w_rel0;  dxr = dz . w_root0."""
    lib = _lib.require_device()
    n = dt1.shape[0]
    arr = (_lib.Mlp2BwdChan * len(chans))()
    arr_s = (_lib.Mlp2BwdChanSage * len(chans))()
    keep = []
    for q, (w0, w0r, w1, w1r, c1, cr, ch, cz, cm, cx) in enumerate(chans):
        ws_ = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in (w0, w0r, w1, w1r)]
        keep += ws_
        arr[q] = _lib.Mlp2BwdChan(ws_[0].data_ptr(), ws_[2].data_ptr(), int(c1), int(ch), int(cz), int(cm))
        arr_s[q] = _lib.Mlp2BwdChanSage(ws_[1].data_ptr(), ws_[3].data_ptr(), int(cr), int(cx))
    need = int(lib.pea_mlp2_backward_data_workspace_bytes(len(chans), int(emb), int(hid), int(out)))
    if need == 0:
        raise ValueError('mlp2_backward_data_sage: unsupported widths (%d, %d, %d)' % (emb, hid, out))
    key = (dt1.device, need)
    ws = _m2b_ws.get(key)
    if ws is None:
        ws = _m2b_ws[key] = torch.empty(need, dtype=torch.uint8, device=dt1.device)
    _lib.check(lib.pea_mlp2_backward_data_sage(n, len(chans), arr, arr_s, int(emb), int(hid), int(out), _lib.ptr(dt1), dt1.stride(0),
                                               _lib.ptr(dr1), dr1.stride(0), _lib.ptr(h), h.stride(0), _lib.ptr(dz), dz.stride(0),
                                               _lib.ptr(dm), dm.stride(0), _lib.ptr(dxr), dxr.stride(0),
                                               None if rows is None else _lib.ptr(rows.ids),
                                               None if rows is None else _lib.ptr(rows.count), _lib.ptr(ws), ws.numel(),
                                               _lib.current_stream()))


def block_sum(src, n_blocks, width):
    """[N, width] = sum of the n_blocks side-by-side column blocks of src [N, >= n_blocks * width] (fixed order)."""
    lib = _lib.require_device()
    src = _rows2d(src)
    out = torch.empty((src.shape[0], width), dtype=torch.float32, device=src.device)
    _lib.check(lib.pea_block_sum(src.shape[0], int(n_blocks), int(width), _lib.ptr(src), src.stride(0), _lib.ptr(out), out.stride(0),
                                 _lib.current_stream()))
    return out


_pending_err = []      # error flags of bpr_score calls that have not been read back yet (one int32 view each)
_pending_what = {}     # id(flag) -> the IndexError message of a queued flag that is not a BPR batch's


def check_pending_errors():
    """Raise IndexError if a bpr_score call since the last check saw a node id outside [0, num_nodes) -- what the
    reference raises at `cached_repr[unids]` (models/base.py:209-210).  The flag lives on the device, so reading it is
    a stream synchronize: it is read where the host synchronizes anyway (predict, rank_eval, model.eval(),
    bpr_score(validate=True)); until then the loss of such a batch is NaN, never a silently smaller sum."""
    global _pending_err, _pending_what
    flags, _pending_err = _pending_err, []
    what, _pending_what = _pending_what, {}
    if flags and int(torch.stack([f.reshape(-1)[0] for f in flags]).max().item()) != 0:
        message = 'index out of range in BPR triples'
        if what:       # the first raised flag names the call it came from
            raised = torch.stack([f.reshape(-1)[0] for f in flags]).cpu().tolist()
            message = next((what.get(id(f), message) for f, v in zip(flags, raised) if v), message)
        for f in flags:
            if f.numel() == 1 and f.dim() == 1:
                f.zero_()          # a persistent flag (sharding.ShardLayout) is re-armed
        raise IndexError(message)


def _defer_error(flag, what=None):
    """Queue the int32 error flag of a launch for the next check_pending_errors(); `what`: its IndexError message, if not the BPR
    one.  The list keeps the flag's storage alive until it is read, so a flag queued here has (or is a few bytes of) a small
    allocation of its own, never a view into a large workspace."""
    if len(_pending_err) >= 64:          # bounded: a long async loop never grows the list
        check_pending_errors()
    _pending_err.append(flag)
    if what:
        _pending_what[id(flag)] = what


def _int64_batch(batch, min_cols):
    """batch as the loss kernels read it: int64 [B, >= min_cols] with unit column stride (else copied)."""
    if batch.dtype != torch.int64 or batch.dim() != 2 or batch.shape[1] < min_cols:
        raise ValueError('batch must be int64 [B, >=%d]' % min_cols)
    return batch if batch.stride(1) == 1 else batch.contiguous()


def bpr_score(repr_, triples, fc1_w, fc1_b, fc2_w, fc2_b, want_preds=False, validate=False):
    """loss = -sum(log(sigmoid(pos - neg))) over rows (u, i+, i-) of `triples` (reference models/base.py:46-48,
    208-214).  Returns a 0-dim tensor (and pos, neg [B] when asked).  A triple with a node id out of range makes the
    loss NaN on the device and IndexError at the next check_pending_errors() (validate=True: at once)."""
    lib = _lib.require_device()
    if triples.dtype != torch.int64 or triples.dim() != 2 or triples.shape[1] < 3:
        raise ValueError('triples must be int64 [B, >=3]')
    if triples.stride(1) != 1:
        triples = triples.contiguous()
    b = triples.shape[0]
    r = repr_.shape[1]
    dev = repr_.device
    ws_bytes = int(lib.pea_bpr_workspace_bytes(b))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pos = torch.empty(b, dtype=torch.float32, device=dev) if want_preds else None
    neg = torch.empty(b, dtype=torch.float32, device=dev) if want_preds else None
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    _lib.check(lib.pea_bpr_score(b, r, repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(triples), triples.stride(0),
                                 _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(args[4]),
                                 _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(loss), _lib.ptr(ws), ws_bytes,
                                 _lib.current_stream()))
    _defer_error(ws[:4].view(torch.int32)[0])
    if validate:
        check_pending_errors()
    return (loss, pos, neg) if want_preds else loss


class _EntityReg(torch.autograd.Function):
    """reg(x) with the gradient rows of the same launch (csrc/entity.hip); backward = one index_add into dx."""

    @staticmethod
    def forward(ctx, x, batch9):
        reg, rows = _entity_launch(x, batch9, want_grad=True)
        ctx.save_for_backward(rows, batch9)
        ctx.shape = x.shape
        return reg

    @staticmethod
    def backward(ctx, g):
        rows, t = ctx.saved_tensors
        ids = t[:, [1, 3, 4, 0, 6, 7]].reshape(-1)            # order of the six gradient rows per batch row
        dx = torch.zeros(ctx.shape, dtype=rows.dtype, device=rows.device)
        dx.index_add_(0, ids, rows * g)
        return dx, None


def _entity_launch(x, batch9, want_grad):
    lib = _lib.require_device()
    if batch9.dtype != torch.int64 or batch9.dim() != 2 or batch9.shape[1] < 9:
        raise ValueError('entity-aware batches are int64 [B, 9] (u, i+, i-, 6 entity columns)')
    if batch9.stride(1) != 1:
        batch9 = batch9.contiguous()
    xd = x.detach()
    if xd.stride(1) != 1 or xd.stride(0) % 4:
        xd = xd.contiguous()
    b, f = batch9.shape[0], xd.shape[1]
    ws_bytes = int(lib.pea_entity_reg_workspace_bytes(b, f))
    if ws_bytes == 0:
        raise ValueError('entity_reg: emb_dim %d must be a multiple of 4, <= 256' % f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xd.device)
    reg = torch.empty((), dtype=torch.float32, device=xd.device)
    rows = torch.empty((6 * b, f), dtype=torch.float32, device=xd.device) if want_grad else None
    _lib.check(lib.pea_entity_reg(b, f, xd.shape[0], _lib.ptr(xd), xd.stride(0), _lib.ptr(batch9), batch9.stride(0),
                                  _lib.ptr(reg), _lib.ptr(rows), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    _defer_error(ws[:4].view(torch.int32)[0])
    return reg, rows


def entity_reg(x, batch9):
    """Entity-aware regulariser (reference models/base.py:50-73) in one HIP launch; differentiable with respect to x
    when x requires grad (gradient rows come out of the same launch)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _EntityReg.apply(x, batch9)
    return _entity_launch(x, batch9, want_grad=False)[0]


def _check_scored(rc):
    """The return code of a scoring entry point: a node id outside [0, num_nodes) is the reference's IndexError."""
    if rc == -2:
        raise IndexError(_lib.last_error())
    _lib.check(rc)


def _rank_io(unids, cand, dev, variants=()):
    """unids / cand as contiguous int64 and the outputs of an evaluator of cand's [U, C] (its last two dimensions) over
    `variants` tables: (scores [*variants, U, C], rank int32 / auc / loss [*variants, U]).  For the three candidate
    evaluators (rank_eval, rank_eval_multi, dot_rank_eval); the catalogue and pair wrappers have other outputs."""
    unids = unids.to(torch.int64).contiguous()
    cand = cand.to(torch.int64).contiguous()
    u, c = cand.shape[-2:]
    lead = tuple(variants) + (u,)
    outs = (torch.empty(lead + (c,), dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.int32, device=dev),
            torch.empty(lead, dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.float32, device=dev))
    return unids, cand, outs


def predict(repr_, unids, inids, fc1_w, fc1_b, fc2_w, fc2_b):
    """fc2(relu(fc1([repr[u] || repr[i]]))) -> [B, 1]  (reference models/base.py:208-214)."""
    lib = _lib.require_device()
    check_pending_errors()
    unids = unids.to(torch.int64).contiguous()
    inids = inids.to(torch.int64).contiguous()
    if unids.shape != inids.shape or unids.dim() != 1:
        raise ValueError('unids / inids must be 1-d of equal length')
    b = unids.shape[0]
    out = torch.empty(b, dtype=torch.float32, device=repr_.device)
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    rc = lib.pea_predict(b, repr_.shape[1], repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(unids), _lib.ptr(inids),
                         _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(args[4]), _lib.ptr(out),
                         _lib.current_stream())
    _check_scored(rc)
    return out.view(-1, 1)


def rank_eval(repr_, unids, cand, fc1_w, fc1_b, fc2_w, fc2_b):
    """Batched evaluator (reference solvers.py:56-96): cand [U, C], column 0 = the held-out positive.
    Returns scores [U, C], rank of the positive [U] (int32), auc [U], eval loss [U]."""
    lib = _lib.require_device()
    check_pending_errors()
    unids, cand, (scores, rank, auc, loss) = _rank_io(unids, cand, repr_.device)
    u, c = cand.shape
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    rc = lib.pea_rank_eval(u, c, repr_.shape[1], repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(unids), _lib.ptr(cand),
                           _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(args[4]),
                           _lib.ptr(scores), _lib.ptr(rank), _lib.ptr(auc), _lib.ptr(loss), _lib.current_stream())
    _check_scored(rc)
    return scores, rank, auc, loss


def fuse_ablate(stack, att, mode='att', want_att=True):
    """Every ablation variant of a channel stack [N, P, R] in one pass (include/peahip.h, pea_fuse_ablate): returns tables
    [P + 1, N, R] -- tables[0] the unmasked fusion (reference models/base.py:196-203), tables[1 + p] with channel p zeroed
    first (:194-195) -- and the unmasked fusion weights [N, P] (None unless want_att).  att: [P, R] (or [1, P, R]) for
    mode 'att', ignored for 'mean'."""
    lib = _lib.require_device()
    check_pending_errors()
    if mode not in ('att', 'mean'):
        raise NotImplementedError('Other aggr methods not implemeted!')
    if stack.dim() != 3 or stack.dtype != torch.float32 or not stack.is_cuda:
        raise ValueError('stack must be a CUDA float32 [N, P, R] tensor')
    stack = stack.detach().contiguous()
    n, p, r = stack.shape
    att_t = None
    if mode == 'att':
        if att is None:
            raise ValueError("att is required for mode 'att'")
        att_t = att.detach().reshape(p, r).contiguous()
    cols = (C.c_int * p)(*[q * r for q in range(p)])
    tables = torch.empty((p + 1, n, r), dtype=torch.float32, device=stack.device)
    weights = torch.empty((n, p), dtype=torch.float32, device=stack.device) if want_att else None
    _lib.check(lib.pea_fuse_ablate(n, p, r, _lib.ptr(stack), p * r, cols, _lib.ptr(att_t),
                                   _lib.FUSE_ATT if mode == 'att' else _lib.FUSE_MEAN, _lib.ptr(tables), _lib.ptr(weights),
                                   _lib.current_stream()))
    return tables, weights


def rank_eval_multi(tables, unids, cand, fc1_w, fc1_b, fc2_w, fc2_b):
    """rank_eval over V tables [V, N, R] in one launch (include/peahip.h, pea_rank_eval_multi).  cand [U, C]: every variant
    ranks the same candidates; cand [V, U, C]: variant v ranks cand[v].  Returns scores [V, U, C], rank [V, U] (int32),
    auc [V, U], eval loss [V, U]; row v is bitwise rank_eval(tables[v], unids, cand or cand[v], ...)."""
    lib = _lib.require_device()
    check_pending_errors()
    if tables.dim() != 3 or tables.dtype != torch.float32:
        raise ValueError('tables must be float32 [V, N, R]')
    tables = tables.detach().contiguous()
    v, n, r = tables.shape
    u = unids.shape[0]
    if cand.dim() == 2 and cand.shape[0] == u:
        c, stride = cand.shape[1], 0
    elif cand.dim() == 3 and cand.shape[0] == v and cand.shape[1] == u:
        c, stride = cand.shape[2], u * cand.shape[2]
    else:
        raise ValueError('cand must be [U, C] (shared by all variants) or [V, U, C]')
    unids, cand, (scores, rank, auc, loss) = _rank_io(unids, cand, tables.device, variants=(v,))
    args = [t.detach().contiguous() for t in (fc1_w, fc1_b, fc2_w, fc2_b)]
    rc = lib.pea_rank_eval_multi(v, u, c, r, n, _lib.ptr(tables), _lib.ptr(unids), _lib.ptr(cand), stride, _lib.ptr(args[0]),
                                 _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(scores), _lib.ptr(rank),
                                 _lib.ptr(auc), _lib.ptr(loss), _lib.current_stream())
    _check_scored(rc)
    return scores, rank, auc, loss


def _catalogue_args(repr_, unids, item_range, exclude):
    unids = unids.to(torch.int64).contiguous()
    if unids.dim() != 1:
        raise ValueError('unids must be 1-d')
    item_lo, item_hi = int(item_range[0]), int(item_range[1])
    if item_hi < item_lo:
        raise ValueError('item_range is (first item node id, one past the last)')
    rowptr = items = None
    if exclude is not None:
        rowptr, items = exclude
        if rowptr.dtype != torch.int64 or items.dtype != torch.int64 or rowptr.numel() != unids.numel() + 1:
            raise ValueError('exclude is (rowptr int64 [U + 1], items int64) -- see utils.interactions.seen_items_csr')
        if rowptr.device != repr_.device or items.device != repr_.device:
            raise ValueError('the exclusion lists must live on the device of the table')
        rowptr, items = rowptr.contiguous(), items.contiguous()
        if items.numel() == 0:                  # a valid pointer for the C side even when nobody has seen anything
            items = torch.zeros(1, dtype=torch.int64, device=repr_.device)
    return unids, item_lo, item_hi - item_lo, rowptr, items


def recommend_topk(repr_, unids, k, item_range, fc1_w, fc1_b, fc2_w, fc2_b, exclude=None):
    """The k best items of the catalogue item_range = (lo, hi) (node ids [lo, hi)) for every user of `unids`, scored
    like predict (reference models/base.py:208-214) and ordered by (score descending, node id ascending); `exclude`
    = (rowptr [U + 1], items) names per requested user the items to leave out (utils.interactions.seen_items_csr).
    Returns (items int64 [U, k], scores float32 [U, k]); a user with fewer than k eligible items gets (-1, -inf) in the
    tail.  One pass over the catalogue on the device (include/peahip.h, pea_recommend_topk); the [U, items] score matrix
    is never written."""
    lib = _lib.require_device()
    check_pending_errors()
    unids, item_lo, n_items, rowptr, items = _catalogue_args(repr_, unids, item_range, exclude)
    u, k, r = unids.shape[0], int(k), repr_.shape[1]
    dev = repr_.device
    out_items = torch.empty((u, max(k, 0)), dtype=torch.int64, device=dev)
    out_scores = torch.empty((u, max(k, 0)), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_topk_workspace_bytes(u, n_items, k, r))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    rc = lib.pea_recommend_topk(u, k, r, repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(unids), item_lo, n_items,
                                _lib.ptr(rowptr), _lib.ptr(items), _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]),
                                _lib.ptr(args[4]), _lib.ptr(out_items), _lib.ptr(out_scores), _lib.ptr(ws), ws_bytes,
                                _lib.current_stream())
    _check_scored(rc)
    return out_items, out_scores


def rank_full(repr_, unids, pos_items, item_range, fc1_w, fc1_b, fc2_w, fc2_b, exclude=None):
    """All-item evaluation (the protocol of reference solvers.py:56-96 with EVERY eligible item as a negative instead of
    99 sampled ones): per user the rank of the held-out positive = number of eligible other items scoring strictly
    higher, auc = share of them scoring strictly lower, and the positive's score.  Returns (rank int32 [U], auc [U],
    pos_score [U]).  include/peahip.h, pea_rank_full."""
    lib = _lib.require_device()
    check_pending_errors()
    unids, item_lo, n_items, rowptr, items = _catalogue_args(repr_, unids, item_range, exclude)
    pos_items = pos_items.to(torch.int64).contiguous()
    if pos_items.shape != unids.shape:
        raise ValueError('one positive per requested user')
    u, r = unids.shape[0], repr_.shape[1]
    dev = repr_.device
    rank = torch.empty(u, dtype=torch.int32, device=dev)
    auc = torch.empty(u, dtype=torch.float32, device=dev)
    pos_score = torch.empty(u, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_topk_workspace_bytes(u, n_items, 1, r))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    rc = lib.pea_rank_full(u, r, repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(unids), _lib.ptr(pos_items), item_lo, n_items,
                           _lib.ptr(rowptr), _lib.ptr(items), _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]),
                           _lib.ptr(args[4]), _lib.ptr(rank), _lib.ptr(auc), _lib.ptr(pos_score), _lib.ptr(ws), ws_bytes,
                           _lib.current_stream())
    _check_scored(rc)
    return rank, auc, pos_score


def _dot_table(repr_):
    """Validation shared by the inner-product entry points (include/peahip.h, pea_dot_*): a CUDA float32 [N, D] table, D a
    multiple of 4 and <= 256; returned detached and contiguous."""
    if not torch.is_tensor(repr_) or repr_.dim() != 2 or repr_.dtype != torch.float32:
        raise ValueError('the table must be a float32 [N, D] tensor')
    if not repr_.is_cuda:
        raise ValueError('the table must live on the GPU (there is no CPU fallback)')
    d = repr_.shape[1]
    if d < 4 or d % 4 != 0 or d > 256:
        raise ValueError('the table width %d must be a multiple of 4 in 4..256' % d)
    return repr_.detach().contiguous()


def dot_predict(repr_, unids, inids):
    """sum(repr[u] * repr[i]) -> [B]  (reference models/kgat.py, kgcn.py, ngcf.py: predict), as one fma chain over the
    columns in ascending order (include/peahip.h, pea_dot_predict)."""
    lib = _lib.require_device()
    check_pending_errors()
    table = _dot_table(repr_)
    unids = unids.to(torch.int64).contiguous()
    inids = inids.to(torch.int64).contiguous()
    if unids.shape != inids.shape or unids.dim() != 1:
        raise ValueError('unids / inids must be 1-d of equal length')
    b = unids.shape[0]
    out = torch.empty(b, dtype=torch.float32, device=table.device)
    rc = lib.pea_dot_predict(b, table.shape[1], table.shape[0], _lib.ptr(table), _lib.ptr(unids), _lib.ptr(inids),
                             _lib.ptr(out), _lib.current_stream())
    _check_scored(rc)
    return out


def dot_rank_eval(repr_, unids, cand):
    """rank_eval with the inner-product scorer: cand [U, C], column 0 = the held-out positive.  Returns scores [U, C], rank
    of the positive [U] (int32), auc [U], eval loss [U]."""
    lib = _lib.require_device()
    check_pending_errors()
    table = _dot_table(repr_)
    if cand.dim() != 2 or unids.dim() != 1 or cand.shape[0] != unids.shape[0]:
        raise ValueError('cand must be [U, C] with one row per user of unids')
    unids, cand, (scores, rank, auc, loss) = _rank_io(unids, cand, table.device)
    u, c = cand.shape
    rc = lib.pea_dot_rank_eval(u, c, table.shape[1], table.shape[0], _lib.ptr(table), _lib.ptr(unids), _lib.ptr(cand),
                               _lib.ptr(scores), _lib.ptr(rank), _lib.ptr(auc), _lib.ptr(loss), _lib.current_stream())
    _check_scored(rc)
    return scores, rank, auc, loss


def dot_recommend_topk(repr_, unids, k, item_range, exclude=None):
    """recommend_topk with the inner-product scorer: the k best items of the catalogue item_range = (lo, hi) for every user
    of `unids`, ordered by (score descending, node id ascending), `exclude` = (rowptr [U + 1], items) left out.  Returns
    (items int64 [U, k], scores float32 [U, k]) with a (-1, -inf) tail.  The catalogue scan is an MFMA GEMM whose score
    tiles are selected from in registers (include/peahip.h, pea_dot_recommend_topk); the [U, items] score matrix is never
    written."""
    lib = _lib.require_device()
    check_pending_errors()
    table = _dot_table(repr_)
    unids, item_lo, n_items, rowptr, items = _catalogue_args(table, unids, item_range, exclude)
    u, k, d = unids.shape[0], int(k), table.shape[1]
    dev = table.device
    out_items = torch.empty((u, max(k, 0)), dtype=torch.int64, device=dev)
    out_scores = torch.empty((u, max(k, 0)), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_dot_topk_workspace_bytes(u, n_items, k, d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    rc = lib.pea_dot_recommend_topk(u, k, d, table.shape[0], _lib.ptr(table), _lib.ptr(unids), item_lo, n_items,
                                    _lib.ptr(rowptr), _lib.ptr(items), _lib.ptr(out_items), _lib.ptr(out_scores),
                                    _lib.ptr(ws), ws_bytes, _lib.current_stream())
    _check_scored(rc)
    return out_items, out_scores


def dot_rank_full(repr_, unids, pos_items, item_range, exclude=None):
    """rank_full with the inner-product scorer: per user the number of eligible other items scoring strictly higher than
    the held-out positive, the share scoring strictly lower, and the positive's score.  Returns (rank int32 [U], auc [U],
    pos_score [U]).  include/peahip.h, pea_dot_rank_full."""
    lib = _lib.require_device()
    check_pending_errors()
    table = _dot_table(repr_)
    unids, item_lo, n_items, rowptr, items = _catalogue_args(table, unids, item_range, exclude)
    pos_items = pos_items.to(torch.int64).contiguous()
    if pos_items.shape != unids.shape:
        raise ValueError('one positive per requested user')
    u, d = unids.shape[0], table.shape[1]
    dev = table.device
    rank = torch.empty(u, dtype=torch.int32, device=dev)
    auc = torch.empty(u, dtype=torch.float32, device=dev)
    pos_score = torch.empty(u, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_dot_topk_workspace_bytes(u, n_items, 1, d))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    rc = lib.pea_dot_rank_full(u, d, table.shape[0], _lib.ptr(table), _lib.ptr(unids), _lib.ptr(pos_items), item_lo, n_items,
                               _lib.ptr(rowptr), _lib.ptr(items), _lib.ptr(rank), _lib.ptr(auc), _lib.ptr(pos_score),
                               _lib.ptr(ws), ws_bytes, _lib.current_stream())
    _check_scored(rc)
    return rank, auc, pos_score


def bpr_train_raw(picked, att, fc1_w, fc1_b, fc2_w, fc2_b):
    """One launch of csrc/bpr_train.hip + the two fixed-order reductions (pea_grad_weight): returns
    (loss, grad_rows [3B, P*R], (d_att | None, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b)) for picked [3B, P, R]."""
    lib = _lib.require_device()
    n3, p_, r_ = picked.shape
    b = n3 // 3
    rows = picked.detach()
    if not rows.is_contiguous():
        rows = rows.contiguous()
    dev = rows.device
    keep = [t.detach().contiguous() for t in (fc1_w, fc1_b, fc2_w, fc2_b)]
    att_c = att.detach().contiguous().view(-1) if att is not None else None
    grad_rows = torch.empty((n3, p_ * r_), dtype=torch.float32, device=dev)
    dhx = torch.empty((2 * b, r_ + 4), dtype=torch.float32, device=dev)
    zx = torch.empty((2 * b, 3 * r_ + 4), dtype=torch.float32, device=dev)
    p4 = (p_ + 3) // 4 * 4
    dsc = torch.empty((n3, p4), dtype=torch.float32, device=dev) if att is not None else None
    ws_bytes = int(lib.pea_bpr_train_workspace_bytes(b))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    _lib.check(lib.pea_bpr_train(b, p_, r_, _lib.ptr(rows), p_ * r_, _lib.ptr(att_c), _lib.ptr(keep[0]), _lib.ptr(keep[1]),
                                 _lib.ptr(keep[2]), _lib.ptr(keep[3]), _lib.ptr(loss), _lib.ptr(grad_rows), _lib.ptr(dhx),
                                 _lib.ptr(zx), _lib.ptr(dsc), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    g = grad_weight([(dhx, zx)])[0]                    # [R + 4, 3R + 4]
    d_att = None
    if att is not None:
        full = grad_weight([(dsc, rows.view(n3, p_ * r_))])[0]      # [P4, P * R]: the diagonal R-blocks are d att[p]
        d_att = torch.stack([full[q, q * r_:(q + 1) * r_] for q in range(p_)]).view(att.shape)
    return loss, grad_rows, (d_att, g[:r_, :2 * r_], g[:r_, 3 * r_], g[r_, 2 * r_:3 * r_].view(fc2_w.shape),
                             g[r_, 3 * r_].view(fc2_b.shape))


def rows_scatter_sum(ids, src, num_channels, repr_dim, col_of_channel, dst):
    """dst[id, col_of_channel[p] + c] = sum_{k: ids[k] == id} src[k, p * R + c] in increasing k (ids < 0 skipped): the
    deterministic index backward of rows = stack[ids] into the node-indexed gradient buffer (an LDS sort of the batch's
    ids + one wave per node); at most ROWS_SCATTER_MAX positions."""
    lib = _lib.require_device()
    cols = (C.c_int * num_channels)(*[int(c) for c in col_of_channel])
    ws_bytes = int(lib.pea_rows_scatter_sum_workspace_bytes(ids.numel()))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=src.device)
    _lib.check(lib.pea_rows_scatter_sum(ids.numel(), _lib.ptr(ids), _lib.ptr(src), src.stride(0), int(num_channels), int(repr_dim),
                                        cols, _lib.ptr(dst), dst.stride(0), dst.shape[0], _lib.ptr(ws), ws_bytes, _lib.current_stream()))


ROWS_SCATTER_MAX = 16384      # positions pea_rows_scatter_sum sorts in LDS (a BPR batch of up to 5461 triples)


def _scatter_dense(ids, rows, n, w):
    """The dense [n, w] gradient of a table from the gradient rows [len(ids), w] of the positions that read it."""
    dst = torch.zeros((n, w), dtype=torch.float32, device=rows.device)
    rows_scatter_sum(ids, rows, 1, w, [0], dst)
    return dst


class _BprTrainLoss(torch.autograd.Function):
    """loss = -sum_b log sigmoid(score(u_b, i+_b) - score(u_b, i-_b)) over the fused rows of the batch's stack rows, and its
    whole backward, in one HIP launch (csrc/bpr_train.hip) + two fixed-order reductions for the parameter gradients
    (pea_grad_weight).  Reference: models/base.py:193-203 (fusion), :208-214 (fc1 / fc2 scorer), :46-48 (BPR loss) under
    loss.backward() (solvers.py:213-214)."""

    @staticmethod
    def forward(ctx, picked, att, fc1_w, fc1_b, fc2_w, fc2_b):
        loss, grad_rows, head = bpr_train_raw(picked, att, fc1_w, fc1_b, fc2_w, fc2_b)
        ctx.grads = (grad_rows.view(picked.shape),) + head
        return loss

    @staticmethod
    def backward(ctx, g):
        return tuple(None if t is None else t * g for t in ctx.grads)


def bpr_train_supported(num_channels, repr_dim):
    return bool(_lib.require_device().pea_bpr_train_supported(int(num_channels), int(repr_dim)))


def bpr_train_loss(picked, att, fc1_w, fc1_b, fc2_w, fc2_b):
    """Differentiable BPR loss of a batch from its stack rows picked [3B, P, R] (rows 3b, 3b+1, 3b+2 = user, positive,
    negative of triple b): channel fusion ('att' with the [.., P, R] attention tensor, 'mean' with att=None), the fc1 / fc2
    scorer and the loss, forward and backward in HIP."""
    return _BprTrainLoss.apply(picked, att, fc1_w, fc1_b, fc2_w, fc2_b)


DOT_TRAIN_MAX_BLOCKS = 4      # column blocks pea_dot_bpr_train takes (include/peahip.h)


def dot_bpr_train_raw(blocks, batch):
    """One launch of csrc/dot_train.hip: (loss, grad_rows [3B, D], error flag) for the raw conv outputs `blocks` (a list of
    [N, w_k] tensors whose normalised concatenation is the models' table) and the int64 [B, >= 3] triples `batch`."""
    lib = _lib.require_device()
    batch = _int64_batch(batch, 3)
    if not 1 <= len(blocks) <= DOT_TRAIN_MAX_BLOCKS:
        raise ValueError('1..%d column blocks expected' % DOT_TRAIN_MAX_BLOCKS)
    rows = [_block16(t) for t in blocks]
    n, b, dev = rows[0].shape[0], batch.shape[0], rows[0].device
    if any(t.shape[0] != n for t in rows):
        raise ValueError('the blocks must have the same number of rows')
    k = len(rows)
    d = sum(t.shape[1] for t in rows)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in rows])
    lds = (C.c_int64 * k)(*[t.stride(0) for t in rows])
    widths = (C.c_int * k)(*[t.shape[1] for t in rows])
    grad_rows = torch.empty((3 * b, d), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_dot_bpr_train_workspace_bytes(b))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pea_dot_bpr_train(b, k, ptrs, lds, widths, n, _lib.ptr(batch), batch.stride(0), _lib.ptr(loss),
                                     _lib.ptr(grad_rows), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    return loss, grad_rows, ws[:4].view(torch.int32)[0]


class _DotBprLoss(torch.autograd.Function):
    """loss = -sum_b log sigmoid(pos_b - neg_b) under the inner-product scorer over cat_k normalize(block_k), with its whole
    backward from the same launch (csrc/dot_train.hip); backward scatters the batch's gradient rows into one dense gradient
    per block with pea_rows_scatter_sum (fixed order).  Reference: models/kgat.py:45-57 + experiments/kgat_solver_bpr.py:
    101-108 under loss.backward()."""

    @staticmethod
    def forward(ctx, batch, *blocks):
        loss, grad_rows, flag = dot_bpr_train_raw(blocks, batch)
        _defer_error(flag)
        ctx.ids = batch[:, :3].reshape(-1).contiguous()
        ctx.grad_rows = grad_rows
        ctx.shapes = [tuple(t.shape) for t in blocks]
        return loss

    @staticmethod
    def backward(ctx, g):
        rows = ctx.grad_rows * g
        grads, off = [], 0
        for i, (n, w) in enumerate(ctx.shapes):
            grads.append(_scatter_dense(ctx.ids, rows[:, off:off + w], n, w) if ctx.needs_input_grad[1 + i] else None)
            off += w
        return (None,) + tuple(grads)


def dot_bpr_supported(widths, batch_size):
    """Whether dot_bpr_loss takes these block widths and this batch (else the caller stays on autograd)."""
    return (1 <= len(widths) <= DOT_TRAIN_MAX_BLOCKS and all(w >= 4 and w % 4 == 0 for w in widths) and sum(widths) <= 256
            and 3 * int(batch_size) <= ROWS_SCATTER_MAX)


def dot_bpr_loss(blocks, batch):
    """Differentiable BPR loss of the int64 [B, >= 3] triples `batch` from the UN-normalised conv outputs `blocks` (a list of
    [N, w_k] float32 tensors; the table the reference scores is cat_k normalize(block_k), which is never formed here).
    backward() gives one dense [N, w_k] gradient per block.  3 B <= ROWS_SCATTER_MAX (dot_bpr_supported)."""
    blocks = list(blocks)
    if not dot_bpr_supported([int(t.shape[1]) for t in blocks], batch.shape[0]):
        raise ValueError('dot_bpr_loss: block widths (multiples of 4, sum <= 256, at most %d blocks) or batch size (3 B <= %d) '
                         'not supported' % (DOT_TRAIN_MAX_BLOCKS, ROWS_SCATTER_MAX))
    return _DotBprLoss.apply(batch, *blocks)


def transr_supported(emb, batch_size):
    """Whether transr_loss takes this width (a multiple of 4 in 4..128, csrc/transr_train.hip) and this batch (its 3 B node
    positions go back through rows_scatter_sum); needs no device.  Else the caller stays on autograd."""
    return bool(_lib.load().pea_transr_supported(int(emb))) and 3 * int(batch_size) <= ROWS_SCATTER_MAX


def _block16(t):
    """t as dot_bpr_train / transr_train read it: rows with a stride that is a multiple of 4 floats and a 16-byte aligned start (a column
    block of a wider buffer qualifies); anything else is copied."""
    t = _rows2d(t.detach())
    if t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def transr_train_raw(x, proj, r, batch, need_grad=True):
    """One launch of csrc/transr_train.hip (+ its fixed-order reduction): (loss, pos [B], neg [B], grad_rows [3B, E],
    grad_rel_rows [B, E], dproj [E, E], error flag) of the TransR-style kg_loss for x [N, E], proj [E, E], r [R, E] and the
    int64 [B, >= 4] rows (h, t+, t-, rel) of `batch`.  need_grad=False is the forward-only form: the three gradients are
    None and no backward work is done."""
    lib = _lib.require_device()
    batch = _int64_batch(batch, 4)
    x, r = _block16(x), _block16(r)
    proj = _rows2d(proj.detach()).contiguous()
    e = x.shape[1]
    if not lib.pea_transr_supported(e):
        raise ValueError('transr_train: width %d not supported (a multiple of 4 in 4..128)' % e)
    if tuple(proj.shape) != (e, e) or r.shape[1] != e or r.shape[0] < 1 or x.shape[0] < 1:
        raise ValueError('transr_train: x [N, E], proj [E, E] and r [R, E] expected')
    b, dev = batch.shape[0], x.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pos = torch.empty(b, dtype=torch.float32, device=dev)
    neg = torch.empty(b, dtype=torch.float32, device=dev)
    grad_rows = grad_rel = dproj = None
    if need_grad:
        grad_rows = torch.empty((3 * b, e), dtype=torch.float32, device=dev)
        grad_rel = torch.empty((b, e), dtype=torch.float32, device=dev)
        dproj = torch.empty((e, e), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_transr_train_workspace_bytes(b, e))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pea_transr_train(b, e, _lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(proj), _lib.ptr(r), r.stride(0),
                                    r.shape[0], _lib.ptr(batch), batch.stride(0), _lib.ptr(loss), _lib.ptr(pos), _lib.ptr(neg),
                                    _lib.ptr(grad_rows), _lib.ptr(grad_rel), _lib.ptr(dproj), _lib.ptr(ws), ws_bytes,
                                    _lib.current_stream()))
    return loss, pos, neg, grad_rows, grad_rel, dproj, ws[:4].view(torch.int32)[0]


class _TransrLoss(torch.autograd.Function):
    """loss = -sum_b log sigmoid(pos_b - neg_b) of the TransR-style KG phase with its whole backward from the same launch
    (csrc/transr_train.hip); backward scatters the batch's gradient rows into dense x and r gradients with
    pea_rows_scatter_sum (fixed order).  Reference: experiments/kgat_solver_bpr.py:110-124 under loss.backward()."""

    @staticmethod
    def forward(ctx, batch, need_grad, x, proj, r):
        loss, _, _, grad_rows, grad_rel, dproj, flag = transr_train_raw(x, proj, r, batch, need_grad)
        _defer_error(flag)
        if need_grad:
            ctx.node_ids = batch[:, :3].reshape(-1).contiguous()
            ctx.rel_ids = batch[:, 3].contiguous()
            ctx.grads = (grad_rows, grad_rel, dproj)
            ctx.shapes = (tuple(x.shape), tuple(r.shape))
        return loss

    @staticmethod
    def backward(ctx, g):
        grad_rows, grad_rel, dproj = ctx.grads
        (n, e), (n_rel, _) = ctx.shapes
        dx = dp = dr = None
        if ctx.needs_input_grad[2]:
            dx = _scatter_dense(ctx.node_ids, grad_rows * g, n, e)
        if ctx.needs_input_grad[3]:
            dp = dproj * g
        if ctx.needs_input_grad[4]:
            dr = _scatter_dense(ctx.rel_ids, grad_rel * g, n_rel, e)
        return None, None, dx, dp, dr


def transr_loss(x, proj_mat, r, batch):
    """Differentiable TransR-style kg_loss (models/kg_base.py) of the int64 [B, >= 4] rows (h, t+, t-, rel) of `batch`, forward
    and backward in HIP; backward() gives dense gradients for x [N, E], proj_mat [E, E] and r [R, E].  With grad disabled,
    or when no input requires grad, only the forward runs.  A row with an id out of range contributes nothing and raises
    IndexError at the next check_pending_errors().  transr_supported(E, B) must hold."""
    if x.dim() != 2 or not transr_supported(x.shape[1], batch.shape[0]):
        raise ValueError('transr_loss: width (a multiple of 4 in 4..128) or batch size (3 B <= %d) not supported' % ROWS_SCATTER_MAX)
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, proj_mat, r))
    return _TransrLoss.apply(batch, need_grad, x, proj_mat, r)


# ------------------------------------------------------------------------------------------------------------
# HeRec (csrc/herec.hip; reference models/herec.py, experiments/herec_solver_bpr.py:108-121)
# ------------------------------------------------------------------------------------------------------------
HEREC_MAX_TABLES = 4      # PEA_HEREC_MAX_TABLES (include/peahip.h)


def herec_supported(dim, num_tables, batch_size=0):
    """Whether herec_mse_loss / herec_table take this width and number of metapath tables (include/peahip.h,
    pea_herec_supported) and this batch (its B positions go back through rows_scatter_sum); needs no device."""
    return bool(_lib.load().pea_herec_supported(int(dim), int(num_tables))) and int(batch_size) <= ROWS_SCATTER_MAX


def _herec_args(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias):
    """The tensors as pea_herec_* read them: (tables, ctypes pointer and stride arrays, w [M, D, D], b [M, D], the four
    embedding tables), detached, float32, 16-byte aligned."""
    tables = [_block16(t) for t in tables]
    m = len(tables)
    if m < 1 or any(t.shape != tables[0].shape or t.dtype != torch.float32 for t in tables):
        raise ValueError('herec: a non-empty list of float32 [N, D] tables of one shape expected')
    d = tables[0].shape[1]
    if not _lib.load().pea_herec_supported(d, m):
        raise ValueError('herec: width %d with %d tables is not supported (engine.herec_supported)' % (d, m))
    w = emb_trans_w if torch.is_tensor(emb_trans_w) else torch.stack([t.detach() for t in emb_trans_w])
    b = emb_trans_b if torch.is_tensor(emb_trans_b) else torch.stack([t.detach() for t in emb_trans_b])
    w, b = w.detach().contiguous(), b.detach().contiguous()
    embs = [t.detach().contiguous() for t in (user_emb, item_emb, user_rk_bias, item_rk_bias)]
    if (tuple(w.shape) != (m, d, d) or tuple(b.shape) != (m, d) or any(t.dim() != 2 or t.shape[1] != d for t in embs)
            or embs[0].shape != embs[2].shape or embs[1].shape != embs[3].shape):
        raise ValueError('herec: w [M, D, D], b [M, D], user tables [num_uids, D] and item tables [num_iids, D] expected')
    ptrs = (C.c_void_p * m)(*[t.data_ptr() for t in tables])
    lds = (C.c_int64 * m)(*[t.stride(0) for t in tables])
    return tables, ptrs, lds, w, b, embs


def herec_train_raw(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias, acc_uids, acc_iids,
                    unids, inids, labels, need_grad=True):
    """One launch of csrc/herec.hip (+ its fixed-order reduction): (loss, pred [B], dW [M, D, D], db [M, D], g_user [B, 2D],
    g_item [B, 2D], error flag) for the M frozen tables, the emb_trans weights (a [M, D, D] tensor or a list of [D, D]) and
    biases, the four embedding tables and B labelled pairs.  need_grad=False: forward only, the four gradients are None."""
    lib = _lib.require_device()
    tables, ptrs, lds, w, b, embs = _herec_args(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias)
    m, (n, d), dev = len(tables), tables[0].shape, tables[0].device
    unids = unids.to(torch.int64).contiguous()
    inids = inids.to(torch.int64).contiguous()
    labels = labels.to(torch.float32).contiguous()
    if unids.dim() != 1 or unids.shape != inids.shape or unids.shape != labels.shape:
        raise ValueError('herec: unids, inids and labels must be 1-d of equal length')
    bsz = unids.shape[0]
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pred = torch.empty(bsz, dtype=torch.float32, device=dev)
    dw = db = g_user = g_item = None
    if need_grad:
        dw = torch.empty((m, d, d), dtype=torch.float32, device=dev)
        db = torch.empty((m, d), dtype=torch.float32, device=dev)
        g_user = torch.empty((bsz, 2 * d), dtype=torch.float32, device=dev)
        g_item = torch.empty((bsz, 2 * d), dtype=torch.float32, device=dev)
    ws_bytes = int(lib.pea_herec_train_workspace_bytes(bsz, d, m))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pea_herec_train(bsz, d, m, ptrs, lds, _lib.ptr(w), _lib.ptr(b), _lib.ptr(embs[0]), _lib.ptr(embs[1]),
                                   _lib.ptr(embs[2]), _lib.ptr(embs[3]), int(acc_uids), embs[0].shape[0], int(acc_iids),
                                   embs[1].shape[0], n, _lib.ptr(unids), _lib.ptr(inids), _lib.ptr(labels), _lib.ptr(loss),
                                   _lib.ptr(pred), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(g_user), _lib.ptr(g_item), _lib.ptr(ws),
                                   ws_bytes, _lib.current_stream()))
    return loss, pred, dw, db, g_user, g_item, ws[:4].view(torch.int32)[0].clone()


class _HerecLoss(torch.autograd.Function):
    """loss = mean_b (pred_b - label_b)^2 of the HeRec score with its whole backward from the same launch (csrc/herec.hip);
    backward scatters the pairs' gradient rows into dense gradients of the four embedding tables with pea_rows_scatter_sum
    (fixed order; the two user-indexed tables share their ids, the two item-indexed ones likewise).  Reference:
    models/herec.py:36-46 + experiments/herec_solver_bpr.py:108-121 under loss.backward()."""

    @staticmethod
    def forward(ctx, tables, acc, ids, need_grad, w, b, user_emb, item_emb, user_rk_bias, item_rk_bias):
        unids, inids, labels = ids
        loss, _, dw, db, g_user, g_item, flag = herec_train_raw(tables, w, b, user_emb, item_emb, user_rk_bias, item_rk_bias,
                                                                acc[0], acc[1], unids, inids, labels, need_grad)
        _defer_error(flag, 'index out of range in HeRec pairs (a user id outside the user block or an item id outside the '
                           'item block)')
        if need_grad:
            # an id out of range has zero gradient rows; -1 makes the scatter skip it
            nu, ni = user_emb.shape[0], item_emb.shape[0]
            lu, li = unids.to(torch.int64) - acc[0], inids.to(torch.int64) - acc[1]
            ctx.lu = torch.where((lu >= 0) & (lu < nu), lu, torch.full_like(lu, -1)).contiguous()
            ctx.li = torch.where((li >= 0) & (li < ni), li, torch.full_like(li, -1)).contiguous()
            ctx.grads = (dw, db, g_user, g_item)
            ctx.nums = (nu, ni)
        return loss

    @staticmethod
    def backward(ctx, g):
        dw, db, g_user, g_item = ctx.grads
        nu, ni = ctx.nums
        d = db.shape[1]
        need = ctx.needs_input_grad
        gu = g_user * g if need[6] or need[8] else None
        gi = g_item * g if need[7] or need[9] else None
        return (None, None, None, None,
                dw * g if need[4] else None,
                db * g if need[5] else None,
                _scatter_dense(ctx.lu, gu[:, :d], nu, d) if need[6] else None,
                _scatter_dense(ctx.li, gi[:, :d], ni, d) if need[7] else None,
                _scatter_dense(ctx.lu, gu[:, d:], nu, d) if need[8] else None,
                _scatter_dense(ctx.li, gi[:, d:], ni, d) if need[9] else None)


def herec_mse_loss(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias, acc_uids, acc_iids, unids,
                   inids, labels):
    """Differentiable HeRec training loss mean((pred - label)^2) of B labelled pairs, forward and backward in HIP:
    tables = the M frozen [N, D] metapath2vec tables, emb_trans_w [M, D, D] / emb_trans_b [M, D] the stacked emb_trans
    parameters (torch Linear layout), the four embedding tables [num_uids | num_iids, D].  backward() gives dense gradients
    for the six parameter tensors.  With grad disabled, or when no input requires grad, only the forward runs.  A pair with an
    id outside its block contributes nothing and raises IndexError at the next check_pending_errors().
    herec_supported(D, M, B) must hold."""
    tables = list(tables)
    if not tables or tables[0].dim() != 2 or not herec_supported(tables[0].shape[1], len(tables), unids.shape[0]):
        raise ValueError('herec_mse_loss: width / number of tables (engine.herec_supported) or batch size (B <= %d) not supported'
                         % ROWS_SCATTER_MAX)
    params = (emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias)
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in params)
    return _HerecLoss.apply(tables, (int(acc_uids), int(acc_iids)), (unids, inids, labels), need_grad, *params)


def herec_table(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias, acc_uids, acc_iids):
    """The [N, D + 4] table whose plain row dots are the HeRec scores (include/peahip.h, pea_herec_table): user row
    [user_emb, 1, c_u, 0, 0], item row [item_emb, beta_i, 1, 0, 0], zeros elsewhere.  One launch; feeds dot_predict,
    dot_rank_eval, dot_recommend_topk and dot_rank_full."""
    lib = _lib.require_device()
    tables, ptrs, lds, w, b, embs = _herec_args(tables, emb_trans_w, emb_trans_b, user_emb, item_emb, user_rk_bias, item_rk_bias)
    n, d = tables[0].shape
    out = torch.empty((n, d + 4), dtype=torch.float32, device=tables[0].device)
    _lib.check(lib.pea_herec_table(d, len(tables), ptrs, lds, _lib.ptr(w), _lib.ptr(b), _lib.ptr(embs[0]), _lib.ptr(embs[1]),
                                   _lib.ptr(embs[2]), _lib.ptr(embs[3]), int(acc_uids), embs[0].shape[0], int(acc_iids),
                                   embs[1].shape[0], n, _lib.ptr(out), _lib.current_stream()))
    return out


# ------------------------------------------------------------------------------------------------------------
# metapath2vec (csrc/walk.hip, csrc/skipgram.hip; reference models/metapath2vec.py)
# ------------------------------------------------------------------------------------------------------------
def _walk_starts(starts, device):
    starts = torch.as_tensor(starts, device=device)
    if starts.dtype != torch.int64 or starts.dim() != 1:
        raise ValueError('starts must be an int64 vector')
    return starts.contiguous()


def metapath_walks(plan, relations, starts, walk_length, seed, offset, validate=False, return_status=False):
    """int64 [len(starts), walk_length + 1] walks over `plan` (a GraphPlan built with self_loops=False): column 0 = starts, step
    t follows relation relations[(t - 1) % len(relations)] of the plan from a node to one of the nodes its CSR row holds (the
    sources of its in-edges; multi-edges drawn as often as they occur), picked by the Philox stream (seed, offset) that
    tests/walk_ref.py restates.  A node without an edge in the step's relation ends the walk: -1 from there on.  The call
    stays asynchronous; validate=True reads the device status (a synchronize) and raises IndexError if a start was outside
    [0, num_nodes) -- such a row is all -1.  return_status=True also returns the int32 [2] device tensor (walks that met a
    dead end, bad starts)."""
    lib = _lib.require_device()
    starts = _walk_starts(starts, plan.device)
    n, length = starts.numel(), int(walk_length)
    walks = torch.empty((n, length + 1), dtype=torch.int64, device=plan.device)
    status = torch.empty(2, dtype=torch.int32, device=plan.device)
    rel = (C.c_int * len(relations))(*[int(r) for r in relations])
    _lib.check(lib.pea_metapath_walks(plan._h, len(relations), rel, length, n, _lib.ptr(starts), int(seed) & (2 ** 64 - 1),
                                      int(offset) & 0xffffffff, _lib.ptr(walks), length + 1, _lib.ptr(status),
                                      _lib.current_stream()))
    if validate and int(status[1].item()) != 0:
        raise IndexError('metapath_walks: %d start nodes outside [0, %d)' % (int(status[1].item()), plan.num_nodes))
    return (walks, status) if return_status else walks


def uniform_walks(block_lo, block_n, starts, walk_length, seed, offset):
    """int64 [len(starts), walk_length + 1] "negative walks" (reference models/metapath2vec.py:123-140): column 0 = starts, column
    t >= 1 uniform over the node-id block [block_lo[s], block_lo[s] + block_n[s]) of step s = (t - 1) % len(block_lo), from the
    same Philox stream layout as metapath_walks.  `starts` decides the device."""
    lib = _lib.require_device()
    if not isinstance(starts, torch.Tensor) or not starts.is_cuda:
        raise RuntimeError('starts must live on the GPU (the HIP path has no CPU fallback)')
    starts = _walk_starts(starts, starts.device)
    n, length = starts.numel(), int(walk_length)
    walks = torch.empty((n, length + 1), dtype=torch.int64, device=starts.device)
    if len(block_lo) != len(block_n):
        raise ValueError('block_lo and block_n must have one entry per step of the cycle')
    lo = (C.c_int64 * len(block_lo))(*[int(v) for v in block_lo])
    cnt = (C.c_int64 * len(block_n))(*[int(v) for v in block_n])
    _lib.check(lib.pea_uniform_walks(len(block_lo), lo, cnt, length, n, _lib.ptr(starts), int(seed) & (2 ** 64 - 1),
                                     int(offset) & 0xffffffff, _lib.ptr(walks), length + 1, _lib.current_stream()))
    return walks


def skipgram_supported(dim, row_len, context_size, n_rows=0):
    """Whether skipgram_loss takes a table of width `dim`, rows of `row_len` ids and this context size (csrc/skipgram.hip: dim a
    multiple of 4 in 4..128, 2 <= context_size <= 16, context_size <= row_len <= 128, n_rows * row_len < 2^31); needs no device."""
    return bool(_lib.load().pea_skipgram_supported(int(dim), int(row_len), int(context_size))) and \
        int(n_rows) * int(row_len) < 2 ** 31


def _walk_rows(rw, row_len, device):
    if rw is None:
        return torch.empty((0, row_len), dtype=torch.int64, device=device)
    if rw.dtype != torch.int64 or rw.dim() != 2 or rw.shape[1] != row_len:
        raise ValueError('walks must be int64 [M, %d]' % row_len)
    if not rw.is_cuda:
        raise RuntimeError('walks must live on the GPU (the HIP path has no CPU fallback)')
    return rw if rw.stride(1) == 1 and rw.stride(0) >= row_len else rw.contiguous()


def skipgram_train_raw(weight, pos_rw, neg_rw, context_size):
    """One call of csrc/skipgram.hip.  Returns a dict of device tensors: loss [3] = (loss, pos, neg), n_valid int64 [2], grad
    [N, D] = d loss / d weight (every row written), touched int32 (ascending unique ids of the positions with an id in range;
    the first touched_count[0] entries count), touched_count int32 [1], flag (int32 scalar with storage of its own, not a view
    into the workspace: 1 if an id was >= N)."""
    lib = _lib.require_device()
    w = _block16(weight)
    rows = pos_rw if pos_rw is not None else neg_rw
    t = int(rows.shape[1])
    pos, neg = _walk_rows(pos_rw, t, w.device), _walk_rows(neg_rw, t, w.device)
    n_nodes, d, c = w.shape[0], w.shape[1], int(context_size)
    if not skipgram_supported(d, t, c, pos.shape[0] + neg.shape[0]):
        raise ValueError('skipgram: width %d, rows of %d ids, context %d not supported' % (d, t, c))
    dev = w.device
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    n_valid = torch.empty(2, dtype=torch.int64, device=dev)
    grad = torch.empty((n_nodes, d), dtype=torch.float32, device=dev)
    touched = torch.empty(max(1, min((pos.shape[0] + neg.shape[0]) * t, n_nodes)), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.pea_skipgram_workspace_bytes(pos.shape[0], neg.shape[0], t, c, d))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pea_skipgram_train(pos.shape[0], neg.shape[0], t, c, d, _lib.ptr(w), w.stride(0), n_nodes, _lib.ptr(pos),
                                      max(pos.stride(0), t), _lib.ptr(neg), max(neg.stride(0), t), _lib.ptr(loss),
                                      _lib.ptr(n_valid), _lib.ptr(grad), _lib.ptr(touched), _lib.ptr(count), _lib.ptr(flag),
                                      _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    return {'loss': loss, 'n_valid': n_valid, 'grad': grad, 'touched': touched, 'touched_count': count,
            'flag': flag[0]}


class _SkipgramLoss(torch.autograd.Function):
    """The metapath2vec loss with its whole backward from the same call (csrc/skipgram.hip); backward() scales the [N, D]
    gradient the forward left, or cuts its touched rows out as a coalesced sparse tensor."""

    @staticmethod
    def forward(ctx, weight, pos_rw, neg_rw, context_size, sparse):
        out = skipgram_train_raw(weight, pos_rw, neg_rw, context_size)
        _defer_error(out['flag'], 'index out of range in skip-gram walks (an id >= the rows of the embedding table)')
        ctx.out, ctx.sparse = out, sparse
        return out['loss'][0].clone()

    @staticmethod
    def backward(ctx, g):
        out = ctx.out
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if not ctx.sparse:
            return out['grad'] * g, None, None, None, None
        idx = out['touched'][:int(out['touched_count'].item())].to(torch.int64)       # the one host read of the sparse form
        vals = out['grad'][idx] * g
        return torch.sparse_coo_tensor(idx.unsqueeze(0), vals, out['grad'].shape, is_coalesced=True), None, None, None, None


def skipgram_loss(weight, pos_rw, neg_rw, context_size, sparse=False):
    """Differentiable metapath2vec loss (reference models/metapath2vec.py:147-172) of the embedding table weight [N, D] over
    positive and negative rows of ids, int64 [M, T] on the GPU with T >= context_size: whole walks (every row holds its
    T - context_size + 1 windows) or the reference's window layout (T == context_size).  Ids < 0 (dead-end tails) or >= N are
    skipped pair by pair and the means run over the valid pairs; an id >= N also raises IndexError at the next
    check_pending_errors(): MetaPath2Vec.forward() and .eval() call it, as do predict / rank_eval / model.eval() of the
    recommenders; the queued flag is 4 bytes of its own, the step's workspace is free again when backward() is done.  Forward and backward run in HIP, without float atomics.  backward() gives the dense [N, D]
    gradient, or with sparse=True a COALESCED torch.sparse_coo_tensor of the touched rows (bitwise the dense rows), which is
    what torch.optim.SparseAdam takes; the sparse form costs one host read of the touched-row count per step (a stream
    synchronize).  skipgram_supported(D, T, context_size, rows) must hold."""
    return _SkipgramLoss.apply(weight, pos_rw, neg_rw, int(context_size), bool(sparse))
