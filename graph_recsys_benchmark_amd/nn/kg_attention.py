"""The attention maps of the reference's KG baselines and a drop-in torch_geometric.utils.softmax, on the gfx950 kernels.

    experiments/kgat_solver_bpr.py:313-320   att_map of KGAT  (kgat_attention_map)
    experiments/kgcn_solver_bpr.py:313-319   att_map of KGCN  (kgcn_attention_map)
    torch_geometric.utils.softmax (1.5.0)     softmax(src, index, num_nodes)

Both maps are one call each (include/peahip.h pea_kg_attention): the scores, the per-destination softmax and the
write-out in the caller's COO order happen on the device with nothing of width emb stored per edge.  The plan of an
edge_index (destination-sorted CSR with edge ids) and the edge types in its slot order are built once and cached per
tensor (identity and `_version`, as kg_conv._plan_for does), so repeated epochs pay no rebuild.  There is no CPU path.
"""
import ctypes as C
import weakref

import torch

from .. import _lib

_cache = {}


def _cached(key, tensors, build):
    hit = _cache.get(key)
    if hit is not None and all(r() is t for r, t in zip(hit[0], tensors)):
        return hit[1]
    value = build()
    _cache[key] = ([weakref.ref(t, lambda _r, k=key: _cache.pop(k, None)) for t in tensors], value)
    return value


class _Plan:
    """One relation's CSR (PEA_PLAN_EDGE_IDS, no self-loop handling) over a [2, E] COO, plus the edge types of a KG in
    CSR slot order once set_types() was called."""

    def __init__(self, coo, num_nodes, gather_row_bytes):
        lib = _lib.require_device()
        coo = coo.contiguous()        # read by pea_plan_create only
        self.device = coo.device
        self.num_nodes, self.num_edges = int(num_nodes), int(coo.shape[1])
        ptrs = (C.c_void_p * 1)(coo.data_ptr())
        nedge = (C.c_int64 * 1)(self.num_edges)
        h = C.c_void_p()
        _lib.check(lib.pea_plan_create(self.num_nodes, 1, ptrs, nedge, _lib.PLAN_EDGE_IDS, int(gather_row_bytes), 0, 1,
                                       256, _lib.current_stream(), C.byref(h)))
        self._h = h
        self.types = None

    def set_types(self, edge_attr, num_types):
        col = edge_attr if edge_attr.dim() == 1 else edge_attr[:, 0]
        self.types = torch.empty(self.num_edges, dtype=torch.int32, device=self.device)
        _lib.check(_lib.load().pea_kg_edge_types(self._h, 0, _lib.ptr(col), col.stride(0), int(num_types),
                                                 _lib.ptr(self.types), _lib.current_stream()))
        self.num_types = int(num_types)
        return self

    def _ws(self, nbytes, device):
        return torch.empty(max(int(nbytes), 512), dtype=torch.uint8, device=device)

    def softmax(self, src):
        lib = _lib.load()
        out = torch.empty_like(src)
        ws = self._ws(lib.pea_edge_softmax_workspace_bytes(self._h, 0), src.device)
        _lib.check(lib.pea_edge_softmax(self._h, 0, _lib.ptr(src), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _lib.current_stream()))
        return out

    def softmax_backward(self, y, g):
        lib = _lib.load()
        out = torch.empty_like(y)
        ws = self._ws(lib.pea_edge_softmax_workspace_bytes(self._h, 0), y.device)
        _lib.check(lib.pea_edge_softmax_backward(self._h, 0, _lib.ptr(y), _lib.ptr(g), _lib.ptr(out), _lib.ptr(ws),
                                                 ws.numel(), _lib.current_stream()))
        return out

    def attention(self, mode, x, proj, r):
        lib = _lib.load()
        emb = int(x.shape[1])
        out = torch.empty(self.num_edges, dtype=torch.float32, device=x.device)
        ws = self._ws(lib.pea_kg_attention_workspace_bytes(self._h, 0, mode, emb), x.device)
        _lib.check(lib.pea_kg_attention(self._h, 0, mode, emb, _lib.ptr(x), x.stride(0), _lib.ptr(proj), _lib.ptr(r),
                                        _lib.ptr(self.types), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                        _lib.current_stream()))
        return out

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                _lib.load().pea_plan_destroy(h)
            except Exception:
                pass


def _softmax_plan(index, num_nodes):
    key = ('softmax', id(index), index._version, int(num_nodes))
    return _cached(key, [index], lambda: _Plan(torch.stack([index, index]), num_nodes, 0))


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, plan):
        y = plan.softmax(src)
        ctx.plan = plan
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return ctx.plan.softmax_backward(y, g.contiguous()), None


def softmax(src, index, num_nodes=None):
    """torch_geometric.utils.softmax (PyG 1.5.0) for a 1-D float32 CUDA `src` and int64 `index` of the same length:
    out_e = exp(src_e - max_{index == index_e}) / (sum_{index == index_e} exp(...) + 1e-16).  Differentiable in src."""
    _lib.require_device()
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise ValueError('src and index must be tensors')
    if src.dim() != 1:
        raise ValueError('src must be 1-D (a [E, heads] softmax is not supported)')
    if src.dtype != torch.float32 or index.dtype != torch.int64 or index.dim() != 1:
        raise ValueError('src must be float32 and index int64, both 1-D')
    if not src.is_cuda or not index.is_cuda:
        raise ValueError('src and index must be CUDA tensors')
    if src.numel() != index.numel():
        raise ValueError('src has %d entries, index %d' % (src.numel(), index.numel()))
    if num_nodes is None:
        num_nodes = int(index.max()) + 1 if index.numel() else 0
    if index.numel() == 0:
        return src.clone()
    return _EdgeSoftmax.apply(src.contiguous(), _softmax_plan(index, num_nodes))


def _check_kg(x, r, edge_index, edge_attr, num_nodes, proj_mat=None):
    _lib.require_device()
    for name, t in (('x', x), ('r', r), ('edge_index', edge_index), ('edge_attr', edge_attr)) + \
            ((('proj_mat', proj_mat),) if proj_mat is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError('%s must be a CUDA tensor' % name)
    if x.dim() != 2 or x.dtype != torch.float32 or r.dim() != 2 or r.dtype != torch.float32:
        raise ValueError('x and r must be float32 2-D tensors')
    emb = int(x.shape[1])
    if emb % 4 or emb > 256 or emb <= 0:
        raise ValueError('emb %d must be a multiple of 4 in (0, 256]' % emb)
    if int(r.shape[1]) != emb:
        raise ValueError('r has %d columns, x %d' % (r.shape[1], emb))
    if proj_mat is not None and (proj_mat.dtype != torch.float32 or tuple(proj_mat.shape) != (emb, emb)):
        raise ValueError('proj_mat must be float32 [%d, %d]' % (emb, emb))
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError('edge_index must be int64 [2, E]')
    if edge_attr.dtype != torch.int64 or edge_attr.dim() not in (1, 2) or edge_attr.shape[0] != edge_index.shape[1]:
        raise ValueError('edge_attr must be int64 [E, 1] (or [E]) with E = edge_index.shape[1]')
    if int(x.shape[0]) < int(num_nodes):
        raise ValueError('x has %d rows for %d nodes' % (x.shape[0], num_nodes))


def _kg_plan(edge_index, edge_attr, num_nodes, emb, num_types):
    key = ('kg', id(edge_index), edge_index._version, id(edge_attr), edge_attr._version, int(num_nodes), emb,
           int(num_types))
    return _cached(key, [edge_index, edge_attr],
                   lambda: _Plan(edge_index, num_nodes, 4 * emb).set_types(edge_attr, num_types))


def _as_input(t):
    return t.detach().contiguous()


def kgat_attention_map(x, proj_mat, r, edge_index, edge_attr, num_nodes):
    """att_map of experiments/kgat_solver_bpr.py:313-320 (detached float32 [E], the caller's edge order)."""
    _check_kg(x, r, edge_index, edge_attr, num_nodes, proj_mat)
    plan = _kg_plan(edge_index, edge_attr, num_nodes, int(x.shape[1]), r.shape[0])
    return plan.attention(_lib.KG_KGAT, _as_input(x), _as_input(proj_mat), _as_input(r))


def kgcn_attention_map(x, r, edge_index, edge_attr, num_nodes):
    """att_map of experiments/kgcn_solver_bpr.py:313-319 (detached float32 [E], the caller's edge order)."""
    _check_kg(x, r, edge_index, edge_attr, num_nodes)
    plan = _kg_plan(edge_index, edge_attr, num_nodes, int(x.shape[1]), r.shape[0])
    return plan.attention(_lib.KG_KGCN, _as_input(x), None, _as_input(r))
