"""metapath2vec on the device (csrc/walk.hip, csrc/skipgram.hip; reference models/metapath2vec.py): the walk samplers and
the skip-gram training step."""
import ctypes as C

import torch

from . import _lib
from .errors import defer as _defer_error
from .losses import _block16, _workspace


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
    ws, ws_bytes = _workspace(lib.pea_skipgram_workspace_bytes, (pos.shape[0], neg.shape[0], t, c, d), dev)
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
    recommenders; the queued flag is 4 bytes of its own, the step's workspace is free again when backward() is done.  Forward
    and backward run in HIP, without float atomics.  backward() gives the dense [N, D] gradient, or with sparse=True a
    COALESCED torch.sparse_coo_tensor of the touched rows (bitwise the dense rows), which is what torch.optim.SparseAdam
    takes; the sparse form costs one host read of the touched-row count per step (a stream synchronize).
    skipgram_supported(D, T, context_size, rows) must hold."""
    return _SkipgramLoss.apply(weight, pos_rw, neg_rw, int(context_size), bool(sparse))
