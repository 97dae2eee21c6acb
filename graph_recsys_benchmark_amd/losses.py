"""One-launch training losses: each *_train_raw is a forward, its loss and the whole backward in one HIP launch (plus a
fixed-order reduction), and the autograd.Function over it hands the gradients out in backward().  A loss that validates ids
on the device returns its error flag (errors.ws_flag) and its Function queues it (errors.defer)."""
import ctypes as C

import torch

from . import _lib
from .dense_ops import _rows2d, grad_weight
from .errors import defer as _defer_error, ws_flag

ROWS_SCATTER_MAX = 16384      # positions pea_rows_scatter_sum sorts in LDS (a BPR batch of up to 5461 triples)
DOT_TRAIN_MAX_BLOCKS = 4      # column blocks pea_dot_bpr_train takes (include/peahip.h)
HEREC_MAX_TABLES = 4          # PEA_HEREC_MAX_TABLES (include/peahip.h)


def _int64_batch(batch, min_cols, what=None):
    """batch as the loss kernels read it: int64 [B, >= min_cols] with unit column stride (else copied)."""
    if batch.dtype != torch.int64 or batch.dim() != 2 or batch.shape[1] < min_cols:
        raise ValueError(what or 'batch must be int64 [B, >=%d]' % min_cols)
    return batch if batch.stride(1) == 1 else batch.contiguous()


def _block16(t):
    """t as dot_bpr_train / transr_train read it: rows with a stride that is a multiple of 4 floats and a 16-byte aligned start (a column
    block of a wider buffer qualifies); anything else is copied."""
    t = _rows2d(t.detach())
    if t.stride(0) % 4 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _workspace(query, dims, device):
    """(uint8 workspace on `device`, its size) for a launch whose pea_*_workspace_bytes entry point is `query`"""
    nbytes = int(query(*dims))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _table_arrays(tables):
    """ctypes arrays over a list of _block16 tables: (data pointers, row strides in floats, widths)"""
    k = len(tables)
    return ((C.c_void_p * k)(*[t.data_ptr() for t in tables]), (C.c_int64 * k)(*[t.stride(0) for t in tables]),
            (C.c_int * k)(*[t.shape[1] for t in tables]))


def _outputs(device, *shapes, wanted=True):
    """One float32 output per shape -- or None for each when they are not wanted (need_grad false: the kernels skip the work)"""
    return tuple(torch.empty(s, dtype=torch.float32, device=device) if wanted else None for s in shapes)


def bpr_train_raw(picked, att, fc1_w, fc1_b, fc2_w, fc2_b):
    """One launch of csrc/bpr_train.hip + the two fixed-order reductions (pea_grad_weight): returns
    (loss, grad_rows [3B, P*R], (d_att | None, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b)) for picked [3B, P, R]."""
    lib = _lib.require_device()
    n3, p_, r_ = picked.shape
    rows = picked.detach().contiguous()
    b, dev = n3 // 3, rows.device
    keep = [t.detach().contiguous() for t in (fc1_w, fc1_b, fc2_w, fc2_b)]
    att_c = att.detach().contiguous().view(-1) if att is not None else None
    loss, grad_rows, dhx, zx = _outputs(dev, (), (n3, p_ * r_), (2 * b, r_ + 4), (2 * b, 3 * r_ + 4))
    dsc, = _outputs(dev, (n3, (p_ + 3) // 4 * 4), wanted=att is not None)
    ws, ws_bytes = _workspace(lib.pea_bpr_train_workspace_bytes, (b,), dev)
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
    ws, ws_bytes = _workspace(lib.pea_rows_scatter_sum_workspace_bytes, (ids.numel(),), src.device)
    _lib.check(lib.pea_rows_scatter_sum(ids.numel(), _lib.ptr(ids), _lib.ptr(src), src.stride(0), int(num_channels), int(repr_dim),
                                        cols, _lib.ptr(dst), dst.stride(0), dst.shape[0], _lib.ptr(ws), ws_bytes, _lib.current_stream()))


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
    ptrs, lds, widths = _table_arrays(rows)
    loss, grad_rows = _outputs(dev, (), (3 * b, sum(t.shape[1] for t in rows)))
    ws, ws_bytes = _workspace(lib.pea_dot_bpr_train_workspace_bytes, (b,), dev)
    _lib.check(lib.pea_dot_bpr_train(b, len(rows), ptrs, lds, widths, n, _lib.ptr(batch), batch.stride(0), _lib.ptr(loss),
                                     _lib.ptr(grad_rows), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    return loss, grad_rows, ws_flag(ws)


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


def transr_train_raw(x, proj, r, batch, need_grad=True):
    """One launch of csrc/transr_train.hip (+ its fixed-order reduction): (loss, pos [B], neg [B], grad_rows [3B, E],
    grad_rel_rows [B, E], dproj [E, E], error flag) of the TransR-style kg_loss for x [N, E], proj [E, E], r [R, E] and the
    int64 [B, >= 4] rows (h, t+, t-, rel) of `batch`.  need_grad=False is the forward-only form: the three gradients are
    None and no backward work is done.  (The workspace holds [E, E] partials per workgroup: ws_flag clones the flag out.)"""
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
    loss, pos, neg = _outputs(dev, (), (b,), (b,))
    grad_rows, grad_rel, dproj = _outputs(dev, (3 * b, e), (b, e), (e, e), wanted=need_grad)
    ws, ws_bytes = _workspace(lib.pea_transr_train_workspace_bytes, (b, e), dev)
    _lib.check(lib.pea_transr_train(b, e, _lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(proj), _lib.ptr(r), r.stride(0),
                                    r.shape[0], _lib.ptr(batch), batch.stride(0), _lib.ptr(loss), _lib.ptr(pos), _lib.ptr(neg),
                                    _lib.ptr(grad_rows), _lib.ptr(grad_rel), _lib.ptr(dproj), _lib.ptr(ws), ws_bytes,
                                    _lib.current_stream()))
    return loss, pos, neg, grad_rows, grad_rel, dproj, ws_flag(ws)


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


# ---- CFKG (csrc/cfkg.hip, include/peahip_kge.h; reference models/cfkg.py, experiments/cfkg_solver_bpr.py:95-106)
def cfkg_supported(emb, num_rel, batch_size):
    """Whether cfkg_loss takes this width and number of relations (pea_cfkg_supported: a multiple of 4 in 4..128, 1..64
    relations) and this batch (its 3 B node positions go back through rows_scatter_sum); needs no device.  Else the caller
    stays on autograd."""
    return bool(_lib.load().pea_cfkg_supported(int(emb), int(num_rel))) and 3 * int(batch_size) <= ROWS_SCATTER_MAX


def cfkg_train_raw(x, r, batch, need_grad=True):
    """One launch of csrc/cfkg.hip (+ its fixed-order reduction): (loss, pos [B], neg [B], grad_rows [3B, E], grad_r [R, E],
    error flag) of the CFKG kg_loss for x [N, E], r [R, E] and the int64 [B, >= 4] rows (h, t+, t-, rel) of `batch`.  grad_r is
    the whole relation gradient, summed inside the launch.  need_grad=False is the forward-only form: the two gradients are
    None and no backward work is done."""
    lib = _lib.require_device()
    batch = _int64_batch(batch, 4)
    x, r = _block16(x), _block16(r)
    e, n_rel = x.shape[1], r.shape[0]
    if r.shape[1] != e or x.shape[0] < 1 or not lib.pea_cfkg_supported(e, n_rel):
        raise ValueError('cfkg_train: x [N, E] and r [R, E] with E a multiple of 4 in 4..128 and 1 <= R <= %d expected, got %s and %s'
                         % (_lib.CFKG_MAX_REL, tuple(x.shape), tuple(r.shape)))
    b, dev = batch.shape[0], x.device
    loss, pos, neg = _outputs(dev, (), (b,), (b,))
    grad_rows, grad_r = _outputs(dev, (3 * b, e), (n_rel, e), wanted=need_grad)
    ws, ws_bytes = _workspace(lib.pea_cfkg_train_workspace_bytes, (b, e, n_rel), dev)
    _lib.check(lib.pea_cfkg_train(b, e, _lib.ptr(x), x.stride(0), x.shape[0], _lib.ptr(r), r.stride(0), n_rel, _lib.ptr(batch),
                                  batch.stride(0), _lib.ptr(loss), _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(grad_rows),
                                  _lib.ptr(grad_r), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    return loss, pos, neg, grad_rows, grad_r, ws_flag(ws)


class _CfkgLoss(torch.autograd.Function):
    """loss = -(sum_b log sigmoid(pos_b) + sum_b log sigmoid(-neg_b)) of the CFKG KG phase with its whole backward from the same
    launch (csrc/cfkg.hip); backward scatters the batch's gradient rows into the dense x gradient with pea_rows_scatter_sum
    (fixed order) and hands the relation gradient out as the launch left it.  Reference: experiments/cfkg_solver_bpr.py:95-106
    under loss.backward()."""

    @staticmethod
    def forward(ctx, batch, need_grad, x, r):
        loss, _, _, grad_rows, grad_r, flag = cfkg_train_raw(x, r, batch, need_grad)
        _defer_error(flag, 'index out of range in KG quadruples')
        if need_grad:
            ctx.node_ids = batch[:, :3].reshape(-1).contiguous()
            ctx.grads = (grad_rows, grad_r)
            ctx.shape = tuple(x.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        grad_rows, grad_r = ctx.grads
        dx = dr = None
        if ctx.needs_input_grad[2]:
            dx = _scatter_dense(ctx.node_ids, grad_rows * g, *ctx.shape)
        if ctx.needs_input_grad[3]:
            dr = grad_r * g
        return None, None, dx, dr


def cfkg_loss(x, r, batch):
    """Differentiable CFKG kg_loss (models/cfkg.py) of the int64 [B, >= 4] rows (h, t+, t-, rel) of `batch`, forward and backward
    in HIP; backward() gives dense gradients for x [N, E] and r [R, E].  With grad disabled, or when no input requires grad,
    only the forward runs.  A row with an id out of range contributes nothing and raises IndexError at the next
    check_pending_errors().  cfkg_supported(E, R, B) must hold."""
    if x.dim() != 2 or r.dim() != 2 or not cfkg_supported(x.shape[1], r.shape[0], batch.shape[0]):
        raise ValueError('cfkg_loss: width (a multiple of 4 in 4..128), relations (1..%d) or batch size (3 B <= %d) not supported'
                         % (_lib.CFKG_MAX_REL, ROWS_SCATTER_MAX))
    need_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (x, r))
    return _CfkgLoss.apply(batch, need_grad, x, r)


# ---- HeRec (csrc/herec.hip; reference models/herec.py, experiments/herec_solver_bpr.py:108-121)
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
    return (tables,) + _table_arrays(tables)[:2] + (w, b, embs)


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
    loss, pred = _outputs(dev, (), (bsz,))
    dw, db, g_user, g_item = _outputs(dev, (m, d, d), (m, d), (bsz, 2 * d), (bsz, 2 * d), wanted=need_grad)
    ws, ws_bytes = _workspace(lib.pea_herec_train_workspace_bytes, (bsz, d, m), dev)
    _lib.check(lib.pea_herec_train(bsz, d, m, ptrs, lds, _lib.ptr(w), _lib.ptr(b), _lib.ptr(embs[0]), _lib.ptr(embs[1]),
                                   _lib.ptr(embs[2]), _lib.ptr(embs[3]), int(acc_uids), embs[0].shape[0], int(acc_iids),
                                   embs[1].shape[0], n, _lib.ptr(unids), _lib.ptr(inids), _lib.ptr(labels), _lib.ptr(loss),
                                   _lib.ptr(pred), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(g_user), _lib.ptr(g_item), _lib.ptr(ws),
                                   ws_bytes, _lib.current_stream()))
    return loss, pred, dw, db, g_user, g_item, ws_flag(ws)


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


# ---- NFM (csrc/nfm.hip, include/peahip_fm.h; reference models/nfm.py over torchfm's NeuralFactorizationMachineModel)
NFM_DENSE = ('w1', 'b1', 'w2', 'b2', 'bias0', 'bn1_w', 'bn1_b', 'bn2_w', 'bn2_b')      # the dense gradients of nfm_train_raw


def nfm_supported(emb_dim, hidden_size, batch_size=2):
    """Whether nfm_mse_loss / nfm_fold / the nfm scorers take these widths (include/peahip_fm.h, pea_nfm_supported: multiples
    of 4 in 4..128) and this batch (2 <= B, torch's BatchNorm refuses one row; its 2 B positions go back through
    rows_scatter_sum); needs no device."""
    return (bool(_lib.load().pea_nfm_supported(int(emb_dim), int(hidden_size))) and 2 <= int(batch_size)
            and 2 * int(batch_size) <= ROWS_SCATTER_MAX)


def _nfm_dense(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2):
    """The NFM tensors as pea_nfm_* read them: emb as a 16-byte aligned block with a row stride that is a multiple of 4, the
    rest detached and contiguous; bn = (weight, bias, running_mean, running_var), the running buffers as they are (the launch
    updates them in place)."""
    emb = _block16(emb)
    e, n = emb.shape[1], emb.shape[0]
    flat = [t.detach().contiguous() for t in (lin, bias0, bn1[0], bn1[1], w1, b1, bn2[0], bn2[1], w2, b2)]
    h = flat[4].shape[0]
    if (flat[0].numel() != n or flat[1].numel() != 1 or tuple(flat[4].shape) != (h, e) or flat[5].numel() != h or flat[8].numel() != h
            or flat[9].numel() != 1 or any(t.numel() != e for t in (flat[2], flat[3], bn1[2], bn1[3]))
            or any(t.numel() != h for t in (flat[6], flat[7], bn2[2], bn2[3]))):
        raise ValueError('nfm: emb [U + I, E], lin [U + I, 1], W1 [H, E], w2 [1, H] and batch normalisations of E and H columns expected')
    if any(t.dtype != torch.float32 for t in [emb] + flat + list(bn1[2:]) + list(bn2[2:])):
        raise ValueError('nfm: float32 tensors expected')
    if not all(t.is_contiguous() for t in list(bn1[2:]) + list(bn2[2:])):
        raise ValueError('nfm: the running buffers must be contiguous')
    return emb, flat, e, h


def nfm_train_raw(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2, num_users, uids, iids, labels, keep=None, keep_scale=1.0,
                  need_grad=True, update_running=True, eps=1e-5, momentum=0.1):
    """The training step of csrc/nfm.hip for B labelled pairs of LOCAL ids: a dict with loss, pred [B], batch_stats (mean1,
    var1 [E], mean2, var2 [H]: the batch's means and biased variances), grads {name: tensor} over NFM_DENSE, grad_rows
    [2B, E + 4] (row b the user position of pair b, row B + b the item position: [d emb row | d lin, 0, 0, 0]), pos_ids [2B]
    (the table rows of those positions, -1 for a pair with an id out of range: what rows_scatter_sum takes), dense (the buffer
    grads views) and the error flag.  bn1 / bn2 = (weight, bias, running_mean, running_var); with update_running the running buffers are updated in
    place as torch's BatchNorm1d does in training mode.  keep = (keep1 [B, E], keep2 [B, H]) uint8 / bool dropout masks with
    keep_scale = 1 / (1 - p), or None.  need_grad=False: forward only, grads and grad_rows are None."""
    lib = _lib.require_device()
    emb, flat, e, h = _nfm_dense(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2)
    dev, n = emb.device, emb.shape[0]
    uids, iids = uids.to(torch.int64).contiguous(), iids.to(torch.int64).contiguous()
    labels = labels.to(torch.float32).contiguous()
    if uids.dim() != 1 or uids.shape != iids.shape or uids.shape != labels.shape:
        raise ValueError('nfm: uids, iids and labels must be 1-d of equal length')
    bsz = uids.shape[0]
    if not nfm_supported(e, h, bsz):
        raise ValueError('nfm_train: widths (%d, %d) or batch size %d not supported (engine.nfm_supported)' % (e, h, bsz))
    k1 = k2 = None
    if keep is not None:
        k1, k2 = ((k.view(torch.uint8) if k.dtype == torch.bool else k.to(torch.uint8)).contiguous() for k in keep)
        if tuple(k1.shape) != (bsz, e) or tuple(k2.shape) != (bsz, h):
            raise ValueError('nfm: keep masks [B, E] and [B, H] expected')
    loss, pred, stats = _outputs(dev, (), (bsz,), (2 * e + 2 * h,))
    dense, rows = _outputs(dev, (h * e + 2 * h + 4 + 2 * e + 2 * h,), (2 * bsz, e + 4), wanted=need_grad)
    pos = torch.empty(2 * bsz, dtype=torch.int64, device=dev) if need_grad else None
    ws, ws_bytes = _workspace(lib.pea_nfm_train_workspace_bytes, (bsz, e, h), dev)
    _lib.check(lib.pea_nfm_train(bsz, e, h, int(num_users), n - int(num_users), _lib.ptr(emb), emb.stride(0), _lib.ptr(flat[0]),
                                 _lib.ptr(flat[1]), _lib.ptr(flat[2]), _lib.ptr(flat[3]), _lib.ptr(bn1[2]), _lib.ptr(bn1[3]),
                                 _lib.ptr(flat[4]), _lib.ptr(flat[5]), _lib.ptr(flat[6]), _lib.ptr(flat[7]), _lib.ptr(bn2[2]),
                                 _lib.ptr(bn2[3]), _lib.ptr(flat[8]), _lib.ptr(flat[9]), float(eps), float(momentum),
                                 int(bool(update_running)), _lib.ptr(uids), _lib.ptr(iids), _lib.ptr(labels), _lib.ptr(k1), _lib.ptr(k2),
                                 float(keep_scale), _lib.ptr(loss), _lib.ptr(pred), _lib.ptr(stats), _lib.ptr(dense), _lib.ptr(rows),
                                 _lib.ptr(pos), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    return {'loss': loss, 'pred': pred, 'dense': dense, 'grads': _nfm_dense_views(dense, e, h) if need_grad else None,
            'grad_rows': rows, 'pos_ids': pos, 'flag': ws_flag(ws),
            'batch_stats': (stats[:e], stats[e:2 * e], stats[2 * e:2 * e + h], stats[2 * e + h:])}


def _nfm_dense_views(dense, e, h):
    """{name: view} over NFM_DENSE of the d_dense buffer of pea_nfm_train (include/peahip_fm.h)"""
    o = h * e + 2 * h + 4
    return {'w1': dense[:h * e].view(h, e), 'b1': dense[h * e:h * e + h], 'w2': dense[h * e + h:h * e + 2 * h].view(1, h),
            'b2': dense[h * e + 2 * h:h * e + 2 * h + 1], 'bias0': dense[h * e + 2 * h + 1:h * e + 2 * h + 2],
            'bn1_w': dense[o:o + e], 'bn1_b': dense[o + e:o + 2 * e], 'bn2_w': dense[o + 2 * e:o + 2 * e + h],
            'bn2_b': dense[o + 2 * e + h:o + 2 * e + 2 * h]}


def nfm_position_ids(num_users, num_items, uids, iids):
    """The 2 B rows of the [U + I] tables that B pairs of local ids read, users first; -1 (skipped by rows_scatter_sum) for
    both positions of a pair with an id out of range."""
    u, i = uids.to(torch.int64), iids.to(torch.int64)
    ok = (u >= 0) & (u < num_users) & (i >= 0) & (i < num_items)
    bad = torch.full_like(u, -1)
    return torch.cat([torch.where(ok, u, bad), torch.where(ok, i + num_users, bad)]).contiguous()


class _NfmLoss(torch.autograd.Function):
    """loss = mean_b (sigmoid(y_b) - label_b)^2 of the NFM score with its whole backward from the same chain of launches
    (csrc/nfm.hip); backward scatters the 2 B position rows into ONE dense [U + I, E + 4] buffer with pea_rows_scatter_sum
    (fixed order): its first E columns are emb's gradient, column E is lin's.  Reference: models/nfm.py:16-33 under
    loss.backward()."""

    @staticmethod
    def forward(ctx, ids, opts, emb, lin, bias0, bn1_w, bn1_b, w1, b1, bn2_w, bn2_b, w2, b2):
        uids, iids, labels = ids
        num_users = int(opts['num_users'])
        out = nfm_train_raw(emb, lin, bias0, (bn1_w, bn1_b) + tuple(opts['bn1_running']), w1, b1,
                            (bn2_w, bn2_b) + tuple(opts['bn2_running']), w2, b2, num_users, uids, iids, labels, keep=opts.get('keep'),
                            keep_scale=opts.get('keep_scale', 1.0), need_grad=opts['need_grad'],
                            update_running=opts.get('update_running', True), eps=opts.get('eps', 1e-5),
                            momentum=opts.get('momentum', 0.1))
        _defer_error(out['flag'], 'index out of range in NFM pairs (a user id outside [0, num_users) or an item id outside '
                                  '[0, num_items))')
        if opts['need_grad']:
            ctx.out = out
            ctx.shapes = (tuple(emb.shape), tuple(lin.shape), w1.shape[0])
        opts['pred'] = out['pred']
        return out['loss']

    @staticmethod
    def backward(ctx, g):
        (n, e), lin_shape, h = ctx.shapes
        need = ctx.needs_input_grad
        d_emb = d_lin = None
        if need[2] or need[3]:
            table = _scatter_dense(ctx.out['pos_ids'], ctx.out['grad_rows'] * g, n, e + 4)
            d_emb = table[:, :e] if need[2] else None
            d_lin = table[:, e].reshape(lin_shape) if need[3] else None
        grads = _nfm_dense_views(ctx.out['dense'] * g, e, h)        # one multiply for the nine dense gradients

        def dense(k, name):
            return grads[name] if need[k] else None
        return (None, None, d_emb, d_lin, dense(4, 'bias0'), dense(5, 'bn1_w'), dense(6, 'bn1_b'), dense(7, 'w1'), dense(8, 'b1'),
                dense(9, 'bn2_w'), dense(10, 'bn2_b'), dense(11, 'w2'), dense(12, 'b2'))


def nfm_mse_loss(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2, num_users, uids, iids, labels, keep=None, keep_scale=1.0,
                 update_running=True, eps=1e-5, momentum=0.1, info=None):
    """Differentiable NFM training loss mean((sigmoid(y) - label)^2) of B labelled pairs of LOCAL ids, forward and backward in
    HIP.  bn1 / bn2 = (weight, bias, running_mean, running_var) of the two BatchNorm1d: the running buffers are updated in place
    (update_running), the caller counts num_batches_tracked.  keep = (keep1 [B, E], keep2 [B, H]) dropout masks with keep_scale
    = 1 / (1 - p), or None: nothing is drawn here.  backward() gives dense gradients for the eleven parameter tensors.  With
    grad disabled, or when no input requires grad, only the forward runs (the running buffers are still updated, as torch
    does).  A pair with an id out of range raises IndexError at the next check_pending_errors().  info: a dict that receives
    'pred' [B].  nfm_supported(E, H, B) must hold."""
    if emb.dim() != 2 or w1.dim() != 2 or not nfm_supported(emb.shape[1], w1.shape[0], uids.shape[0]):
        raise ValueError('nfm_mse_loss: widths (multiples of 4 in 4..128) or batch size (2 <= B, 2 B <= %d) not supported'
                         % ROWS_SCATTER_MAX)
    params = (emb, lin, bias0, bn1[0], bn1[1], w1, b1, bn2[0], bn2[1], w2, b2)
    opts = {'num_users': num_users, 'bn1_running': bn1[2:], 'bn2_running': bn2[2:], 'keep': keep, 'keep_scale': keep_scale,
            'update_running': update_running, 'eps': eps, 'momentum': momentum,
            'need_grad': torch.is_grad_enabled() and any(t.requires_grad for t in params)}
    loss = _NfmLoss.apply((uids, iids, labels), opts, *params)
    if info is not None:
        info['pred'] = opts['pred']
    return loss
