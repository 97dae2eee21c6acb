"""Scoring and evaluation on a table of node rows: the BPR score of a batch, the entity regulariser, the ablation fusion and
the five scoring operations (predict, candidate ranking, catalogue top-K, catalogue ranking, catalogue ranking with several
positives per user).  Each has ONE host body for the fc1 / fc2 scorer (pea_*) and the inner product (pea_dot_*): `fc` is the
four fc tensors or None (_scorer)."""
import ctypes as C

import torch

from . import _lib
from .errors import check as check_pending_errors, defer as _defer_error, ws_flag
from .losses import _int64_batch


def bpr_score(repr_, triples, fc1_w, fc1_b, fc2_w, fc2_b, want_preds=False, validate=False):
    """loss = -sum(log(sigmoid(pos - neg))) over rows (u, i+, i-) of `triples` (reference models/base.py:46-48,
    208-214).  Returns a 0-dim tensor (and pos, neg [B] when asked).  A triple with a node id out of range makes the
    loss NaN on the device and IndexError at the next check_pending_errors() (validate=True: at once)."""
    lib = _lib.require_device()
    triples = _int64_batch(triples, 3, 'triples must be int64 [B, >=3]')
    b, r, dev = triples.shape[0], repr_.shape[1], repr_.device
    ws_bytes = int(lib.pea_bpr_workspace_bytes(b))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pos, neg = (torch.empty(b, dtype=torch.float32, device=dev) if want_preds else None for _ in range(2))
    args = [t.detach().contiguous() for t in (repr_, fc1_w, fc1_b, fc2_w, fc2_b)]
    _lib.check(lib.pea_bpr_score(b, r, repr_.shape[0], _lib.ptr(args[0]), _lib.ptr(triples), triples.stride(0),
                                 _lib.ptr(args[1]), _lib.ptr(args[2]), _lib.ptr(args[3]), _lib.ptr(args[4]),
                                 _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(loss), _lib.ptr(ws), ws_bytes,
                                 _lib.current_stream()))
    _defer_error(ws_flag(ws))
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
    batch9 = _int64_batch(batch9, 9, 'entity-aware batches are int64 [B, 9] (u, i+, i-, 6 entity columns)')
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
    _defer_error(ws_flag(ws))
    return reg, rows


def entity_reg(x, batch9):
    """Entity-aware regulariser (reference models/base.py:50-73) in one HIP launch; differentiable with respect to x
    when x requires grad (gradient rows come out of the same launch)."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _EntityReg.apply(x, batch9)
    return _entity_launch(x, batch9, want_grad=False)[0]


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


def _check_scored(rc):
    """The return code of a scoring entry point: a node id outside [0, num_nodes) is the reference's IndexError."""
    if rc == -2:
        raise IndexError(_lib.last_error())
    _lib.check(rc)


def _rank_io(unids, cand, dev, variants=()):
    """unids / cand as contiguous int64 and the outputs of an evaluator of cand's [U, C] (its last two dimensions) over
    `variants` tables: (scores [*variants, U, C], rank int32 / auc / loss [*variants, U]).  For the candidate evaluators
    (rank_eval, rank_eval_multi, dot_rank_eval); the catalogue and pair bodies have other outputs."""
    unids = unids.to(torch.int64).contiguous()
    cand = cand.to(torch.int64).contiguous()
    u, c = cand.shape[-2:]
    lead = tuple(variants) + (u,)
    outs = (torch.empty(lead + (c,), dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.int32, device=dev),
            torch.empty(lead, dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.float32, device=dev))
    return unids, cand, outs


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


# ---- the four scoring operations: one body each, two public names each
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


def _scorer(op, repr_, fc):
    """The two forms of scoring operation `op` behind one call.  Returns (table, run, query): run(head, tail) launches
    pea_dot_<op>(*head, *tail, stream) for fc None (the inner product, over a table that _dot_table has checked), else
    pea_<op>(*head, the four fc pointers, *tail, stream): the fc pointers sit where include/peahip.h has them.  run raises like
    _check_scored; query is the form's workspace query for `op`: rank_multi_workspace_bytes for 'rank_full_multi'
    (include/peahip_eval.h), topk_workspace_bytes for the rest."""
    lib = _lib.require_device()
    if fc is None:
        prefix, table, fc = 'pea_dot_', repr_, ()
    else:
        prefix, table, fc = 'pea_', repr_.detach().contiguous(), [t.detach().contiguous() for t in fc]

    def run(head, tail):
        _check_scored(getattr(lib, prefix + op)(*head, *[_lib.ptr(t) for t in fc], *tail, _lib.current_stream()))
    query = 'rank_multi_workspace_bytes' if op == 'rank_full_multi' else 'topk_workspace_bytes'
    return table, run, getattr(lib, prefix + query)


def _exclusion_csr(exclude, n_users, device, owner):
    """exclude checked and contiguous, or (None, None); owner ('table' or 'fold') is what must share its device"""
    if exclude is None:
        return None, None
    rowptr, items = exclude
    if rowptr.dtype != torch.int64 or items.dtype != torch.int64 or rowptr.numel() != n_users + 1:
        raise ValueError('exclude is (rowptr int64 [U + 1], items int64) -- see utils.interactions.seen_items_csr')
    if rowptr.device != device or items.device != device:
        raise ValueError('the exclusion lists must live on the device of the %s' % owner)
    rowptr, items = rowptr.contiguous(), items.contiguous()
    if items.numel() == 0:                  # a valid pointer for the C side even when nobody has seen anything
        items = torch.zeros(1, dtype=torch.int64, device=device)
    return rowptr, items


def _positives_csr(pos_rowptr, pos_items, n_users, device, owner):
    """the positives CSR (pos_rowptr int64 [n_users + 1], pos_items int64 [Q]) checked and contiguous"""
    for t in (pos_rowptr, pos_items):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError('positives are (pos_rowptr int64 [U + 1], pos_items int64 [Q]) -- see utils.interactions.positives_csr')
        if t.device != device:
            raise ValueError('the positives must live on the device of the %s' % owner)
    if pos_rowptr.numel() != n_users + 1:
        raise ValueError('pos_rowptr must have one entry per requested user and one more')
    return pos_rowptr.contiguous(), pos_items.contiguous()


def _rank_outputs(u, dev):
    """(rank int32, auc, pos_score) [u] of the all-item rank forms"""
    return (torch.empty(u, dtype=torch.int32, device=dev), torch.empty(u, dtype=torch.float32, device=dev),
            torch.empty(u, dtype=torch.float32, device=dev))


def _multi_outputs(u, q, dev):
    """(above int32 [q], below int32 [q], pos_score [q], n_neg int32 [u]) of the multi-positive rank forms"""
    return (torch.empty(q, dtype=torch.int32, device=dev), torch.empty(q, dtype=torch.int32, device=dev),
            torch.empty(q, dtype=torch.float32, device=dev), torch.empty(u, dtype=torch.int32, device=dev))


def _ptr_or_spare(q, dev):
    """_lib.ptr for the [Q] arrays of a multi-positive call; with Q == 0 a spare address, valid where there is nothing to read"""
    if q:
        return _lib.ptr
    spare = torch.zeros(2, dtype=torch.int64, device=dev)
    return lambda t: _lib.ptr(spare)


def _catalogue_args(repr_, unids, item_range, exclude):
    unids = unids.to(torch.int64).contiguous()
    if unids.dim() != 1:
        raise ValueError('unids must be 1-d')
    item_lo, item_hi = int(item_range[0]), int(item_range[1])
    if item_hi < item_lo:
        raise ValueError('item_range is (first item node id, one past the last)')
    rowptr, items = _exclusion_csr(exclude, unids.numel(), repr_.device, 'table')
    return unids, item_lo, item_hi - item_lo, rowptr, items


def _catalogue_ws(query, u, n_items, k, r, dev):
    """(workspace, its size as the C side wants it) of a catalogue scan keeping k items per user"""
    ws_bytes = int(query(u, n_items, k, r))
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev), ws_bytes


def _predict(repr_, unids, inids, fc):
    unids = unids.to(torch.int64).contiguous()
    inids = inids.to(torch.int64).contiguous()
    if unids.shape != inids.shape or unids.dim() != 1:
        raise ValueError('unids / inids must be 1-d of equal length')
    table, run, _ = _scorer('predict', repr_, fc)
    out = torch.empty(unids.shape[0], dtype=torch.float32, device=table.device)
    run((unids.shape[0], table.shape[1], table.shape[0], _lib.ptr(table), _lib.ptr(unids), _lib.ptr(inids)), (_lib.ptr(out),))
    return out


def _rank_eval(repr_, unids, cand, fc):
    table, run, _ = _scorer('rank_eval', repr_, fc)
    unids, cand, outs = _rank_io(unids, cand, table.device)
    run((cand.shape[0], cand.shape[1], table.shape[1], table.shape[0], _lib.ptr(table), _lib.ptr(unids), _lib.ptr(cand)),
        [_lib.ptr(t) for t in outs])
    return outs


def _recommend_topk(repr_, unids, k, item_range, exclude, fc):
    table, run, query = _scorer('recommend_topk', repr_, fc)
    unids, item_lo, n_items, rowptr, items = _catalogue_args(table, unids, item_range, exclude)
    u, k, r, dev = unids.shape[0], int(k), table.shape[1], table.device
    out_items = torch.empty((u, max(k, 0)), dtype=torch.int64, device=dev)
    out_scores = torch.empty((u, max(k, 0)), dtype=torch.float32, device=dev)
    ws, ws_bytes = _catalogue_ws(query, u, n_items, k, r, dev)
    run((u, k, r, table.shape[0], _lib.ptr(table), _lib.ptr(unids), item_lo, n_items, _lib.ptr(rowptr), _lib.ptr(items)),
        (_lib.ptr(out_items), _lib.ptr(out_scores), _lib.ptr(ws), ws_bytes))
    return out_items, out_scores


def _rank_call(run, query, query_args, table, unids, pos_ptrs, catalogue, out_ptrs):
    """What the two all-item rank forms share once their arguments are checked: the workspace of query(*query_args) bytes and the
    call itself (one set of kernels on the C side too: include/peahip_eval.h).  catalogue: what _catalogue_args returns after unids."""
    item_lo, n_items, rowptr, items = catalogue
    ws_bytes = int(query(*query_args))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=table.device)
    run((unids.shape[0], table.shape[1], table.shape[0], _lib.ptr(table), _lib.ptr(unids), *pos_ptrs, item_lo, n_items, _lib.ptr(rowptr),
         _lib.ptr(items)), (*out_ptrs, _lib.ptr(ws), ws_bytes))


def _rank_full(repr_, unids, pos_items, item_range, exclude, fc):
    table, run, query = _scorer('rank_full', repr_, fc)
    unids, *catalogue = _catalogue_args(table, unids, item_range, exclude)
    pos_items = pos_items.to(torch.int64).contiguous()
    if pos_items.shape != unids.shape:
        raise ValueError('one positive per requested user')
    u, r = unids.shape[0], table.shape[1]
    outs = _rank_outputs(u, table.device)
    _rank_call(run, query, (u, catalogue[1], 1, r), table, unids, (_lib.ptr(pos_items),), catalogue, [_lib.ptr(t) for t in outs])
    return outs


def _rank_full_multi(repr_, unids, pos_rowptr, pos_items, item_range, exclude, fc):
    table, run, query = _scorer('rank_full_multi', repr_, fc)
    unids, *catalogue = _catalogue_args(table, unids, item_range, exclude)
    u, r, dev = unids.shape[0], table.shape[1], table.device
    pos_rowptr, pos_items = _positives_csr(pos_rowptr, pos_items, u, dev, 'table')
    q = pos_items.numel()
    above, below, pos_score, n_neg = outs = _multi_outputs(u, q, dev)
    if u == 0:                                  # nobody asked: an empty tensor has no address to hand to the C side
        return outs
    at = _ptr_or_spare(q, dev)
    _rank_call(run, query, (u, q, catalogue[1], r), table, unids, (_lib.ptr(pos_rowptr), at(pos_items), q), catalogue,
               (at(above), at(below), at(pos_score), _lib.ptr(n_neg)))
    return outs


def predict(repr_, unids, inids, fc1_w, fc1_b, fc2_w, fc2_b):
    """fc2(relu(fc1([repr[u] || repr[i]]))) -> [B, 1]  (reference models/base.py:208-214)."""
    check_pending_errors()
    return _predict(repr_, unids, inids, (fc1_w, fc1_b, fc2_w, fc2_b)).view(-1, 1)


def dot_predict(repr_, unids, inids):
    """sum(repr[u] * repr[i]) -> [B]  (reference models/kgat.py, kgcn.py, ngcf.py: predict), as one fma chain over the
    columns in ascending order (include/peahip.h, pea_dot_predict)."""
    check_pending_errors()
    return _predict(_dot_table(repr_), unids, inids, None)


def rank_eval(repr_, unids, cand, fc1_w, fc1_b, fc2_w, fc2_b):
    """Batched evaluator (reference solvers.py:56-96): cand [U, C], column 0 = the held-out positive.
    Returns scores [U, C], rank of the positive [U] (int32), auc [U], eval loss [U]."""
    check_pending_errors()
    return _rank_eval(repr_, unids, cand, (fc1_w, fc1_b, fc2_w, fc2_b))


def dot_rank_eval(repr_, unids, cand):
    """rank_eval with the inner-product scorer: cand [U, C], column 0 = the held-out positive.  Returns scores [U, C], rank
    of the positive [U] (int32), auc [U], eval loss [U]."""
    check_pending_errors()
    table = _dot_table(repr_)
    if cand.dim() != 2 or unids.dim() != 1 or cand.shape[0] != unids.shape[0]:
        raise ValueError('cand must be [U, C] with one row per user of unids')
    return _rank_eval(table, unids, cand, None)


def recommend_topk(repr_, unids, k, item_range, fc1_w, fc1_b, fc2_w, fc2_b, exclude=None):
    """The k best items of the catalogue item_range = (lo, hi) (node ids [lo, hi)) for every user of `unids`, scored
    like predict (reference models/base.py:208-214) and ordered by (score descending, node id ascending); `exclude`
    = (rowptr [U + 1], items) names per requested user the items to leave out (utils.interactions.seen_items_csr).
    Returns (items int64 [U, k], scores float32 [U, k]); a user with fewer than k eligible items gets (-1, -inf) in the
    tail.  One pass over the catalogue on the device (include/peahip.h, pea_recommend_topk); the [U, items] score matrix
    is never written."""
    check_pending_errors()
    return _recommend_topk(repr_, unids, k, item_range, exclude, (fc1_w, fc1_b, fc2_w, fc2_b))


def dot_recommend_topk(repr_, unids, k, item_range, exclude=None):
    """recommend_topk with the inner-product scorer: the k best items of the catalogue item_range = (lo, hi) for every user
    of `unids`, ordered by (score descending, node id ascending), `exclude` = (rowptr [U + 1], items) left out.  Returns
    (items int64 [U, k], scores float32 [U, k]) with a (-1, -inf) tail.  The catalogue scan is an MFMA GEMM whose score
    tiles are selected from in registers (include/peahip.h, pea_dot_recommend_topk); the [U, items] score matrix is never
    written."""
    check_pending_errors()
    return _recommend_topk(_dot_table(repr_), unids, k, item_range, exclude, None)


def rank_full(repr_, unids, pos_items, item_range, fc1_w, fc1_b, fc2_w, fc2_b, exclude=None):
    """All-item evaluation (the protocol of reference solvers.py:56-96 with EVERY eligible item as a negative instead of
    99 sampled ones): per user the rank of the held-out positive = number of eligible other items scoring strictly
    higher, auc = share of them scoring strictly lower, and the positive's score.  Returns (rank int32 [U], auc [U],
    pos_score [U]).  include/peahip.h, pea_rank_full."""
    check_pending_errors()
    return _rank_full(repr_, unids, pos_items, item_range, exclude, (fc1_w, fc1_b, fc2_w, fc2_b))


def dot_rank_full(repr_, unids, pos_items, item_range, exclude=None):
    """rank_full with the inner-product scorer: per user the number of eligible other items scoring strictly higher than
    the held-out positive, the share scoring strictly lower, and the positive's score.  Returns (rank int32 [U], auc [U],
    pos_score [U]).  include/peahip.h, pea_dot_rank_full."""
    check_pending_errors()
    return _rank_full(_dot_table(repr_), unids, pos_items, item_range, exclude, None)


def rank_full_multi(repr_, unids, pos_rowptr, pos_items, item_range, fc1_w, fc1_b, fc2_w, fc2_b, exclude=None):
    """rank_full for users with any number of held-out positives, in one catalogue scan (include/peahip_eval.h,
    pea_rank_full_multi).  The positives are a CSR (pos_rowptr int64 [U + 1], pos_items int64 [Q]) on the table's device,
    every row strictly ascending (utils.interactions.positives_csr); a user's negatives are the catalogue items in neither
    its exclusion row nor its positive row.  Returns, in the flat order of pos_items, (above int32 [Q] = negatives scoring
    strictly higher, below int32 [Q] = negatives scoring strictly lower, pos_score [Q]) and n_neg int32 [U]: the integers
    rank_full gives for (user, positive j) when the user's other positives are excluded too."""
    check_pending_errors()
    return _rank_full_multi(repr_, unids, pos_rowptr, pos_items, item_range, exclude, (fc1_w, fc1_b, fc2_w, fc2_b))


def dot_rank_full_multi(repr_, unids, pos_rowptr, pos_items, item_range, exclude=None):
    """rank_full_multi with the inner-product scorer (include/peahip_eval.h, pea_dot_rank_full_multi): (above int32 [Q],
    below int32 [Q], pos_score [Q], n_neg int32 [U])."""
    check_pending_errors()
    return _rank_full_multi(_dot_table(repr_), unids, pos_rowptr, pos_items, item_range, exclude, None)


# ---- NFM (csrc/nfm.hip, include/peahip_fm.h): the eval-mode fold and the pair scorer over it
NFM_ID_MESSAGE = 'index out of range in NFM pairs (a user id outside [0, num_users) or an item id outside [0, num_items))'


class NfmFolded:
    """The eval-mode NFM as the scorer reads it: emb [U + I, E] (a 16-byte aligned block), lin [U + I], the folded first
    layer w [H, E] / b [H], w2 [H], the scalar bias [1], and the block sizes."""

    def __init__(self, emb, lin, w, b, w2, bias, num_users):
        self.emb, self.lin, self.w, self.b, self.w2, self.bias = emb, lin, w, b, w2, bias
        self.num_users, self.num_items = int(num_users), int(emb.shape[0]) - int(num_users)

    @property
    def device(self):
        return self.emb.device


def nfm_fold_torch(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2, num_users, eps=1e-5):
    """nfm_fold in torch ops, on any device and in the tensors' dtype: the same three products in the same association."""
    s1 = bn1[0] / torch.sqrt(bn1[3] + eps)
    t1 = bn1[1] - bn1[2] * s1
    s2 = bn2[0] / torch.sqrt(bn2[3] + eps)
    t2 = bn2[1] - bn2[2] * s2
    w = (s2[:, None] * w1) * s1[None, :]
    b = s2 * (w1 @ t1 + b1) + t2
    return NfmFolded(emb.detach(), lin.detach().reshape(-1), w.detach(), b.detach(), w2.detach().reshape(-1),
                     (bias0 + b2).detach().reshape(1), num_users)


def nfm_fold(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2, num_users, eps=1e-5):
    """The eval-mode MLP of NFM folded into one affine map and a relu (include/peahip_fm.h, pea_nfm_fold), one launch:
    bn = (weight, bias, running_mean, running_var).  Returns the NfmFolded the nfm scorers take."""
    from .losses import _nfm_dense
    lib = _lib.require_device()
    emb, flat, e, h = _nfm_dense(emb, lin, bias0, bn1, w1, b1, bn2, w2, b2)
    dev = emb.device
    w, b, bias = (torch.empty(s, dtype=torch.float32, device=dev) for s in ((h, e), (h,), (1,)))
    _lib.check(lib.pea_nfm_fold(e, h, _lib.ptr(flat[4]), _lib.ptr(flat[5]), _lib.ptr(flat[2]), _lib.ptr(flat[3]), _lib.ptr(bn1[2]),
                                _lib.ptr(bn1[3]), _lib.ptr(flat[6]), _lib.ptr(flat[7]), _lib.ptr(bn2[2]), _lib.ptr(bn2[3]),
                                _lib.ptr(flat[1]), _lib.ptr(flat[9]), float(eps), _lib.ptr(w), _lib.ptr(b), _lib.ptr(bias),
                                _lib.current_stream()))
    return NfmFolded(emb, flat[0].reshape(-1), w, b, flat[8].reshape(-1), bias, num_users)


def _nfm_score(fold, mode, uids, iids, n_users, c, lo, want_logits, want_pred, want_rank):
    lib = _lib.require_device()
    dev = fold.device
    e, h = fold.emb.shape[1], fold.w.shape[0]
    if not lib.pea_nfm_supported(e, h):
        raise ValueError('nfm scorer: widths (%d, %d) not supported (engine.nfm_supported)' % (e, h))
    shape = (n_users,) if mode == _lib.NFM_PAIRS else (n_users, c)
    logits = torch.empty(shape, dtype=torch.float32, device=dev) if want_logits or want_rank else None
    pred = torch.empty(shape, dtype=torch.float32, device=dev) if want_pred else None
    rank = torch.empty(n_users, dtype=torch.int32, device=dev) if want_rank else None
    auc = torch.empty(n_users, dtype=torch.float32, device=dev) if want_rank else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.pea_nfm_score(mode, n_users, c, lo, e, h, fold.num_users, fold.num_items, _lib.ptr(fold.emb), fold.emb.stride(0),
                                 _lib.ptr(fold.lin), _lib.ptr(fold.w), _lib.ptr(fold.b), _lib.ptr(fold.w2), _lib.ptr(fold.bias),
                                 _lib.ptr(uids), _lib.ptr(iids), _lib.ptr(logits), _lib.ptr(pred), _lib.ptr(rank), _lib.ptr(auc),
                                 _lib.ptr(flag), _lib.current_stream()))
    _defer_error(flag, NFM_ID_MESSAGE)
    return logits, pred, rank, auc


def nfm_predict(fold, uids, iids, logits=False):
    """pred [B] = sigmoid(y) of B pairs of LOCAL ids over the folded weights (what the reference's predict returns in eval
    mode); logits=True: (y, pred).  An id out of range scores y = 0 and raises IndexError at the next
    check_pending_errors()."""
    check_pending_errors()
    uids, iids = uids.to(torch.int64).contiguous().view(-1), iids.to(torch.int64).contiguous().view(-1)
    if uids.shape != iids.shape:
        raise ValueError('uids and iids must have the same length')
    y, pred, _, _ = _nfm_score(fold, _lib.NFM_PAIRS, uids, iids, uids.numel(), 1, 0, logits, True, False)
    return (y, pred) if logits else pred


def nfm_rank_eval(fold, uids, cand):
    """The contract of dot_rank_eval on the NFM scorer: cand [U', C] of LOCAL item ids, column 0 the held-out positive.
    Returns (logits [U', C], pred [U', C], rank [U'] int32, auc [U']): rank counts the negatives whose logit is strictly
    higher, auc is the share strictly lower; both read the logits, which order as pred does until the sigmoid saturates."""
    check_pending_errors()
    uids, cand = uids.to(torch.int64).contiguous(), cand.to(torch.int64).contiguous()
    if cand.dim() != 2 or uids.dim() != 1 or cand.shape[0] != uids.shape[0] or cand.shape[1] < 1:
        raise ValueError('cand must be [U, C >= 1] with one row per user of uids')
    return _nfm_score(fold, _lib.NFM_ROWS, uids, cand, uids.numel(), cand.shape[1], 0, True, True, True)


def nfm_score_block(fold, uids, item_lo, n_items):
    """logits [U', n_items] of every user of uids against the LOCAL items item_lo .. item_lo + n_items - 1."""
    check_pending_errors()
    uids = uids.to(torch.int64).contiguous()
    if not (0 <= int(item_lo) and int(n_items) >= 1 and int(item_lo) + int(n_items) <= fold.num_items):
        raise ValueError('the item range must lie inside the %d items' % fold.num_items)
    return _nfm_score(fold, _lib.NFM_RANGE, uids, None, uids.numel(), int(n_items), int(item_lo), True, False, False)[0]


# ---- the full-catalogue scan over the NFM fold (csrc/nfm_scan.hip, include/peahip_fm_eval.h)
def nfm_scan_supported(emb_dim, hidden_size, k=0):
    """Whether the fused catalogue scan takes these widths and k (pea_nfm_scan_supported; k = 0 asks for the rank forms,
    else k in 1..128).  Needs no device."""
    return bool(_lib.load().pea_nfm_scan_supported(int(emb_dim), int(hidden_size), int(k)))


def nfm_scan_splits(n_users, n_items, k=0):
    """The item ranges a fused call over n_users users and n_items items uses (pea_nfm_scan_splits)."""
    return int(_lib.load().pea_nfm_scan_splits(int(n_users), int(n_items), int(k)))


def _nfm_scan_args(fold, what, uids, k, item_lo, n_items, exclude):
    """What the three fused calls share: (lib, the 11 fold arguments, uids, item_lo, n_items, exclusion rowptr, items)"""
    lib = _lib.require_device()
    e, h = fold.emb.shape[1], fold.w.shape[0]
    if not lib.pea_nfm_scan_supported(e, h, int(k)):
        raise ValueError('%s: widths (%d, %d) with k = %d not supported (engine.nfm_scan_supported)' % (what, e, h, int(k)))
    uids = uids.to(torch.int64).contiguous()
    if uids.dim() != 1:
        raise ValueError('uids must be 1-d')
    item_lo, n_items = int(item_lo), int(n_items)
    if not (0 <= item_lo and n_items >= 0 and item_lo + n_items <= fold.num_items):
        raise ValueError('the item range must lie inside the %d items' % fold.num_items)
    rowptr, items = _exclusion_csr(exclude, uids.numel(), fold.device, 'fold')
    head = (e, h, fold.num_users, fold.num_items, _lib.ptr(fold.emb), fold.emb.stride(0), _lib.ptr(fold.lin), _lib.ptr(fold.w),
            _lib.ptr(fold.b), _lib.ptr(fold.w2), _lib.ptr(fold.bias))
    return lib, head, uids, item_lo, n_items, rowptr, items


def _nfm_scan_ws(lib, fold, n_users, q, items, n_items, k):
    """(workspace, its size, the zeroed error flag) of a fused call"""
    n_excl = int(items.numel()) if items is not None else 0
    ws_bytes = int(lib.pea_nfm_scan_workspace_bytes(n_users, q, n_excl, n_items, int(k), fold.emb.shape[1], fold.w.shape[0]))
    return (torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=fold.device), ws_bytes,
            torch.zeros(1, dtype=torch.int32, device=fold.device))


def nfm_recommend_topk(fold, uids, k, item_lo, n_items, item_node0=0, exclude=None):
    """The k best of the LOCAL items item_lo .. item_lo + n_items - 1 for every LOCAL user of uids over the folded weights, in
    one pass over the catalogue (include/peahip_fm_eval.h, pea_nfm_recommend_topk): (items int64 [U', k] as NODE ids =
    item_node0 + local, logits [U', k]) ordered by (logit descending, node id ascending) with a (-1, -inf) tail.  exclude =
    (rowptr [U' + 1], items) names NODE ids to leave out, every row strictly ascending.  The logits are nfm_score_block's
    bits.  A user id out of range gets an empty list and raises IndexError at the next check_pending_errors()."""
    check_pending_errors()
    lib, head, uids, item_lo, n_items, rowptr, items = _nfm_scan_args(fold, 'nfm_recommend_topk', uids, k, item_lo, n_items, exclude)
    u, k, dev = uids.numel(), int(k), fold.device
    out_items = torch.empty((u, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((u, k), dtype=torch.float32, device=dev)
    if u == 0:
        return out_items, out_scores
    ws, ws_bytes, flag = _nfm_scan_ws(lib, fold, u, 0, items, n_items, k)
    _lib.check(lib.pea_nfm_recommend_topk(*head, _lib.ptr(uids), u, k, item_lo, n_items, int(item_node0), _lib.ptr(rowptr),
                                          _lib.ptr(items), _lib.ptr(out_items), _lib.ptr(out_scores), _lib.ptr(flag), _lib.ptr(ws),
                                          ws_bytes, _lib.current_stream()))
    _defer_error(flag, NFM_ID_MESSAGE)
    return out_items, out_scores


def nfm_rank_full(fold, uids, pos_items, item_lo, n_items, item_node0=0, exclude=None):
    """The all-item rank of one held-out positive (a NODE id) per LOCAL user over the folded weights, in one pass over the
    catalogue (pea_nfm_rank_full): (rank int32 [U'] = the catalogue items, neither excluded nor the positive, whose logit is
    strictly higher, auc [U'] = float32(those strictly lower) / float32(their number), pos_score [U'])."""
    check_pending_errors()
    lib, head, uids, item_lo, n_items, rowptr, items = _nfm_scan_args(fold, 'nfm_rank_full', uids, 0, item_lo, n_items, exclude)
    pos_items = pos_items.to(torch.int64).contiguous()
    if pos_items.shape != uids.shape:
        raise ValueError('one positive per requested user')
    u = uids.numel()
    rank, auc, pos_score = _rank_outputs(u, fold.device)
    if u == 0:
        return rank, auc, pos_score
    ws, ws_bytes, flag = _nfm_scan_ws(lib, fold, u, u, items, n_items, 0)
    _lib.check(lib.pea_nfm_rank_full(*head, _lib.ptr(uids), u, _lib.ptr(pos_items), item_lo, n_items, int(item_node0),
                                     _lib.ptr(rowptr), _lib.ptr(items), _lib.ptr(rank), _lib.ptr(auc), _lib.ptr(pos_score),
                                     _lib.ptr(flag), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    _defer_error(flag, NFM_ID_MESSAGE)
    return rank, auc, pos_score


def nfm_rank_full_multi(fold, uids, pos_rowptr, pos_items, item_lo, n_items, item_node0=0, exclude=None):
    """nfm_rank_full for users with any number of held-out positives, in one catalogue scan (pea_nfm_rank_full_multi): the
    positives are a CSR (pos_rowptr int64 [U' + 1], pos_items int64 [Q] of NODE ids) on the fold's device, every row strictly
    ascending.  Returns, in the flat order of pos_items, (above int32 [Q], below int32 [Q], pos_score [Q]) and n_neg int32
    [U']: the contract of rank_full_multi."""
    check_pending_errors()
    lib, head, uids, item_lo, n_items, rowptr, items = _nfm_scan_args(fold, 'nfm_rank_full_multi', uids, 0, item_lo, n_items, exclude)
    u, dev = uids.numel(), fold.device
    pos_rowptr, pos_items = _positives_csr(pos_rowptr, pos_items, u, dev, 'fold')
    q = pos_items.numel()
    above, below, pos_score, n_neg = _multi_outputs(u, q, dev)
    if u == 0:
        return above, below, pos_score, n_neg
    ws, ws_bytes, flag = _nfm_scan_ws(lib, fold, u, q, items, n_items, 0)
    at = _ptr_or_spare(q, dev)
    _lib.check(lib.pea_nfm_rank_full_multi(*head, _lib.ptr(uids), u, _lib.ptr(pos_rowptr), at(pos_items), q, item_lo, n_items,
                                           int(item_node0), _lib.ptr(rowptr), _lib.ptr(items), at(above), at(below), at(pos_score),
                                           _lib.ptr(n_neg), _lib.ptr(flag), _lib.ptr(ws), ws_bytes, _lib.current_stream()))
    _defer_error(flag, NFM_ID_MESSAGE)
    return above, below, pos_score, n_neg
