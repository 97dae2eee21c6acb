"""The evaluation protocol in plain torch, written once: the candidate rank, the leave-one-out labels and losses, the
exclusion mask, and the three all-item compositions (rank_full, recommend, rank_full_multi) behind every model's ranking hooks.

A model hands the compositions two callbacks and they do the rest on whatever device the callbacks answer on:
    block(r0, r1)      -> scores [r1 - r0, hi - lo] of the requested users r0 .. r1 against the catalogue item_range = (lo, hi)
    pairs(rows, items) -> scores [len(rows)] of (requested-user row, item NODE id) pairs: the positives
The contracts are those documented on engine.rank_full, engine.recommend_topk and engine.rank_full_multi.  The compositions are
what a model falls back to where no fused kernel answers, and the yardstick every fused route is tested and measured against.
Imports torch alone: no engine, no library, no model."""
import torch
import torch.nn.functional as F


def candidate_ranks(scores):
    """scores [U, C], column 0 the held-out positive: (rank int32 [U] = negatives scoring strictly higher, auc float32 [U] =
    share of the negatives scoring strictly lower).  A tie with the positive counts on neither side."""
    pos, neg = scores[:, :1], scores[:, 1:]
    rank = (neg > pos).sum(dim=1).to(torch.int32)
    auc = (neg < pos).sum(dim=1).to(torch.float32) / max(neg.shape[1], 1)
    return rank, auc


def _labels(pred, dim):
    """the leave-one-out labels of pred: 1 for the first entry along dim (the positive), 0 for the rest"""
    label = torch.zeros_like(pred)
    label.select(dim, 0).fill_(1.0)
    return label


def leave_one_out_loss(pred, kind):
    """The reference's evaluation loss of rows (u, pos, neg...) from their predictions [U, C], column 0 the positive: labels
    [1, 0, ...] under MSELoss (kind 'mse') or BCEWithLogitsLoss (kind 'bce'); one value per row."""
    label = _labels(pred, 1)
    if kind == 'mse':
        return ((pred - label) ** 2).mean(dim=1)
    if kind == 'bce':
        return F.binary_cross_entropy_with_logits(pred, label, reduction='none').mean(dim=1)
    raise ValueError("kind is 'mse' or 'bce', not %r" % (kind,))


def eval_pairs(predict, batch):
    """(pred, label) of the eval branch of the reference's loss() over rows (u, pos, neg..) of ONE user (models/base.py:117-122):
    the first row's positive prediction followed by every row's negative one, labels [1, 0, ...] in float32."""
    pos_pred = predict(batch[:, 0], batch[:, 1])[:1]
    neg_pred = predict(batch[:, 0], batch[:, 2])
    pred = torch.cat([pos_pred, neg_pred])
    return pred, _labels(pred, 0).float()


def _rows_of(rowptr, r0, r1):
    """(b, e, rows): the entries b .. e of a CSR that belong to its rows r0 .. r1, and the row of each counted from r0"""
    counts = rowptr[r0 + 1:r1 + 1] - rowptr[r0:r1]
    return int(rowptr[r0]), int(rowptr[r1]), torch.repeat_interleave(torch.arange(r1 - r0, device=rowptr.device), counts)


def exclusion_mask(csr, n_users, lo, hi, r0, r1, device):
    """bool [r1 - r0, hi - lo]: the items of the node range [lo, hi) that csr = (rowptr [n_users + 1], items) names for users
    r0 .. r1; entries outside the range are ignored, None names nothing.  Reads rows r0 .. r1 of the CSR alone, so the chunks
    of a composition work out the owner of every entry once between them."""
    mask = torch.zeros((r1 - r0, hi - lo), dtype=torch.bool, device=device)
    if csr is not None:
        rowptr, items = (t.to(device) for t in csr)
        if rowptr.numel() != n_users + 1:
            raise ValueError('rowptr must have one entry per requested user and one more')
        b, e, rows = _rows_of(rowptr, r0, r1)
        items = items[b:e]
        inside = (items >= lo) & (items < hi)
        mask[rows[inside], items[inside] - lo] = True
    return mask


def _chunks(n, size):
    return ((r0, min(r0 + size, n)) for r0 in range(0, n, size))


def _cat(parts, dtype, device, width=None):
    """torch.cat(parts), or the empty tensor of dtype ([0] or [0, width]) where nobody asked"""
    if parts:
        return torch.cat(parts)
    return torch.zeros(0 if width is None else (0, width), dtype=dtype, device=device)


def rank_full(block, pairs, pos_items, item_range, exclude=None, user_chunk=256):
    """engine.rank_full's contract: per requested user (one per entry of pos_items, NODE ids) the rank of the held-out positive
    = the items of item_range, neither excluded nor the positive itself, scoring strictly higher; auc = float32(those strictly
    lower) / float32(their number, at least 1); and the positive's score.  (rank int32 [U], auc float32 [U], pos_score [U]):
    rank_full_multi with one positive per user."""
    rowptr = torch.arange(pos_items.numel() + 1, device=pos_items.device)
    above, below, pos_score, n_neg = rank_full_multi(block, pairs, rowptr, pos_items, item_range, exclude, user_chunk, user_chunk)
    return above, below.to(torch.float32) / n_neg.clamp(min=1), pos_score


def recommend(block, n_users, k, item_range, exclude=None, user_chunk=256, device=None):
    """engine.recommend_topk's contract: the k best items of item_range for each of the n_users requested users, ordered by
    (score descending, node id ascending: a stable sort), exclude = (rowptr, items) left out.  (items int64 [U, k], scores
    [U, k]) with a (-1, -inf) tail where fewer than k items are eligible, k larger than the catalogue included.  There are no
    positives, so no pair callback."""
    lo, hi, k = int(item_range[0]), int(item_range[1]), int(k)
    items = torch.arange(lo, hi, device=device)
    out_i, out_s = [], []
    for r0, r1 in _chunks(n_users, user_chunk):
        scores = block(r0, r1).clone()
        scores[exclusion_mask(exclude, n_users, lo, hi, r0, r1, device)] = float('-inf')
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
        top_s = torch.gather(scores, 1, order)
        top_i = torch.where(torch.isinf(top_s) & (top_s < 0), torch.full_like(order, -1), items[order])
        if top_s.shape[1] < k:
            pad = k - top_s.shape[1]
            top_s = F.pad(top_s, (0, pad), value=float('-inf'))
            top_i = F.pad(top_i, (0, pad), value=-1)
        out_i.append(top_i)
        out_s.append(top_s)
    return _cat(out_i, torch.int64, device, k), _cat(out_s, torch.float32, device, k)


def rank_full_multi(block, pairs, pos_rowptr, pos_items, item_range, exclude=None, user_chunk=256, pos_chunk=1024):
    """engine.rank_full_multi's contract: the positives are a CSR (pos_rowptr [U + 1], pos_items [Q] of NODE ids, every row
    strictly ascending); a user's negatives are the items of item_range in neither its exclusion row nor its positive row.
    Returns, in the flat order of pos_items, (above int32 [Q] = negatives scoring strictly higher, below int32 [Q] = strictly
    lower, pos_score [Q]) and n_neg int32 [U].  user_chunk users per block, pos_chunk positives compared at once."""
    lo, hi = int(item_range[0]), int(item_range[1])
    dev, n_users = pos_items.device, pos_rowptr.numel() - 1
    above, below, poss, n_neg = [], [], [], []
    for r0, r1 in _chunks(n_users, user_chunk):
        scores = block(r0, r1)
        negative = ~(exclusion_mask(exclude, n_users, lo, hi, r0, r1, dev) |
                     exclusion_mask((pos_rowptr, pos_items), n_users, lo, hi, r0, r1, dev))
        n_neg.append(negative.sum(dim=1).to(torch.int32))
        b, e, rows = _rows_of(pos_rowptr, r0, r1)
        for p0, p1 in _chunks(e - b, pos_chunk):
            row = rows[p0:p1]
            pos = pairs(row + r0, pos_items[b + p0:b + p1]).view(-1, 1)
            above.append(((scores[row] > pos) & negative[row]).sum(dim=1).to(torch.int32))
            below.append(((scores[row] < pos) & negative[row]).sum(dim=1).to(torch.int32))
            poss.append(pos.view(-1))
    return (_cat(above, torch.int32, dev), _cat(below, torch.int32, dev), _cat(poss, torch.float32, dev),
            _cat(n_neg, torch.int32, dev))
