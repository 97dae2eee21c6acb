"""Batched evaluation with the reference's definitions.

Mirror of BaseSolver.metrics (graph_recsys_benchmark/solvers.py:33-104): the reference walks the test users one by
one (candidate draw, pandas merge, 4 H2D copies, 3 MLP launches, a sort and 3 D2H copies per user).  Here the
candidate ids are drawn on the host with the very same np.random.choice call per user (bit-exact ids, same stream
position afterwards), then ALL users are scored by one launch of pea_rank_eval; HR@5..20 / NDCG@5..20 / AUC / eval
loss follow graph_recsys_benchmark/utils/rec_utils.py:7-30 (hit :7, ndcg :18, auc :28) and solvers.py:72,93-96.

kg_epoch is the KG-phase training loop of the KGAT / KGCN / CFKG drivers over a table that already lives on the device; cf_epoch is
its CF twin (model.loss per step), the loop every model here trains with.
"""
import numpy as np
import torch

from . import engine
from .models.base import GraphRecsysModel
from .utils.interactions import positives_csr, seen_items_csr
from .utils.sampling import generate_candidates

NUM_RECS_RANGE = 20   # utils/rec_utils.py:4


def kg_epoch(model, optimizer, train_data, batch_size, max_steps=None):
    """The KG-phase loop of the reference's drivers (experiments/cfkg_solver_bpr.py:227 ff., kgat_solver_bpr.py:289-306) over a
    table that is already on the model's device (utils.device_kg_negative_sampling): batches are views of consecutive rows,
    the last short one included as DataLoader includes it; every step runs zero_grad, kg_loss, backward, step.  The
    per-batch losses stay in one device tensor and are read ONCE: the return value is their float64 mean, the reference's
    np.mean(kg_loss_per_batch), where its loop reads every step's loss with .item().  max_steps caps the number of steps.
    Pending id errors of the epoch's launches raise here (engine.check_pending_errors)."""
    return _epoch('kg_epoch', model.kg_loss, optimizer, train_data, batch_size, max_steps)


def cf_epoch(model, optimizer, train_data, batch_size, max_steps=None):
    """The CF twin of kg_epoch: the training loop of the reference's BaseSolver.run (solvers.py:211-218) over a table that is
    already on the model's device (utils.device_cf_negative_sampling; three columns, or nine for an entity-aware model).  Every
    step runs zero_grad, model.loss(batch), backward, step on a view of consecutive rows, the last short batch included;
    the losses stay on the device and are read ONCE, the return value is their float64 mean.  max_steps caps the number of
    steps.  Pending id errors of the epoch's launches raise here (engine.check_pending_errors)."""
    return _epoch('cf_epoch', model.loss, optimizer, train_data, batch_size, max_steps)


def _epoch(who, loss_of, optimizer, train_data, batch_size, max_steps):
    """the loop of kg_epoch and cf_epoch over loss_of(batch)"""
    n, batch_size = int(train_data.shape[0]), int(batch_size)
    if batch_size < 1:
        raise ValueError('%s: batch_size %d' % (who, batch_size))
    steps = (n + batch_size - 1) // batch_size
    if max_steps is not None:
        steps = min(steps, int(max_steps))
    if steps <= 0:
        return float('nan')
    losses = torch.zeros(steps, dtype=torch.float32, device=train_data.device)
    for k in range(steps):
        batch = train_data[k * batch_size:(k + 1) * batch_size]
        optimizer.zero_grad()
        loss = loss_of(batch)
        loss.backward()
        optimizer.step()
        losses[k] = loss.detach()
    mean = float(losses.double().mean().item())
    engine.check_pending_errors()
    return mean


def metrics_from_ranks(rank):
    """rank [U]: number of negatives placed before the (single) positive.  Returns HR [U,16], NDCG [U,16] for
    k = 5..20 exactly as hit() / ndcg() compute them from a hit vector with one positive."""
    rank = np.asarray(rank).reshape(-1, 1)
    ks = np.arange(5, NUM_RECS_RANGE + 1).reshape(1, -1)
    inside = rank < ks
    hr = inside.astype(np.float64)
    ndcg = np.where(inside, 1.0 / np.log2(rank + 2.0), 0.0)
    return hr, ndcg


def _hook(model, op):
    """The model's own method `op` where it has one, else engine.<op> of its scorer on cached_repr (GraphRecsysModel.scored,
    unbound: it serves whatever model object it is handed)."""
    own = getattr(model, op, None)
    return own if own is not None else (lambda *args, **kwargs: GraphRecsysModel.scored(model, op, *args, **kwargs))


def metrics(model, dataset, num_neg_candidates=99):
    """Returns (HR[16], NDCG[16], AUC[1], eval_loss[1]) means over the test users, like BaseSolver.metrics.
    `model` must be in eval() mode (cached_repr refreshed; for KGAT / KGCN: model.cf_eval(att_map), as the reference's
    solver does).  A model whose scorer is 'dot' is ranked by engine.dot_rank_eval (GraphRecsysModel.scored)."""
    u_nids = list(dataset.test_pos_unid_inid_map.keys())
    cand = _draw_candidates(dataset, u_nids, num_neg_candidates)
    dev = model.cached_repr.device
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=dev)
    # a model that picks its own evaluator (models/walk.py: HIP or torch by width), else by its scorer; KGAT / KGCN: after
    # model.cf_eval(att_map)
    scores, rank, auc, loss = _hook(model, 'rank_eval')(u_t, torch.from_numpy(cand).to(dev))
    hr, ndcg = metrics_from_ranks(rank.cpu().numpy())
    return hr.mean(axis=0), ndcg.mean(axis=0), np.array([auc.double().mean().item()]), np.array([loss.double().mean().item()])


def _draw_candidates(dataset, u_nids, num_neg_candidates):
    """One metrics() worth of draws: [U, 1 + num_neg_candidates], column 0 the held-out positive, the very np.random.choice
    call per user of the reference, with its leave-one-out checks."""
    cand = np.empty((len(u_nids), 1 + num_neg_candidates), dtype=np.int64)
    for idx, u_nid in enumerate(u_nids):
        pos_i_nids, neg_i_nids = generate_candidates(dataset, u_nid, num_neg_candidates)
        if len(pos_i_nids) == 0 or len(neg_i_nids) == 0:
            raise ValueError("No pos or neg samples found in evaluation!")
        if len(pos_i_nids) != 1:
            raise NotImplementedError('the batched evaluator expects the leave-one-out protocol (one positive per user, '
                                      'datasets/movielens.py:304-308)')
        cand[idx, 0] = pos_i_nids[0]
        cand[idx, 1:] = neg_i_nids
    return cand


def ablation_candidates(dataset, n_variants, num_neg_candidates=99, shared=False):
    """Candidate ids of a metapath sweep.  shared=False: [V, U, C], variant-major, exactly what n_variants successive
    metrics() calls would draw (the same generate_candidates calls in the same order: identical ids, and the legacy numpy
    stream ends in the same state) -- the reference's loop (solvers.py:224-241) draws afresh per metapath.  shared=True: ONE
    draw, [U, C]: every variant is ranked on identical candidates (a paired comparison; consumes one metrics() worth of
    the stream)."""
    u_nids = list(dataset.test_pos_unid_inid_map.keys())
    if shared:
        return _draw_candidates(dataset, u_nids, num_neg_candidates)
    return np.stack([_draw_candidates(dataset, u_nids, num_neg_candidates) for _ in range(int(n_variants))])


def ablation_metrics_from_ranks(rank, auc, loss):
    """Per-variant means from rank [V, U], auc [V, U], loss [V, U]: (HR [V, 16], NDCG [V, 16], AUC [V], eval_loss [V]), each
    row reduced exactly as `metrics` reduces its single table (metrics_from_ranks, float64 means)."""
    rank = np.asarray(rank)
    hr, ndcg = zip(*[[m.mean(axis=0) for m in metrics_from_ranks(r)] for r in rank])
    return (np.stack(hr), np.stack(ndcg), np.asarray(auc, dtype=np.float64).mean(axis=1),
            np.asarray(loss, dtype=np.float64).mean(axis=1))


def metapath_ablation(model, dataset, num_neg_candidates=99, shared_candidates=False, variants=None):
    """The reference's per-metapath table (solvers.py:224-241: model.eval(metapath_idx) + metrics() per metapath) from the
    tables of ONE forward: `model` must be in the eval_ablation() state.  variants: the tables to rank, default
    range(P + 1) (0 = unmasked, 1 + p = metapath p zeroed); a contiguous range is ranked in place (a slice of the tables).
    Row k of the result belongs to variants[k]: (HR [V, 16], NDCG [V, 16], AUC [V], eval_loss [V]) means over the test
    users.  shared_candidates=False draws afresh per variant, in order, as successive metrics() calls would; True ranks
    every variant on one draw.  One ranking launch for all variants (engine.rank_eval_multi)."""
    if getattr(model, '_shard', (0, 1))[1] > 1:
        raise NotImplementedError('the ablation sweep is single-GPU (this model is sharded)')
    tables = getattr(model, 'ablation_repr', None)
    if tables is None or model.training:
        raise RuntimeError('metapath_ablation() reads the ablation tables: call model.eval_ablation() first')
    variants = list(range(tables.shape[0])) if variants is None else [int(v) for v in variants]
    if not variants or min(variants) < 0 or max(variants) >= tables.shape[0]:
        raise ValueError('variants must name tables 0..%d' % (tables.shape[0] - 1))
    if variants == list(range(variants[0], variants[0] + len(variants))):
        picked = tables[variants[0]:variants[0] + len(variants)]
    else:
        picked = tables[torch.as_tensor(variants, device=tables.device)]
    cand = ablation_candidates(dataset, len(variants), num_neg_candidates, shared=shared_candidates)
    u_nids = np.asarray(list(dataset.test_pos_unid_inid_map.keys()), dtype=np.int64)
    dev = tables.device
    _, rank, auc, loss = engine.rank_eval_multi(picked, torch.as_tensor(u_nids, device=dev), torch.from_numpy(cand).to(dev),
                                                model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)
    return ablation_metrics_from_ranks(rank.cpu().numpy(), auc.double().cpu().numpy(), loss.double().cpu().numpy())


def metrics_full_from_ranks(rank, auc):
    """(HR[16], NDCG[16], AUC[1]) means over the users from per-user all-item ranks and aucs."""
    hr, ndcg = metrics_from_ranks(rank)
    return hr.mean(axis=0), ndcg.mean(axis=0), np.array([np.asarray(auc, dtype=np.float64).mean()])


def metrics_full(model, u_nids, pos_items, item_range, exclude=None):
    """Unsampled evaluation: every item of the catalogue item_range that is not in the user's exclusion row is a negative
    (the reference's neg_unid_inid_map[u] in full, where solvers.py:21-31 draws 99 of it).  Returns (HR[16], NDCG[16],
    AUC[1]) means through the same metrics_from_ranks as `metrics`; no eval loss at full catalogue.  `model` must be
    in eval() mode; exclude = (rowptr, items) on the model's device (utils.interactions.seen_items_csr)."""
    dev = model.cached_repr.device
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=dev)
    pos_t = torch.as_tensor(np.asarray(pos_items, dtype=np.int64), device=dev)
    rank, auc, _ = _hook(model, 'rank_full')(u_t, pos_t, item_range, exclude=exclude)
    return metrics_full_from_ranks(rank.cpu().numpy(), auc.double().cpu().numpy())


def _catalogue_of(model, dataset):
    """(u_nids, item_range, exclude) of a dataset's test users: the keys of test_pos_unid_inid_map, the item block from
    type_accs / num_iids and the exclusion CSR from edge_index_nps['user2item'], on the model's device"""
    u_nids = list(dataset.test_pos_unid_inid_map.keys())
    item_range = (dataset.type_accs['iid'], dataset.type_accs['iid'] + dataset.num_iids)
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=model.cached_repr.device)
    return u_nids, item_range, seen_items_csr(dataset.edge_index_nps['user2item'], u_t, item_range)


def metrics_full_from_dataset(model, dataset):
    """metrics_full with users and positives from dataset.test_pos_unid_inid_map (one positive per user, as `metrics`
    insists), the item block from dataset.type_accs / num_iids and the exclusion from dataset.edge_index_nps['user2item']."""
    u_nids, item_range, exclude = _catalogue_of(model, dataset)
    pos = []
    for u_nid in u_nids:
        p = dataset.test_pos_unid_inid_map[u_nid]
        if len(p) != 1:
            raise NotImplementedError('the batched evaluator expects the leave-one-out protocol (one positive per user, '
                                      'datasets/movielens.py:304-308)')
        pos.append(p[0])
    return metrics_full(model, u_nids, pos, item_range, exclude)


# ---- several held-out positives per user (engine.rank_full_multi; include/peahip_eval.h)
MULTI_METRICS = ('HR', 'NDCG_ref', 'Recall', 'Precision', 'NDCG', 'MRR', 'AP', 'AUC')


def multi_metrics_from_counts(above, pos_score, below, pos_rowptr, n_neg):
    """Per-user metrics of an all-item ranking with any number of positives, in float64 from the integer counts of
    engine.rank_full_multi: above / below [Q] (negatives scoring strictly higher / lower than flat positive j), pos_score [Q],
    pos_rowptr [U + 1], n_neg [U].  The 0-based place of positive j in the user's merged descending list is
        r_j = above_j + #{j' of the same user: s_j' > s_j, or s_j' == s_j and j' < j}
    (a positive goes ahead of an equal negative, as rank_one_user has it and as the stable sort of reference solvers.py:88 does
    with the positives first; ties among positives go by row order).  With h_k = #{r_j < k}, r_min = min r_j and P the user's
    positives, for k = 5 .. NUM_RECS_RANGE (columns) the dict holds
        'HR' [U, 16]         [r_min < k]                                    utils/rec_utils.py:7 hit()
        'NDCG_ref' [U, 16]   h_k / log2(r_min + 2) if r_min < k else 0      utils/rec_utils.py:18 ndcg(), exactly: the hits of
                             the first k places over the discount of the FIRST hit alone, not a normalised DCG
        'Recall' [U, 16]     h_k / P
        'Precision' [U, 16]  h_k / k
        'NDCG' [U, 16]       sum over r_j < k of 1 / log2(r_j + 2), over sum over i < min(P, k) of 1 / log2(i + 2)
        'MRR' [U]            1 / (r_min + 1)
        'AP' [U]             mean over the positives in rank order m = 1 .. P of m / (r_(m) + 1)
        'AUC' [U]            sum of below_j over P n_neg                    utils/rec_utils.py:28 auc()
    A user without a positive or without a negative has nan rows here; metrics_full_multi refuses such a user."""
    above = np.asarray(above, dtype=np.int64).reshape(-1)
    below = np.asarray(below, dtype=np.int64).reshape(-1)
    score = np.asarray(pos_score).reshape(-1)
    rowptr = np.asarray(pos_rowptr, dtype=np.int64).reshape(-1)
    n_neg = np.asarray(n_neg, dtype=np.int64).reshape(-1)
    u = rowptr.size - 1
    if above.size != below.size or above.size != score.size or n_neg.size != u or (u >= 0 and rowptr[-1] != above.size):
        raise ValueError('above, below, pos_score are [Q] with Q = pos_rowptr[U], n_neg is [U]')
    ks = np.arange(5, NUM_RECS_RANGE + 1)
    out = {name: np.full((u, ks.size) if name in ('HR', 'NDCG_ref', 'Recall', 'Precision', 'NDCG') else (u,), np.nan)
           for name in MULTI_METRICS}
    disc = 1.0 / np.log2(np.arange(NUM_RECS_RANGE, dtype=np.float64) + 2.0)        # of places 0 .. 19
    ideal = np.cumsum(disc)
    for q in range(u):
        b, e = int(rowptr[q]), int(rowptr[q + 1])
        p = e - b
        if p == 0:
            continue
        s = score[b:e]
        ahead = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (np.arange(p)[None, :] < np.arange(p)[:, None]))
        r = np.sort(above[b:e] + ahead.sum(axis=1))                # r_(1) <= r_(2) <= ...: distinct places
        r_min = int(r[0])
        h = (r[None, :] < ks[:, None]).sum(axis=1).astype(np.float64)
        out['HR'][q] = (r_min < ks).astype(np.float64)
        out['NDCG_ref'][q] = np.where(r_min < ks, h / np.log2(r_min + 2.0), 0.0)
        out['Recall'][q] = h / p
        out['Precision'][q] = h / ks
        gain = np.where(r < NUM_RECS_RANGE, disc[np.minimum(r, NUM_RECS_RANGE - 1)], 0.0)
        dcg = np.array([gain[r < k].sum() for k in ks])
        out['NDCG'][q] = dcg / ideal[np.minimum(p, ks) - 1]
        out['MRR'][q] = 1.0 / (r_min + 1.0)
        out['AP'][q] = np.mean(np.arange(1, p + 1, dtype=np.float64) / (r + 1.0))
        if n_neg[q] > 0:
            out['AUC'][q] = float(below[b:e].sum()) / (float(p) * float(n_neg[q]))
    return out


def _exclude_rows(exclude, u):
    """the exclusion CSR as U numpy rows (empty rows for None)"""
    if exclude is None:
        return [np.zeros(0, dtype=np.int64)] * u
    rowptr, items = (t.detach().cpu().numpy() for t in exclude)
    return [items[rowptr[q]:rowptr[q + 1]] for q in range(u)]


def rank_full_multi_flattened(rank_full, u_nids, pos_rowptr, pos_items, item_range, exclude=None, device=None):
    """engine.rank_full_multi's outputs from a SINGLE-positive rank_full(unids, pos_items, item_range, exclude=) -> (rank, auc,
    pos_score): one call over the Q (user, positive) pairs, the user repeated, each pair's exclusion row the sorted,
    de-duplicated union of the user's exclusion row and its positive row (rank_full skips the positive itself).  Then
    above = rank, pos_score as is, n_neg = the catalogue items outside that union, below = round(auc n_neg): auc is the
    float32 quotient below / n_neg, off by at most 2^-24 of itself, so the product is within one half of below for a catalogue
    of fewer than 2^23 items (a larger one is refused).  Pays the catalogue scan once per positive: the route of a model that
    has a rank_full of its own only, and the yardstick the native route is tested and measured against.  Returns numpy (above int64 [Q], below int64 [Q], pos_score float32 [Q], n_neg
    int64 [U])."""
    u_nids = np.asarray(u_nids, dtype=np.int64).reshape(-1)
    rowptr = np.asarray(pos_rowptr, dtype=np.int64).reshape(-1)
    items = np.asarray(pos_items, dtype=np.int64).reshape(-1)
    lo, hi = int(item_range[0]), int(item_range[1])
    if hi - lo >= 1 << 23:
        raise ValueError('the flattened route recovers `below` from a float32 auc: catalogues of fewer than 2^23 items only')
    excl = _exclude_rows(exclude, u_nids.size)
    unions, n_neg = [], np.zeros(u_nids.size, dtype=np.int64)
    for q in range(u_nids.size):
        un = np.union1d(excl[q], items[rowptr[q]:rowptr[q + 1]]).astype(np.int64)
        unions.append(un)
        n_neg[q] = (hi - lo) - int(((un >= lo) & (un < hi)).sum())
    counts = np.diff(rowptr)
    flat_q = np.repeat(np.arange(u_nids.size), counts)
    if items.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), n_neg
    f_rowptr = np.zeros(items.size + 1, dtype=np.int64)
    np.cumsum([unions[q].size for q in flat_q], out=f_rowptr[1:])
    f_items = np.concatenate([unions[q] for q in flat_q]) if f_rowptr[-1] else np.zeros(0, dtype=np.int64)
    to = (lambda a: torch.as_tensor(a, device=device)) if device is not None else torch.as_tensor
    rank, auc, pos_score = rank_full(to(u_nids[flat_q]), to(items), item_range, exclude=(to(f_rowptr), to(f_items)))
    above = rank.detach().cpu().numpy().astype(np.int64)
    below = np.rint(auc.detach().cpu().numpy().astype(np.float64) * n_neg[flat_q]).astype(np.int64)
    return above, below, pos_score.detach().cpu().numpy(), n_neg


def metrics_full_multi(model, u_nids, positives, item_range, exclude=None):
    """Unsampled evaluation with any number of held-out positives per user (the ratio-split protocol KGAT / NGCF / KGCN were
    published under): a user's negatives are the catalogue items in neither its exclusion row nor its positives.  positives:
    what utils.interactions.positives_csr takes (a sequence of U lists, or [2, E] test edges), or its (pos_rowptr, pos_items)
    result.  Returns the dict of multi_metrics_from_counts reduced to means over the users ([16] for k = 5 .. 20, or a
    scalar).  Raises ValueError('No pos or neg samples found in evaluation!') for a user with no positive or no negative, as
    reference solvers.py:60-61.  One catalogue scan through GraphRecsysModel.scored(model, 'rank_full_multi', ...); a model
    with a rank_full of its own and no rank_full_multi goes through rank_full_multi_flattened on it.  `model` must be in
    eval() mode; exclude = (rowptr, items) on the model's device."""
    dev = model.cached_repr.device
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=dev)
    if isinstance(positives, tuple) and len(positives) == 2 and all(torch.is_tensor(t) and t.dim() == 1 for t in positives):
        pos_rowptr, pos_items = (t.to(dev) for t in positives)
    else:
        pos_rowptr, pos_items = positives_csr(positives, u_t)
    rowptr_np = pos_rowptr.cpu().numpy()
    if u_t.numel() == 0 or np.any(np.diff(rowptr_np) == 0):
        raise ValueError("No pos or neg samples found in evaluation!")
    if hasattr(model, 'rank_full') and not hasattr(model, 'rank_full_multi'):
        above, below, pos_score, n_neg = rank_full_multi_flattened(model.rank_full, u_t.cpu().numpy(), rowptr_np,
                                                                   pos_items.cpu().numpy(), item_range, exclude, device=dev)
    else:
        above, below, pos_score, n_neg = _hook(model, 'rank_full_multi')(u_t, pos_rowptr, pos_items, item_range, exclude=exclude)
    above, below, pos_score, n_neg = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (above, below, pos_score, n_neg))
    if np.any(np.asarray(n_neg) <= 0):
        raise ValueError("No pos or neg samples found in evaluation!")
    per_user = multi_metrics_from_counts(above, pos_score, below, rowptr_np, n_neg)
    return {name: v.mean(axis=0) for name, v in per_user.items()}


def metrics_full_multi_from_dataset(model, dataset):
    """metrics_full_multi with users and positives from dataset.test_pos_unid_inid_map (lists of any length), the item block from
    dataset.type_accs / num_iids and the exclusion from dataset.edge_index_nps['user2item']."""
    u_nids, item_range, exclude = _catalogue_of(model, dataset)
    positives = [dataset.test_pos_unid_inid_map[u_nid] for u_nid in u_nids]
    return metrics_full_multi(model, u_nids, positives, item_range, exclude)
