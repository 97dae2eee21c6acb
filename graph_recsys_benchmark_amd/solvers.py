"""Batched evaluation with the reference's definitions.

Mirror of BaseSolver.metrics (graph_recsys_benchmark/solvers.py:33-104): the reference walks the test users one by
one (candidate draw, pandas merge, 4 H2D copies, 3 MLP launches, a sort and 3 D2H copies per user).  Here the
candidate ids are drawn on the host with the very same np.random.choice call per user (bit-exact ids, same stream
position afterwards), then ALL users are scored by one launch of pea_rank_eval; HR@5..20 / NDCG@5..20 / AUC / eval
loss follow graph_recsys_benchmark/utils/rec_utils.py:7-30 (hit :7, ndcg :18, auc :28) and solvers.py:72,93-96.
"""
import numpy as np
import torch

from . import engine
from .models.base import GraphRecsysModel
from .utils.interactions import seen_items_csr
from .utils.sampling import generate_candidates

NUM_RECS_RANGE = 20   # utils/rec_utils.py:4


def metrics_from_ranks(rank):
    """rank [U]: number of negatives placed before the (single) positive.  Returns HR [U,16], NDCG [U,16] for
    k = 5..20 exactly as hit() / ndcg() compute them from a hit vector with one positive."""
    rank = np.asarray(rank).reshape(-1, 1)
    ks = np.arange(5, NUM_RECS_RANGE + 1).reshape(1, -1)
    inside = rank < ks
    hr = inside.astype(np.float64)
    ndcg = np.where(inside, 1.0 / np.log2(rank + 2.0), 0.0)
    return hr, ndcg


def metrics(model, dataset, num_neg_candidates=99):
    """Returns (HR[16], NDCG[16], AUC[1], eval_loss[1]) means over the test users, like BaseSolver.metrics.
    `model` must be in eval() mode (cached_repr refreshed; for KGAT / KGCN: model.cf_eval(att_map), as the reference's
    solver does).  A model whose scorer is 'dot' is ranked by engine.dot_rank_eval (GraphRecsysModel.scored)."""
    u_nids = list(dataset.test_pos_unid_inid_map.keys())
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
    dev = model.cached_repr.device
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=dev)
    if hasattr(model, 'rank_eval'):                   # a model that picks its own evaluator (models/walk.py: HIP or torch by width)
        scores, rank, auc, loss = model.rank_eval(u_t, torch.from_numpy(cand).to(dev))
    else:                                             # by its scorer; KGAT / KGCN: after model.cf_eval(att_map)
        scores, rank, auc, loss = GraphRecsysModel.scored(model, 'rank_eval', u_t, torch.from_numpy(cand).to(dev))
    hr, ndcg = metrics_from_ranks(rank.cpu().numpy())
    return hr.mean(axis=0), ndcg.mean(axis=0), np.array([auc.double().mean().item()]), np.array([loss.double().mean().item()])


def _draw_candidates(dataset, u_nids, num_neg_candidates):
    """One metrics() worth of draws: [U, 1 + num_neg_candidates], column 0 the held-out positive (same calls, same order,
    same leave-one-out checks as `metrics`)."""
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
    if hasattr(model, 'rank_full'):
        rank, auc, _ = model.rank_full(u_t, pos_t, item_range, exclude=exclude)
    else:
        rank, auc, _ = GraphRecsysModel.scored(model, 'rank_full', u_t, pos_t, item_range, exclude=exclude)
    return metrics_full_from_ranks(rank.cpu().numpy(), auc.double().cpu().numpy())


def metrics_full_from_dataset(model, dataset):
    """metrics_full with users and positives from dataset.test_pos_unid_inid_map (one positive per user, as `metrics`
    insists), the item block from dataset.type_accs / num_iids and the exclusion from dataset.edge_index_nps['user2item']."""
    u_nids = list(dataset.test_pos_unid_inid_map.keys())
    pos = []
    for u_nid in u_nids:
        p = dataset.test_pos_unid_inid_map[u_nid]
        if len(p) != 1:
            raise NotImplementedError('the batched evaluator expects the leave-one-out protocol (one positive per user, '
                                      'datasets/movielens.py:304-308)')
        pos.append(p[0])
    item_range = (dataset.type_accs['iid'], dataset.type_accs['iid'] + dataset.num_iids)
    dev = model.cached_repr.device
    u_t = torch.as_tensor(np.asarray(u_nids, dtype=np.int64), device=dev)
    exclude = seen_items_csr(dataset.edge_index_nps['user2item'], u_t, item_range)
    return metrics_full(model, u_nids, pos, item_range, exclude)
