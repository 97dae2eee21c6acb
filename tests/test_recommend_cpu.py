"""CPU: the index bookkeeping and the declared surface of the full-catalogue entry points (no compute calls here)."""
import os
import re

import numpy as np
import torch

from graph_recsys_benchmark_amd import solvers
from graph_recsys_benchmark_amd.utils import SyntheticHIN, seen_items_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def csr_numpy(edges, unids, lo, hi):
    """plain restatement: per requested user the sorted distinct items of [lo, hi) it has an edge to"""
    rowptr, items = [0], []
    for u in unids:
        mine = sorted({int(i) for uu, i in zip(edges[0], edges[1]) if int(uu) == int(u) and lo <= int(i) < hi})
        items.extend(mine)
        rowptr.append(len(items))
    return np.asarray(rowptr, np.int64), np.asarray(items, np.int64)


def random_edges(seed, n_users, lo, hi, e):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, n_users, size=e)
    items = rng.integers(lo - 5, hi + 5, size=e)          # some outside the catalogue
    edges = np.stack([users, items])
    return np.concatenate([edges, edges[:, : e // 4]], axis=1)   # duplicates


def test_seen_items_csr_matches_numpy():
    lo, hi = 40, 100
    edges = random_edges(3, 30, lo, hi, 400)
    edges = edges[:, edges[0] != 7]                        # user 7 has no interactions at all
    unids = [12, 3, 7, 29, 3, 0, 12]                       # out of order, repeated, one without edges; most users not asked
    want_ptr, want_items = csr_numpy(edges, unids, lo, hi)
    for form in (edges, edges.astype(np.float64), torch.from_numpy(edges)):
        ptr, items = seen_items_csr(form, torch.tensor(unids), (lo, hi))
        assert ptr.dtype == torch.int64 and items.dtype == torch.int64
        np.testing.assert_array_equal(ptr.numpy(), want_ptr)
        np.testing.assert_array_equal(items.numpy(), want_items)
    for q in range(len(unids)):
        row = want_items[want_ptr[q]:want_ptr[q + 1]]
        assert (np.diff(row) > 0).all() and ((row >= lo) & (row < hi)).all()
    assert want_ptr[3] == want_ptr[2]                      # user 7: empty row
    np.testing.assert_array_equal(want_items[want_ptr[1]:want_ptr[2]], want_items[want_ptr[4]:want_ptr[5]])


def test_seen_items_csr_empty_cases():
    ptr, items = seen_items_csr(np.zeros((2, 0)), torch.tensor([1, 2]), (0, 10))
    assert ptr.tolist() == [0, 0, 0] and items.numel() == 0
    ptr, items = seen_items_csr(np.array([[1, 1], [3, 4]]), torch.zeros(0, dtype=torch.int64), (0, 10))
    assert ptr.tolist() == [0] and items.numel() == 0


def test_seen_items_csr_on_the_synthetic_preset():
    d = SyntheticHIN('ml_small')
    i0 = d.type_accs['iid']
    u2i = d.edge_index_nps['user2item']
    unids = np.array([5, 600, 0, 5])
    ptr, items = seen_items_csr(u2i, torch.from_numpy(unids), (i0, i0 + d.num_iids))
    e = u2i.astype(np.int64)
    for q, u in enumerate(unids):
        np.testing.assert_array_equal(items[ptr[q]:ptr[q + 1]].numpy(), np.unique(e[1][e[0] == u]))


def test_eval_holdout_draws_one_unseen_item_per_user():
    d = SyntheticHIN('ml_small')
    u, p = d.eval_holdout()
    i0 = d.type_accs['iid']
    assert u.tolist() == list(range(d.type_accs['uid'], d.type_accs['uid'] + d.num_uids))
    assert p.dtype == np.int64 and p.min() >= i0 and p.max() < i0 + d.num_iids
    e = d.edge_index_nps['user2item'].astype(np.int64)
    seen = set(zip(e[0].tolist(), e[1].tolist()))
    assert not any((a, b) in seen for a, b in zip(u.tolist(), p.tolist()))
    u2, p2 = d.eval_holdout()
    np.testing.assert_array_equal(p, p2)                   # seeded
    u3, p3 = d.eval_holdout(num_users=10, seed=5)
    assert len(u3) == 10 and not any((a, b) in seen for a, b in zip(u3.tolist(), p3.tolist()))


def test_eval_holdout_reaches_every_unseen_item_and_no_other():
    """a tiny catalogue, many seeds: the set of items ever drawn for a user is exactly its unseen set"""
    d = SyntheticHIN('ml_small', scale=0.02)
    e = d.edge_index_nps['user2item'].astype(np.int64)
    i0 = d.type_accs['iid']
    drawn = [set() for _ in range(d.num_uids)]
    for seed in range(400):
        _, p = d.eval_holdout(seed=seed)
        for k, item in enumerate(p.tolist()):
            drawn[k].add(item)
    for k in range(d.num_uids):
        unseen = set(range(i0, i0 + d.num_iids)) - set(e[1][e[0] == d.type_accs['uid'] + k].tolist())
        assert drawn[k] <= unseen
        assert len(unseen) > 12 or drawn[k] == unseen      # 400 draws cover a set of <= 12 with overwhelming probability


def test_header_declares_the_full_catalogue_entry_points():
    text = open(os.path.join(ROOT, 'include', 'peahip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    syms = set(re.findall(r'\b(pea_[a-z_0-9]+)\s*\(', text))
    for must in ('pea_recommend_topk', 'pea_rank_full', 'pea_topk_workspace_bytes'):
        assert must in syms
    from graph_recsys_benchmark_amd import _lib
    for must in ('pea_recommend_topk', 'pea_rank_full', 'pea_topk_workspace_bytes'):
        assert must in _lib.SIGNATURES


def test_metrics_full_aggregation_is_metrics_from_ranks():
    rng = np.random.default_rng(0)
    rank = rng.integers(0, 40, size=500)
    auc = rng.random(500).astype(np.float32)
    hr, ndcg, a = solvers.metrics_full_from_ranks(rank, auc)
    want_hr, want_ndcg = solvers.metrics_from_ranks(rank)
    np.testing.assert_array_equal(hr, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg, want_ndcg.mean(axis=0))
    assert hr.shape == (16,) and ndcg.shape == (16,) and a.shape == (1,)
    assert a[0] == auc.astype(np.float64).mean()
    assert hr[0] == (rank < 5).mean() and hr[15] == (rank < 20).mean()
