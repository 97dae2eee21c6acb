"""CPU: host side of the one-pass metapath ablation sweep -- candidate draws, declared surface, argument errors, the
per-variant metric reduction (no compute calls here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from graph_recsys_benchmark_amd import solvers
from graph_recsys_benchmark_amd.utils import SyntheticHIN
from graph_recsys_benchmark_amd.utils.sampling import generate_candidates
from helpers import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pea_fuse_ablate', 'pea_model_forward_ablate', 'pea_rank_eval_multi')


@pytest.fixture(scope='module')
def small_ds():
    ds = SyntheticHIN('ml_small', scale=0.1, seed=7)
    ds.eval_split()
    return ds


def loops(ds, n, num_neg=99):
    """n successive per-user generate_candidates loops, as n metrics() calls make them"""
    out = []
    for _ in range(n):
        rows = []
        for u in ds.test_pos_unid_inid_map.keys():
            pos, neg = generate_candidates(ds, u, num_neg)
            rows.append(np.asarray(list(pos) + list(neg), dtype=np.int64))
        out.append(np.stack(rows))
    return out


def states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('num_neg', [99, 7])
def test_fresh_draws_are_successive_metrics_draws(small_ds, num_neg):
    V = 4
    np.random.seed(123)
    want = loops(small_ds, V, num_neg)
    want_state = np.random.get_state()
    np.random.seed(123)
    got = solvers.ablation_candidates(small_ds, V, num_neg, shared=False)
    assert got.dtype == np.int64 and got.shape == (V, len(small_ds.test_pos_unid_inid_map), 1 + num_neg)
    for v in range(V):
        np.testing.assert_array_equal(got[v], want[v])
    assert states_equal(np.random.get_state(), want_state)
    assert not np.array_equal(got[0], got[1])        # really fresh draws


def test_shared_draw_consumes_one_loop(small_ds):
    np.random.seed(5)
    want = loops(small_ds, 1)[0]
    want_state = np.random.get_state()
    np.random.seed(5)
    got = solvers.ablation_candidates(small_ds, 6, shared=True)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert states_equal(np.random.get_state(), want_state)


def test_leave_one_out_checks_are_those_of_metrics(small_ds):
    class TwoPositives:
        test_pos_unid_inid_map = {u: list(p) + list(p) for u, p in small_ds.test_pos_unid_inid_map.items()}
        neg_unid_inid_map = small_ds.neg_unid_inid_map

    with pytest.raises(NotImplementedError):
        solvers.ablation_candidates(TwoPositives(), 2)


def test_header_and_binding_declare_the_ablation_entry_points():
    text = open(os.path.join(ROOT, 'include', 'peahip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    syms = set(re.findall(r'\b(pea_[a-z_0-9]+)\s*\(', text))
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    for must in NEW:
        assert must in syms and must in _lib.SIGNATURES and hasattr(lib, must)
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    # argument lists as the header spells them
    assert _lib.SIGNATURES['pea_fuse_ablate'] == (i32, [i64, i32, i32, vp, i64, ctypes.POINTER(i32), vp, i32, vp, vp, vp])
    assert _lib.SIGNATURES['pea_model_forward_ablate'] == (i32, [vp, ctypes.POINTER(vp), vp, vp, vp, sz, vp, vp, vp])
    assert _lib.SIGNATURES['pea_rank_eval_multi'] == (i32, [i32, i64, i32, i32, i64, vp, vp, vp, i64] + [vp] * 9)
    for name, n_args in (('pea_fuse_ablate', 11), ('pea_model_forward_ablate', 9), ('pea_rank_eval_multi', 18)):
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, text).group(1)
        assert len(decl.split(',')) == n_args == len(_lib.SIGNATURES[name][1])


def cpu_model():
    rng = np.random.default_rng(0)
    edges = [[rng.integers(0, 12, size=(2, 30)) for _ in range(2)] for _ in range(3)]
    return build_model('gcn', 12, edges, [2, 2, 2], 8, 8, 4, device='cpu')


def test_state_errors_on_a_cpu_model(small_ds):
    import torch
    model = cpu_model()
    ids = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='eval_ablation'):
        model.explain(ids, ids)
    with pytest.raises(RuntimeError, match='eval_ablation'):
        solvers.metapath_ablation(model, small_ds)
    with pytest.raises(RuntimeError):                # no CPU fallback for the forward itself
        model.eval_ablation()
    assert model.ablation_repr is None and model.ablation_att is None
    # the tables belong to the mode they were computed in: train() / eval(...) drop them (eval() goes through train(False))
    model.ablation_repr = model.ablation_att = torch.zeros(1)
    model.train()
    assert model.ablation_repr is None and model.ablation_att is None
    model.ablation_repr = torch.zeros(4, 12, 4)
    model.train(False)
    assert model.ablation_repr is None


def test_sharded_model_is_refused(small_ds):
    import torch
    model = cpu_model().shard(1, 2)
    ids = torch.zeros(2, dtype=torch.int64)
    for call in (model.eval_ablation, lambda: model.explain(ids, ids), lambda: solvers.metapath_ablation(model, small_ds)):
        with pytest.raises(NotImplementedError):
            call()


def test_reduction_is_per_variant_metrics_from_ranks():
    rng = np.random.default_rng(1)
    V, U = 5, 300
    rank = rng.integers(0, 40, size=(V, U)).astype(np.int32)
    auc = rng.random((V, U)).astype(np.float32)
    loss = (rng.random((V, U)) * 80).astype(np.float32)
    hr, ndcg, a, l = solvers.ablation_metrics_from_ranks(rank, auc, loss)
    assert hr.shape == (V, 16) and ndcg.shape == (V, 16) and a.shape == (V,) and l.shape == (V,)
    for v in range(V):
        want_hr, want_ndcg = solvers.metrics_from_ranks(rank[v])
        np.testing.assert_array_equal(hr[v], want_hr.mean(axis=0))
        np.testing.assert_array_equal(ndcg[v], want_ndcg.mean(axis=0))
        assert a[v] == auc[v].astype(np.float64).mean() and l[v] == loss[v].astype(np.float64).mean()
