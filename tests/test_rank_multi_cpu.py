"""CPU: what the multi-positive all-item evaluation decides without a device -- the third header (include/peahip_eval.h) against
_lib.EVAL_SIGNATURES and the library's exports, the workspace queries, every argument refusal (returned before anything is
launched, so no GPU is needed to see it), utils.interactions.positives_csr, and the metric layer of solvers.py: against the
reference-recorded fixture tests/golden/rec_utils_multi.json (tests/make_multipos_golden.py), against a brute-force sort, its
ValueError cases and the flattened route with a numpy scorer standing in for the model."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from graph_recsys_benchmark_amd import _lib, engine, solvers
from graph_recsys_benchmark_amd.utils import positives_csr
from graph_recsys_benchmark_amd.utils.interactions import positives_csr as positives_csr_home

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_RANGE, ERR_NOMEM = 0, -1, -2, -4
NAMES = ['pea_dot_rank_full_multi', 'pea_dot_rank_multi_workspace_bytes', 'pea_rank_full_multi', 'pea_rank_multi_workspace_bytes']
KS = np.arange(5, 21)

_keep = []


def fake(nbytes=4096):
    """A 16-byte aligned host address that stands in for a device pointer: the calls below fail validation before they would
    read through it."""
    buf = C.create_string_buffer(nbytes + 32)
    _keep.append(buf)
    return C.c_void_p((C.addressof(buf) + 15) & ~15)


# ---------------------------------------------------------------- the third header (the parsing helpers of test_cabi.py, restated)
C_WIDTH = {'void': 'void', 'int': 'int', 'int64_t': 'int64', 'size_t': 'uint64', 'uint64_t': 'uint64', 'uint32_t': 'uint32',
           'float': 'float', 'double': 'double'}


def c_width(decl, is_param):
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w not in ('const', 'struct')]
    if is_param and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    return C_WIDTH.get(' '.join(words), 'unknown C type: %s' % decl.strip())


def ctypes_width(t):
    if t is None:
        return 'void'
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return 'pointer'
    table = {C.c_int: 'int', C.c_int64: 'int64', C.c_size_t: 'uint64', C.c_uint64: 'uint64', C.c_uint32: 'uint32',
             C.c_float: 'float', C.c_double: 'double'}
    return table.get(t, 'unknown ctypes type: %r' % t)


def prototypes(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    protos = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w \*]*?)\b(pea_[a-z_0-9]+)\s*\(([^)]*)\)\s*;', text):
        params = [p for p in params.split(',') if p.strip() and p.strip() != 'void']
        assert name not in protos, 'declared twice: %s' % name
        protos[name] = (c_width(ret, False), [c_width(p, True) for p in params])
    return protos


def test_third_header_matches_its_ctypes_table():
    protos = prototypes('peahip_eval.h')
    assert sorted(protos) == sorted(_lib.EVAL_SIGNATURES) == NAMES
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.EVAL_SIGNATURES[name]
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    others = set(prototypes('peahip.h')) | set(prototypes('peahip_kge.h'))
    assert not others & set(protos)
    assert not (set(_lib.SIGNATURES) | set(_lib.KGE_SIGNATURES)) & set(_lib.EVAL_SIGNATURES)
    assert len(_lib.SIGNATURES) == 112                   # the first table is where test_cabi.py pins it


def test_engine_reexports_and_scoring_stands_alone():
    assert engine.rank_full_multi.__module__.endswith('.scoring') and engine.dot_rank_full_multi.__module__.endswith('.scoring')
    assert positives_csr is positives_csr_home


# ---------------------------------------------------------------- workspace queries
def test_workspace_queries():
    lib = _lib.load()
    mlp, dot = lib.pea_rank_multi_workspace_bytes, lib.pea_dot_rank_multi_workspace_bytes
    for r in (4, 16, 20, 32, 64):
        assert mlp(10, 50, 100, r) > 0
    for r in (0, -4, 6, 68, 128):
        assert mlp(10, 50, 100, r) == 0
    for d in (4, 20, 64, 128, 256):
        assert dot(10, 50, 100, d) > 0
    for d in (0, 2, 6, 260, -4):
        assert dot(10, 50, 100, d) == 0
    for q in (mlp, dot):
        assert q(-1, 5, 10, 16) == 0 and q(1, -5, 10, 16) == 0 and q(1, 5, -10, 16) == 0 and q(1, 5, 2 ** 31 - 1, 16) == 0
        assert q(0, 0, 0, 16) > 0                                       # nothing to do is not refused
        assert q(1000, 9000, 5000, 16) == q(1000, 9000, 5000, 16)       # a function of its arguments alone
        sizes = [q(1000, n, 5000, 16) for n in (0, 1, 7, 8, 9, 4000, 40000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]          # the rows are U + Q / 8: more positives never need less
    # the rows of the dot form grow with Q / 8 only: 8 more positives are one more row of 2 x 8 counters per item range
    assert dot(64, 16, 100, 16) >= dot(64, 8, 100, 16)


# ---------------------------------------------------------------- refusals before any launch
def call(form, **over):
    a = dict(U=10, W=16, num_nodes=200, repr=fake(), unids=fake(), pos_rowptr=fake(), pos_items=fake(), Q=30, item_lo=50, n_items=100,
             excl_rowptr=fake(), excl_items=fake(), fc1_w=fake(), fc1_b=fake(), fc2_w=fake(), fc2_b=fake(), above=fake(),
             below=fake(), pos_score=fake(), n_neg=fake(), ws=fake(), ws_bytes=1 << 40, stream=None)
    a.update(over)
    lib = _lib.load()
    head = [a['U'], a['W'], a['num_nodes'], a['repr'], a['unids'], a['pos_rowptr'], a['pos_items'], a['Q'], a['item_lo'],
            a['n_items'], a['excl_rowptr'], a['excl_items']]
    tail = [a['above'], a['below'], a['pos_score'], a['n_neg'], a['ws'], a['ws_bytes'], a['stream']]
    if form == 'mlp':
        return lib.pea_rank_full_multi(*head, a['fc1_w'], a['fc1_b'], a['fc2_w'], a['fc2_b'], *tail)
    return lib.pea_dot_rank_full_multi(*head, *tail)


COMMON_BAD = [(dict(U=-1), ERR_ARG), (dict(num_nodes=0), ERR_ARG), (dict(n_items=-1), ERR_ARG), (dict(n_items=2 ** 31 - 1), ERR_ARG),
              (dict(Q=-1), ERR_ARG), (dict(item_lo=-1), ERR_RANGE), (dict(item_lo=150), ERR_RANGE), (dict(repr=None), ERR_ARG),
              (dict(unids=None), ERR_ARG), (dict(pos_rowptr=None), ERR_ARG), (dict(pos_items=None), ERR_ARG),
              (dict(above=None), ERR_ARG), (dict(below=None), ERR_ARG), (dict(pos_score=None), ERR_ARG), (dict(n_neg=None), ERR_ARG),
              (dict(ws=None), ERR_ARG), (dict(excl_items=None), ERR_ARG), (dict(W=0), ERR_ARG), (dict(W=6), ERR_ARG)]
BAD = ([('mlp', o, rc) for o, rc in COMMON_BAD + [(dict(W=68), ERR_ARG), (dict(fc1_w=None), ERR_ARG), (dict(fc1_b=None), ERR_ARG),
                                                  (dict(fc2_w=None), ERR_ARG), (dict(fc2_b=None), ERR_ARG)]] +
       [('dot', o, rc) for o, rc in COMMON_BAD + [(dict(W=260), ERR_ARG), (dict(W=2), ERR_ARG)]])


def case_id(form, over, i):
    return '%s-%r#%d' % (form, {k: 'ptr' if isinstance(v, C.c_void_p) else v for k, v in over.items()}, i)


@pytest.mark.parametrize('form,over,rc', BAD, ids=[case_id(f, o, i) for i, (f, o, _) in enumerate(BAD)])
def test_argument_errors_need_no_device(form, over, rc):
    assert call(form, **over) == rc
    assert _lib.last_error()


@pytest.mark.parametrize('form', ['mlp', 'dot'])
def test_short_workspace_and_empty_call(form):
    lib = _lib.load()
    query = lib.pea_rank_multi_workspace_bytes if form == 'mlp' else lib.pea_dot_rank_multi_workspace_bytes
    need = query(10, 30, 100, 16)
    assert call(form, ws_bytes=need - 1) == ERR_NOMEM
    assert call(form, U=0, Q=0, ws_bytes=query(0, 0, 100, 16)) == OK       # no user: nothing is launched, nothing is read
    assert call(form, U=0, Q=0, ws_bytes=query(0, 0, 100, 16) - 1) == ERR_NOMEM


def test_host_validation_needs_no_launch(monkeypatch):
    """the checks of scoring._rank_full_multi that mirror _catalogue_args run before the library is asked for anything but its
    handle: a CPU table is enough to reach them"""
    monkeypatch.setattr(_lib, 'require_device', _lib.load)
    tb = torch.zeros(20, 8)
    u = torch.arange(3)
    rp, it = torch.tensor([0, 1, 1, 2]), torch.tensor([5, 6])
    fc = (torch.zeros(8, 16), torch.zeros(8), torch.zeros(1, 8), torch.zeros(1))
    with pytest.raises(ValueError):
        engine.rank_full_multi(tb, u, rp[:3], it, (4, 10), *fc)                     # rowptr one short
    with pytest.raises(ValueError):
        engine.rank_full_multi(tb, u, rp.to(torch.int32), it, (4, 10), *fc)         # dtype
    with pytest.raises(ValueError):
        engine.rank_full_multi(tb, u, rp, it.view(1, 2), (4, 10), *fc)              # shape
    with pytest.raises(ValueError):
        engine.rank_full_multi(tb, u, rp, it, (10, 4), *fc)                         # catalogue
    with pytest.raises(ValueError):
        engine.dot_rank_full_multi(tb, u, rp, it, (4, 10))                          # the dot table must live on the GPU


# ---------------------------------------------------------------- positives_csr
def test_positives_csr_from_edges():
    edges = np.array([[3, 3, 1, 3, 9, 3], [7, 5, 2, 7, 1, 6]])                      # unordered, (3, 7) twice, user 9 not asked for
    rowptr, items = positives_csr(edges, np.array([3, 1, 4, 3]))
    assert rowptr.dtype == torch.int64 and items.dtype == torch.int64
    assert rowptr.tolist() == [0, 3, 4, 4, 7] and items.tolist() == [5, 6, 7, 2, 5, 6, 7]
    rowptr2, items2 = positives_csr(torch.from_numpy(edges.astype(np.float64)), torch.tensor([3, 1, 4, 3]))
    assert torch.equal(rowptr, rowptr2) and torch.equal(items, items2)
    rowptr3, items3 = positives_csr(np.zeros((2, 0)), np.array([3, 1]))
    assert rowptr3.tolist() == [0, 0, 0] and items3.numel() == 0
    with pytest.raises(ValueError):
        positives_csr(np.zeros((3, 4)), np.array([1]))


def test_positives_csr_from_lists():
    rowptr, items = positives_csr([[5, 2, 5], [], [9], [2, 1]], np.array([3, 1, 3, 0]))       # a repeated user, a row of its own each
    assert rowptr.tolist() == [0, 2, 2, 3, 5] and items.tolist() == [2, 5, 9, 1, 2]
    rowptr, items = positives_csr([[], []], torch.tensor([3, 1]))
    assert rowptr.tolist() == [0, 0, 0] and items.numel() == 0 and items.dtype == torch.int64
    with pytest.raises(ValueError):
        positives_csr([[1], [2]], np.array([3]))
    with pytest.raises(ValueError):
        positives_csr([[1], [-2]], np.array([3, 4]))


# ---------------------------------------------------------------- the metric layer
def counts_of(pos, neg):
    pos, neg = np.asarray(pos), np.asarray(neg)
    above = (neg[None, :] > pos[:, None]).sum(axis=1)
    below = (neg[None, :] < pos[:, None]).sum(axis=1)
    return above, below


def brute_force(pos, neg):
    """the metrics from the merged list itself: a stable descending sort of [pos || neg] puts a positive ahead of an equal
    negative and equal positives in row order"""
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    p = pos.size
    order = np.argsort(-np.concatenate([pos, neg]), kind='stable')
    hit = order < p
    places = np.flatnonzero(hit)
    out = {'HR': np.array([float(hit[:k].any()) for k in KS]),
           'NDCG_ref': np.array([hit[:k].sum() / np.log2(np.argmax(hit[:k]) + 2) for k in KS]),
           'Recall': np.array([hit[:k].sum() / p for k in KS]),
           'Precision': np.array([hit[:k].sum() / k for k in KS]),
           'NDCG': np.array([sum(1.0 / np.log2(i + 2) for i in range(min(k, hit.size)) if hit[i]) /
                             sum(1.0 / np.log2(i + 2) for i in range(min(p, k))) for k in KS]),
           'MRR': 1.0 / (places[0] + 1.0),
           'AP': np.mean([hit[:i + 1].sum() / (i + 1.0) for i in places]),
           'AUC': np.mean([1.0 if a > b else 0.0 for a in pos for b in neg])}
    return out


def test_metrics_against_the_reference_fixture():
    with open(os.path.join(ROOT, 'tests', 'golden', 'rec_utils_multi.json')) as f:
        golden = json.load(f)
    assert golden['ks'] == KS.tolist() and len(golden['cases']) == 20
    assert sorted({len(c['pos']) for c in golden['cases']}) == list(range(1, 13))
    rowptr, above, below, score, n_neg = [0], [], [], [], []
    for c in golden['cases']:
        a, b = counts_of(np.float32(c['pos']), np.float32(c['neg']))
        above += a.tolist(); below += b.tolist(); score += c['pos']
        rowptr.append(len(above)); n_neg.append(len(c['neg']))
    m = solvers.multi_metrics_from_counts(above, np.float32(score), below, rowptr, n_neg)
    for q, c in enumerate(golden['cases']):
        assert m['HR'][q].tolist() == c['hit'], q
        np.testing.assert_allclose(m['NDCG_ref'][q], c['ndcg'], rtol=1e-12, atol=0, err_msg=str(q))
        np.testing.assert_allclose(m['AUC'][q], c['auc'], rtol=1e-12, atol=0, err_msg=str(q))
        bf = brute_force(c['pos'], c['neg'])                       # and the hit vector the reference built is the brute force's
        assert bf['HR'].tolist() == c['hit']


@pytest.mark.parametrize('levels', [0, 7, 3])
def test_metrics_against_brute_force(levels):
    """levels > 0: integer scores in [0, levels): ties between a positive and negatives and between positives are the rule"""
    rng = np.random.default_rng(100 + levels)
    rowptr, above, below, score, n_neg, users = [0], [], [], [], [], []
    for _ in range(40):
        p, n = int(rng.integers(1, 26)), int(rng.integers(1, 120))
        if levels:
            pos, neg = rng.integers(0, levels, p).astype(np.float32), rng.integers(0, levels, n).astype(np.float32)
        else:
            pos, neg = rng.standard_normal(p).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        a, b = counts_of(pos, neg)
        above += a.tolist(); below += b.tolist(); score += pos.tolist()
        rowptr.append(len(above)); n_neg.append(n); users.append((pos, neg))
    m = solvers.multi_metrics_from_counts(np.int32(above), np.float32(score), np.int32(below), np.int64(rowptr), np.int32(n_neg))
    assert sorted(m) == sorted(solvers.MULTI_METRICS)
    for q, (pos, neg) in enumerate(users):
        bf = brute_force(pos, neg)
        for name in solvers.MULTI_METRICS:
            assert m[name].dtype == np.float64
            np.testing.assert_allclose(m[name][q], bf[name], rtol=1e-12, atol=0, err_msg='%s of user %d' % (name, q))


def test_one_positive_is_metrics_from_ranks():
    rank = np.array([0, 3, 4, 5, 19, 20, 77])
    m = solvers.multi_metrics_from_counts(rank, np.zeros(7, np.float32), 100 - rank, np.arange(8), np.full(7, 100))
    hr, ndcg = solvers.metrics_from_ranks(rank)
    assert np.array_equal(m['HR'], hr) and np.array_equal(m['NDCG_ref'], ndcg) and np.array_equal(m['NDCG'], ndcg)
    np.testing.assert_array_equal(m['AUC'], (100 - rank) / 100.0)
    with pytest.raises(ValueError):
        solvers.multi_metrics_from_counts(rank, np.zeros(7), 100 - rank, np.arange(7), np.full(7, 100))


# ---------------------------------------------------------------- a numpy scorer standing in for the model
class NumpyModel:
    """a model with a rank_full of its own over a score matrix [N, N] (CPU tensors in and out, engine.rank_full's contract)"""

    def __init__(self, scores):
        self.scores = scores
        self.cached_repr = torch.zeros(1)
        self.calls = 0

    def rank_full(self, unids, pos_items, item_range, exclude=None):
        self.calls += 1
        lo, hi = item_range
        unids, pos_items = unids.numpy(), pos_items.numpy()
        rowptr, items = (t.numpy() for t in exclude) if exclude is not None else (np.zeros(unids.size + 1, np.int64), None)
        rank, auc, ps = [], [], []
        for q, (u, p) in enumerate(zip(unids, pos_items)):
            gone = set(items[rowptr[q]:rowptr[q + 1]].tolist()) | {int(p)}
            neg = np.array([self.scores[u, i] for i in range(lo, hi) if i not in gone], dtype=np.float32)
            s = np.float32(self.scores[u, p])
            rank.append((neg > s).sum()); ps.append(s)
            auc.append(np.float32((neg < s).sum()) / np.float32(neg.size) if neg.size else np.float32(0))
        return torch.tensor(rank, dtype=torch.int32), torch.tensor(auc, dtype=torch.float32), torch.tensor(ps, dtype=torch.float32)


def multi_case(seed, levels=5):
    rng = np.random.default_rng(seed)
    n_nodes, lo, hi = 60, 10, 50
    scores = rng.integers(0, levels, (n_nodes, n_nodes)).astype(np.float32) if levels else \
        rng.standard_normal((n_nodes, n_nodes)).astype(np.float32)
    u_nids = np.array([0, 3, 3, 7, 9])
    lists = [sorted(rng.choice(np.arange(5, 55), size=k, replace=False).tolist()) for k in (1, 4, 9, 2, 12)]   # some outside [10, 50)
    excl_rows = [sorted(rng.choice(np.arange(5, 55), size=k, replace=False).tolist()) for k in (0, 6, 3, 30, 11)]
    excl_rows[2] = sorted(set(excl_rows[2]) | set(lists[2][:2]))                      # positives inside the exclusion row
    ex_rowptr = np.cumsum([0] + [len(r) for r in excl_rows])
    exclude = (torch.tensor(ex_rowptr, dtype=torch.int64), torch.tensor(sum(excl_rows, []), dtype=torch.int64))
    return scores, u_nids, lists, excl_rows, exclude, (lo, hi)


def brute_counts(scores, u_nids, lists, excl_rows, item_range):
    lo, hi = item_range
    above, below, ps, n_neg, negs = [], [], [], [], []
    for u, pos, ex in zip(u_nids, lists, excl_rows):
        neg = np.array([scores[u, i] for i in range(lo, hi) if i not in set(pos) | set(ex)], dtype=np.float32)
        negs.append(neg)
        n_neg.append(neg.size)
        for p in pos:
            above.append(int((neg > scores[u, p]).sum())); below.append(int((neg < scores[u, p]).sum())); ps.append(scores[u, p])
    return np.array(above), np.array(below), np.float32(ps), np.array(n_neg), negs


@pytest.mark.parametrize('levels', [5, 0])
def test_flattened_route_against_brute_force(levels):
    scores, u_nids, lists, excl_rows, exclude, item_range = multi_case(3, levels)
    rowptr, items = positives_csr(lists, u_nids)
    model = NumpyModel(scores)
    above, below, ps, n_neg = solvers.rank_full_multi_flattened(model.rank_full, u_nids, rowptr.numpy(), items.numpy(), item_range,
                                                                exclude)
    want = brute_counts(scores, u_nids, lists, excl_rows, item_range)
    assert model.calls == 1
    for got, exp in zip((above, below, ps, n_neg), want[:4]):
        assert np.array_equal(got, exp)
    # no exclusion at all
    above, below, ps, n_neg = solvers.rank_full_multi_flattened(model.rank_full, u_nids, rowptr.numpy(), items.numpy(), item_range)
    want = brute_counts(scores, u_nids, lists, [[]] * 5, item_range)
    for got, exp in zip((above, below, ps, n_neg), want[:4]):
        assert np.array_equal(got, exp)


def test_metrics_full_multi_through_a_models_own_rank_full():
    scores, u_nids, lists, excl_rows, exclude, item_range = multi_case(4, 6)
    model = NumpyModel(scores)
    got = solvers.metrics_full_multi(model, u_nids, lists, item_range, exclude)
    *_, negs = brute_counts(scores, u_nids, lists, excl_rows, item_range)
    per_user = [brute_force([scores[u, p] for p in pos], neg) for u, pos, neg in zip(u_nids, lists, negs)]
    assert sorted(got) == sorted(solvers.MULTI_METRICS)
    for name in solvers.MULTI_METRICS:
        np.testing.assert_allclose(got[name], np.mean([m[name] for m in per_user], axis=0), rtol=1e-12, atol=0, err_msg=name)
    # the same through the CSR a caller built itself
    again = solvers.metrics_full_multi(model, u_nids, positives_csr(lists, u_nids), item_range, exclude)
    for name in solvers.MULTI_METRICS:
        assert np.array_equal(got[name], again[name])


def test_value_errors():
    scores, u_nids, lists, excl_rows, exclude, item_range = multi_case(5)
    model = NumpyModel(scores)
    with pytest.raises(ValueError, match='No pos or neg samples found in evaluation!'):
        solvers.metrics_full_multi(model, u_nids, [lists[0], [], lists[2], lists[3], lists[4]], item_range, exclude)
    assert model.calls == 0
    everything = list(range(item_range[0], item_range[1]))
    rows = [[], everything[1:], [], [], []]                          # user 1: every catalogue item excluded or (item 10) positive
    ex = (torch.tensor(np.cumsum([0] + [len(r) for r in rows])), torch.tensor(sum(rows, []), dtype=torch.int64))
    with pytest.raises(ValueError, match='No pos or neg samples found in evaluation!'):
        solvers.metrics_full_multi(model, u_nids, [[12], [10], [12], [12], [12]], item_range, ex)
    with pytest.raises(ValueError, match='No pos or neg samples found in evaluation!'):
        solvers.metrics_full_multi(model, [], [], item_range)


class FakeDataset:
    def __init__(self, test_map, u2i, acc_iid, num_iids):
        self.test_pos_unid_inid_map = test_map
        self.edge_index_nps = {'user2item': u2i}
        self.type_accs = {'iid': acc_iid}
        self.num_iids = num_iids


def test_from_dataset_reads_lists_of_any_length():
    scores, u_nids, lists, excl_rows, _, item_range = multi_case(6, 4)
    keep = [0, 1, 3, 4]                                              # a dict holds a user once
    test_map = {int(u_nids[q]): lists[q] for q in keep}
    u2i = np.array([[u_nids[q] for q in keep for _ in excl_rows[q]], [i for q in keep for i in excl_rows[q]]], dtype=np.float64)
    model = NumpyModel(scores)
    got = solvers.metrics_full_multi_from_dataset(model, FakeDataset(test_map, u2i, item_range[0], item_range[1] - item_range[0]))
    in_cat = [[i for i in excl_rows[q] if item_range[0] <= i < item_range[1]] for q in keep]
    ex = (torch.tensor(np.cumsum([0] + [len(r) for r in in_cat])), torch.tensor(sum(in_cat, []), dtype=torch.int64))
    want = solvers.metrics_full_multi(model, u_nids[keep], [lists[q] for q in keep], item_range, ex)
    for name in solvers.MULTI_METRICS:
        assert np.array_equal(got[name], want[name])
