"""CPU: the full-catalogue scan over the NFM fold without a device -- the sixth header (include/peahip_fm_eval.h) against
_lib.FM_EVAL_SIGNATURES and the library's exports, the three pure queries, every argument error of the three entry points
(returned with NULL device pointers, so before anything is launched), and NFMRecsysModel.rank_full_multi on a CPU model with
small-integer weights (no blocking of torch's can move a bit) against solvers.rank_full_multi_flattened over its rank_full."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from graph_recsys_benchmark_amd import _lib, engine, solvers
from graph_recsys_benchmark_amd.models import NFMRecsysModel
from test_nfm_cpu import ctypes_width, fake, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_RANGE, ERR_NOMEM = -1, -2, -4
NAMES = ['pea_nfm_rank_full', 'pea_nfm_rank_full_multi', 'pea_nfm_recommend_topk', 'pea_nfm_scan_splits', 'pea_nfm_scan_supported',
         'pea_nfm_scan_workspace_bytes']


# ---------------------------------------------------------------- the sixth header
def test_sixth_header_matches_its_ctypes_table():
    protos = prototypes('peahip_fm_eval.h')
    assert sorted(protos) == sorted(_lib.FM_EVAL_SIGNATURES) == NAMES
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.FM_EVAL_SIGNATURES[name]
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    others = set()
    for header in ('peahip.h', 'peahip_kge.h', 'peahip_eval.h', 'peahip_sample.h', 'peahip_fm.h'):
        others |= set(prototypes(header))
    assert not others & set(protos)
    tables = (_lib.SIGNATURES, _lib.KGE_SIGNATURES, _lib.EVAL_SIGNATURES, _lib.SAMPLE_SIGNATURES, _lib.FM_SIGNATURES)
    assert not set().union(*[set(t) for t in tables]) & set(_lib.FM_EVAL_SIGNATURES)
    assert len(_lib.SIGNATURES) == 112 and len(_lib.FM_SIGNATURES) == 5          # where test_cabi.py and test_nfm_cpu.py pin them
    text = open(os.path.join(ROOT, 'include', 'peahip_fm_eval.h')).read()
    assert re.search(r'#define\s+PEA_NFM_SCAN_USERS\s+%d\b' % _lib.NFM_SCAN_USERS, text)


# ---------------------------------------------------------------- the pure queries
def test_scan_supported_is_pure_and_implies_the_scorer():
    lib = _lib.load()
    for e, h, k in itertools.product((0, 4, 6, 20, 64, 128, 132), (0, 4, 6, 20, 64, 128, 132), (0, 1, 128, 129)):
        got = lib.pea_nfm_scan_supported(e, h, k)
        assert got == lib.pea_nfm_scan_supported(e, h, k) and got in (0, 1)
        assert not got or lib.pea_nfm_supported(e, h), (e, h, k)
        # every width the scorer takes fits the scan's LDS (the header says so): K alone decides among them
        assert got == int(bool(lib.pea_nfm_supported(e, h)) and k <= 128), (e, h, k)
        assert engine.nfm_scan_supported(e, h, k) == bool(got)
    assert not lib.pea_nfm_scan_supported(64, 64, -1)


def test_scan_splits_is_pure_and_bounded():
    lib = _lib.load()
    for k in (20, 128):
        assert lib.pea_nfm_scan_splits(3, 1100, k) >= 2 and engine.nfm_scan_splits(3, 1100, k) == lib.pea_nfm_scan_splits(3, 1100, k)
    for n_users, n_items, k in itertools.product((0, 1, 7, 8, 9, 100, 1016, 1024, 4096, 162541), (0, 1, 63, 64, 65, 511, 1100, 59047, 1 << 22),
                                                 (0, 1, 16, 17, 20, 100, 127, 128)):
        s = lib.pea_nfm_scan_splits(n_users, n_items, k)
        assert s == lib.pea_nfm_scan_splits(n_users, n_items, k) and 1 <= s <= 64
        assert s * max(k, 1) <= 2048, (n_users, n_items, k)
    assert lib.pea_nfm_scan_splits(-1, 10, 1) == 0 and lib.pea_nfm_scan_splits(1, -1, 1) == 0 and lib.pea_nfm_scan_splits(1, 10, 129) == 0


def test_workspace_query_refuses_and_is_monotone():
    lib = _lib.load()
    query = lib.pea_nfm_scan_workspace_bytes
    base = dict(n_users=100, q=300, n_excl=1000, n_items=5000, k=20, e=64, h=64)
    order = ('n_users', 'q', 'n_excl', 'n_items', 'k', 'e', 'h')
    size = lambda **over: query(*[dict(base, **over)[name] for name in order])
    assert size() > 0 and size() == size()
    for bad in (dict(e=6), dict(h=132), dict(e=0), dict(k=129), dict(k=-1), dict(n_users=-1), dict(q=-1), dict(n_excl=-1), dict(n_items=-1),
                dict(n_items=(1 << 31) - 1)):
        assert size(**bad) == 0, bad
    sweeps = dict(n_users=(0, 1, 7, 8, 9, 64, 1000, 1015, 1016, 1017, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 162541),
                  q=(0, 1, 63, 64, 65, 1000, 4096, 100000), n_excl=(0, 1, 1000, 24700000),
                  n_items=(0, 1, 64, 511, 512, 1023, 1024, 1100, 5000, 59047, 1 << 20),
                  k=(0, 1, 2, 16, 17, 20, 100, 120, 121, 127, 128), e=(4, 20, 64, 128), h=(4, 24, 64, 128))
    for name, values in sweeps.items():
        for other in (dict(), dict(n_users=3, n_items=1100), dict(n_users=4096, n_items=59047, q=40000)):
            sizes = [size(**dict(other, **{name: v})) for v in values]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (name, other, sizes)
    assert size(n_users=162541, q=162541, n_items=59047) < 1 << 30        # the bounds stay far from the S = 64 worst case


# ---------------------------------------------------------------- argument errors, with NULL device pointers
FOLD = ('E', 'H', 'U', 'I', 'emb', 'ld_emb', 'lin', 'wf', 'bf', 'w2', 'bias')
ORDER = {
    'pea_nfm_recommend_topk': FOLD + ('uids', 'n', 'K', 'lo', 'n_items', 'node0', 'ex_rowptr', 'ex_items', 'out_items', 'out_scores', 'err',
                                      'ws', 'ws_bytes', 'stream'),
    'pea_nfm_rank_full': FOLD + ('uids', 'n', 'pos', 'lo', 'n_items', 'node0', 'ex_rowptr', 'ex_items', 'rank', 'auc', 'pos_score', 'err', 'ws',
                                 'ws_bytes', 'stream'),
    'pea_nfm_rank_full_multi': FOLD + ('uids', 'n', 'pos_rowptr', 'pos', 'Q', 'lo', 'n_items', 'node0', 'ex_rowptr', 'ex_items', 'above', 'below',
                                       'pos_score', 'n_neg', 'err', 'ws', 'ws_bytes', 'stream'),
}
SCALARS = dict(E=16, H=8, U=50, I=60, ld_emb=16, n=10, K=5, Q=30, lo=2, n_items=50, node0=50, ws_bytes=1 << 40, stream=None)


def scan_call(name, pointers, **over):
    """the entry point with NULL (pointers False) or stand-in device pointers and the scalars of SCALARS, `over` on top"""
    a = {k: (fake() if pointers else None) for k in ORDER[name]}
    a.update({k: v for k, v in SCALARS.items() if k in a})
    a.update(over)
    return getattr(_lib.load(), name)(*[a[k] for k in ORDER[name]])


def needed(name):
    lib, s = _lib.load(), SCALARS
    if name == 'pea_nfm_recommend_topk':
        return lib.pea_nfm_scan_workspace_bytes(s['n'], 0, 0, s['n_items'], s['K'], s['E'], s['H'])
    q = s['n'] if name == 'pea_nfm_rank_full' else s['Q']
    return lib.pea_nfm_scan_workspace_bytes(s['n'], q, 0, s['n_items'], 0, s['E'], s['H'])


BAD = [(dict(n=-1), ERR_ARG), (dict(n_items=-1), ERR_ARG), (dict(U=0), ERR_ARG), (dict(I=0), ERR_ARG), (dict(E=6), ERR_ARG),
       (dict(H=132), ERR_ARG), (dict(ld_emb=12), ERR_ARG), (dict(ld_emb=18), ERR_ARG), (dict(lo=11), ERR_RANGE), (dict(lo=-1), ERR_RANGE),
       (dict(lo=0, n_items=61), ERR_RANGE), (dict(ex_rowptr='fake'), ERR_ARG), (dict(ws_bytes='short'), ERR_NOMEM)]


@pytest.mark.parametrize('name', sorted(ORDER))
def test_argument_errors_are_returned_with_null_pointers(name):
    cases = list(BAD)
    if name == 'pea_nfm_recommend_topk':
        cases += [(dict(K=0), ERR_ARG), (dict(K=129), ERR_ARG), (dict(K=-3), ERR_ARG)]
    if name == 'pea_nfm_rank_full_multi':
        cases += [(dict(Q=-1), ERR_ARG)]
    for over, want in cases:
        over = {k: (fake() if v == 'fake' else needed(name) - 1 if v == 'short' else v) for k, v in over.items()}
        assert scan_call(name, False, **over) == want, (name, over)
        assert _lib.last_error()
    # the scalars are fine: now the NULL pointers themselves are the error, one at a time among stand-ins
    assert needed(name) > 0 and scan_call(name, False) == ERR_ARG
    optional = ('ex_rowptr', 'ex_items', 'stream')
    for key in ORDER[name]:
        if key not in SCALARS and key not in optional:
            assert scan_call(name, True, **{key: None}) == ERR_ARG, (name, key)
    assert scan_call(name, True, emb=fake(misalign=4)) == ERR_ARG and scan_call(name, True, ws=fake(misalign=8)) == ERR_ARG
    assert scan_call(name, True, ex_items=None) == ERR_ARG


# ---------------------------------------------------------------- the CPU model, integer-valued weights
N_USER, N_ITEM, E, H, ACC_I = 12, 70, 8, 12, 100
COUNTS = (1, 2, 8, 9, 17)


@pytest.fixture(scope='module')
def int_model():
    """A CPU model whose fold holds small integers: every logit is an integer that float32 holds exactly in any order"""
    g = torch.Generator().manual_seed(5)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    model = NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=E, hidden_size=H, dropout=0, acc_uids=0, acc_iids=ACC_I).eval()
    model.folded = engine.NfmFolded(ri(-1, 1, N_USER + N_ITEM, E), ri(-3, 3, N_USER + N_ITEM), ri(-2, 2, H, E), ri(-3, 3, H), ri(-2, 2, H),
                                    ri(-3, 3, 1), N_USER)
    model.cached_repr = model.folded.w
    model.USER_CHUNK, model.POS_CHUNK = 2, 5           # several chunks of users and of positives
    assert not model._fused() and not model._hip_scorer()
    return model


def multi_case():
    """users with 1, 2, 8, 9 and 17 positives over the catalogue [ACC_I + 3, ACC_I + 60): some positives lie outside it, some are
    named by the user's exclusion row too; rows strictly ascending"""
    rng = np.random.RandomState(9)
    lo, hi = ACC_I + 3, ACC_I + 60
    unids = np.array([4, 0, 11, 4, 7])
    pos, excl = [], []
    for n in COUNTS:
        row = np.sort(rng.choice(np.arange(ACC_I, ACC_I + N_ITEM), size=n, replace=False))
        pos.append(row)
        rest = np.setdiff1d(np.arange(ACC_I, ACC_I + N_ITEM), row)
        excl.append(np.sort(np.concatenate([rng.choice(rest, size=6, replace=False), row[:n // 3]])))
    pos[2][0], pos[4][-1] = ACC_I + 1, ACC_I + 65                              # outside the catalogue, below and above it
    pos[2].sort(), pos[4].sort()
    assert all(len(np.unique(r)) == len(r) for r in pos) and any(((r < lo) | (r >= hi)).any() for r in pos)
    csr = lambda rows: (torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), dtype=torch.int64),
                        torch.tensor(np.concatenate(rows), dtype=torch.int64))
    return torch.tensor(unids), csr(pos), csr(excl), (lo, hi)


def test_rank_full_multi_equals_the_flattened_route(int_model):
    unids, (pos_rowptr, pos_items), exclude, item_range = multi_case()
    assert np.diff(pos_rowptr.numpy()).tolist() == list(COUNTS)
    got = int_model.rank_full_multi(unids, pos_rowptr, pos_items, item_range, exclude=exclude)
    want = solvers.rank_full_multi_flattened(int_model.rank_full, unids.numpy(), pos_rowptr.numpy(), pos_items.numpy(), item_range, exclude)
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.int32]
    for g, w, what in zip(got, want, ('above', 'below', 'pos_score', 'n_neg')):
        assert np.array_equal(g.numpy(), w), what
    assert got[0].sum() > 0 and got[1].sum() > 0 and len(set(got[3].tolist())) > 1
    # without an exclusion the union is the positive row alone
    got = int_model.rank_full_multi(unids, pos_rowptr, pos_items, item_range)
    want = solvers.rank_full_multi_flattened(int_model.rank_full, unids.numpy(), pos_rowptr.numpy(), pos_items.numpy(), item_range)
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)


def test_metrics_full_multi_takes_the_hook(int_model):
    unids, positives, exclude, item_range = multi_case()
    calls = []
    hook = int_model.rank_full_multi
    int_model.rank_full_multi = lambda *a, **kw: calls.append(1) or hook(*a, **kw)
    try:
        got = solvers.metrics_full_multi(int_model, unids.numpy(), positives, item_range, exclude=exclude)
    finally:
        del int_model.rank_full_multi
    assert calls == [1]
    above, below, pos_score, n_neg = solvers.rank_full_multi_flattened(int_model.rank_full, unids.numpy(), positives[0].numpy(),
                                                                       positives[1].numpy(), item_range, exclude)
    per_user = solvers.multi_metrics_from_counts(above, pos_score, below, positives[0].numpy(), n_neg)
    assert sorted(got) == sorted(solvers.MULTI_METRICS)
    for name, v in per_user.items():
        np.testing.assert_array_equal(got[name], v.mean(axis=0), err_msg=name)
