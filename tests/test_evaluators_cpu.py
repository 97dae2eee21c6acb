"""CPU: evaluators.py, the one torch composition behind every model's ranking hooks, against a numpy brute force.  The score
matrix holds small integers, so ties are the rule and every comparison, count and float32 quotient is exact: all asserts are
array_equal."""
import os
import re

import numpy as np
import pytest
import torch

from graph_recsys_benchmark_amd import evaluators
from graph_recsys_benchmark_amd.models.base import MFRecsysModel

N_NODES, LO, HI = 60, 10, 50
U_NIDS = np.array([0, 3, 3, 7, 9])                       # user 3 asked for twice, with rows of its own each time
COUNTS = (1, 4, 9, 2, 12)                                # positives per requested user
NEG_INF = float('-inf')


def csr(rows):
    return (torch.tensor(np.cumsum([0] + [len(r) for r in rows]), dtype=torch.int64),
            torch.tensor([i for r in rows for i in r], dtype=torch.int64))


@pytest.fixture(scope='module')
def case():
    """scores [60, 60] of 5 levels; positives drawn from 5 .. 54 (some outside the catalogue [10, 50)); exclusion rows: an empty
    one, ones with entries outside the catalogue, one naming two of its user's positives, one leaving 2 catalogue items"""
    rng = np.random.default_rng(11)
    scores = rng.integers(0, 5, (N_NODES, N_NODES)).astype(np.float32)
    lists = [sorted(rng.choice(np.arange(5, 55), size=k, replace=False).tolist()) for k in COUNTS]
    excl = [sorted(rng.choice(np.arange(5, 55), size=k, replace=False).tolist()) for k in (0, 6, 3, 0, 11)]
    excl[2] = sorted(set(excl[2]) | set(lists[2][:2]))
    excl[3] = [5, 8] + [i for i in range(LO, HI) if i not in (17, 33)] + [52]
    assert any(i < LO or i >= HI for r in lists for i in r) and any(i < LO or i >= HI for r in excl for i in r)
    return scores, lists, excl


def callbacks(scores, u_nids=U_NIDS, seen=None):
    """(block, pairs) over the score matrix; seen collects the user chunks block was asked for"""
    s, u = torch.from_numpy(scores), torch.from_numpy(np.asarray(u_nids, dtype=np.int64))

    def block(r0, r1):
        if seen is not None:
            seen.append((r0, r1))
        return s[u[r0:r1], LO:HI]

    return block, lambda rows, items: s[u[rows], items]


def eligible(u_row, excl_row, also=()):
    gone = set(excl_row) | set(also)
    return [i for i in range(LO, HI) if i not in gone]


# ---------------------------------------------------------------- the candidate rank, the labels and losses
def test_candidate_ranks_against_brute_force():
    rng = np.random.default_rng(2)
    for c in (1, 2, 14):
        s = rng.integers(0, 4, (9, c)).astype(np.float32)
        rank, auc = evaluators.candidate_ranks(torch.from_numpy(s))
        assert rank.dtype == torch.int32 and auc.dtype == torch.float32
        assert np.array_equal(rank.numpy(), [(row[1:] > row[0]).sum() for row in s])
        assert np.array_equal(auc.numpy(), [np.float32((row[1:] < row[0]).sum()) / np.float32(max(c - 1, 1)) for row in s])
    assert c == 14 and (s[:, 1:] == s[:, :1]).any()                   # a tie with the positive counted on neither side


def test_leave_one_out_loss_is_the_torch_loss_row_by_row():
    g = torch.Generator().manual_seed(4)
    pred = torch.randn((6, 9), generator=g, dtype=torch.float64)
    label = torch.tensor([1.0] + [0.0] * 8, dtype=torch.float64)
    for kind, loss in (('mse', torch.nn.MSELoss()), ('bce', torch.nn.BCEWithLogitsLoss())):
        got = evaluators.leave_one_out_loss(pred, kind)
        assert got.shape == (6,)
        for row in range(6):
            assert torch.equal(got[row], loss(pred[row], label)), (kind, row)
    with pytest.raises(ValueError):
        evaluators.leave_one_out_loss(pred, 'bpr')


class _DotMF(MFRecsysModel):
    def _init(self, **kwargs):
        self.user, self.item = torch.nn.Embedding(7, 4), torch.nn.Embedding(11, 4)

    def reset_parameters(self):
        pass

    def forward(self, uid, iid):
        return torch.sum(self.user(uid) * self.item(iid), dim=-1)


def test_eval_pairs_is_the_eval_branch_of_the_mf_loss():
    torch.manual_seed(6)
    model = _DotMF().eval()
    batch = torch.tensor([[2, 5, 0], [2, 5, 9], [2, 5, 3], [2, 5, 10]])
    with torch.no_grad():
        pos_pred = model.predict(batch[:, 0], batch[:, 1])[:1]        # reference models/base.py:117-122, restated
        neg_pred = model.predict(batch[:, 0], batch[:, 2])
        want_pred = torch.cat([pos_pred, neg_pred])
        want_label = torch.cat([torch.ones_like(pos_pred), torch.zeros_like(neg_pred)]).float()
        pred, label = evaluators.eval_pairs(model.predict, batch)
        assert torch.equal(pred, want_pred) and torch.equal(label, want_label) and label.dtype == torch.float32
        assert label.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
        assert torch.equal(model.loss(batch), torch.nn.BCEWithLogitsLoss()(want_pred, want_label))


# ---------------------------------------------------------------- the exclusion mask
def test_exclusion_mask_reads_the_rows_it_is_asked_for(case):
    _, _, excl = case
    for r0, r1 in ((0, 5), (0, 2), (2, 5), (3, 4), (1, 1)):
        mask = evaluators.exclusion_mask(csr(excl), 5, LO, HI, r0, r1, torch.device('cpu'))
        want = np.array([[i in excl[q] for i in range(LO, HI)] for q in range(r0, r1)], dtype=bool).reshape(r1 - r0, HI - LO)
        assert mask.dtype == torch.bool and np.array_equal(mask.numpy(), want)
    assert not evaluators.exclusion_mask(None, 5, LO, HI, 0, 5, torch.device('cpu')).any()
    with pytest.raises(ValueError):
        evaluators.exclusion_mask(csr(excl), 4, LO, HI, 0, 4, torch.device('cpu'))


# ---------------------------------------------------------------- the three compositions
@pytest.mark.parametrize('user_chunk', [2, 3, 256])
@pytest.mark.parametrize('with_exclude', [True, False])
def test_rank_full_against_brute_force(case, user_chunk, with_exclude):
    scores, lists, excl = case
    rows = excl if with_exclude else [[]] * 5
    pos = [lists[0][0], lists[1][0], lists[2][0], 17, lists[4][-1]]      # [2]: inside its exclusion row; [3]: one of the 2 left
    assert pos[2] in rows[2] or not with_exclude
    seen = []
    rank, auc, pos_score = evaluators.rank_full(*callbacks(scores, seen=seen), torch.tensor(pos), (LO, HI),
                                                csr(rows) if with_exclude else None, user_chunk)
    assert [t.dtype for t in (rank, auc, pos_score)] == [torch.int32, torch.float32, torch.float32]
    assert seen == [(r0, min(r0 + user_chunk, 5)) for r0 in range(0, 5, user_chunk)]
    for q, (u, p) in enumerate(zip(U_NIDS, pos)):
        neg = scores[u, eligible(u, rows[q], [p])]
        assert int(rank[q]) == (neg > scores[u, p]).sum() and float(pos_score[q]) == scores[u, p]
        assert auc[q].item() == np.float32((neg < scores[u, p]).sum()) / np.float32(max(neg.size, 1))
    if with_exclude:
        assert eligible(7, rows[3], [17]) == [33]                          # one negative left for user 3


def brute_topk(scores, u, excl_row, k):
    keep = sorted(eligible(u, excl_row), key=lambda i: (-scores[u, i], i))[:k]
    return keep + [-1] * (k - len(keep)), [scores[u, i] for i in keep] + [NEG_INF] * (k - len(keep))


@pytest.mark.parametrize('user_chunk', [2, 3, 256])
@pytest.mark.parametrize('k', [1, 7, 40, 55])
def test_recommend_against_brute_force(case, user_chunk, k):
    """k = 7 leaves user row 3 (2 eligible items) a tail of 5; k = 55 is larger than the catalogue of 40"""
    scores, _, excl = case
    block, _ = callbacks(scores)
    items, top = evaluators.recommend(block, 5, k, (LO, HI), csr(excl), user_chunk)
    assert items.shape == top.shape == (5, k) and items.dtype == torch.int64 and top.dtype == torch.float32
    for q, u in enumerate(U_NIDS):
        want_i, want_s = brute_topk(scores, u, excl[q], k)
        assert np.array_equal(items[q].numpy(), want_i) and np.array_equal(top[q].numpy(), np.float32(want_s)), q
    if k >= 7:
        assert items[3].tolist()[:3] == sorted([17, 33], key=lambda i: (-scores[7, i], i)) + [-1] and top[3, 2] == NEG_INF
        tied = (top[0, 1:] == top[0, :-1]) & (items[0, 1:] >= 0)
        assert tied.any() and (items[0, 1:][tied] > items[0, :-1][tied]).all()       # equal scores: the lower node id first
    # no exclusion: everybody gets the whole catalogue
    items, top = evaluators.recommend(block, 5, k, (LO, HI), None, user_chunk)
    for q, u in enumerate(U_NIDS):
        want_i, want_s = brute_topk(scores, u, [], k)
        assert np.array_equal(items[q].numpy(), want_i) and np.array_equal(top[q].numpy(), np.float32(want_s)), q


def brute_multi(scores, lists, excl):
    above, below, ps, n_neg = [], [], [], []
    for u, pos, ex in zip(U_NIDS, lists, excl):
        neg = scores[u, eligible(u, ex, pos)]
        n_neg.append(neg.size)
        for p in pos:
            above.append((neg > scores[u, p]).sum()), below.append((neg < scores[u, p]).sum()), ps.append(scores[u, p])
    return np.array(above), np.array(below), np.float32(ps), np.array(n_neg)


@pytest.mark.parametrize('user_chunk', [2, 3, 256])
@pytest.mark.parametrize('with_exclude', [True, False])
def test_rank_full_multi_against_brute_force(case, user_chunk, with_exclude):
    """rows of 1 to 12 positives compared 5 at a time: a user's row spans several chunks, a chunk never spans two user blocks"""
    scores, lists, excl = case
    rows = excl if with_exclude else [[]] * 5
    assert set(lists[2][:2]) <= set(excl[2])                               # positives inside the exclusion row
    got = evaluators.rank_full_multi(*callbacks(scores), *csr(lists), (LO, HI), csr(rows) if with_exclude else None, user_chunk, 5)
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.int32]
    for g, w, what in zip(got, brute_multi(scores, lists, rows), ('above', 'below', 'pos_score', 'n_neg')):
        assert np.array_equal(g.numpy(), w), what
    assert got[0].sum() > 0 and got[1].sum() > 0
    # one positive per user: the single-positive form, rank = above and auc = below / n_neg
    first = [[r[0]] for r in lists]
    above, below, ps, n_neg = evaluators.rank_full_multi(*callbacks(scores), *csr(first), (LO, HI), csr(rows), user_chunk, 5)
    rank, auc, pos_score = evaluators.rank_full(*callbacks(scores), csr(first)[1], (LO, HI), csr(rows), user_chunk)
    assert torch.equal(rank, above) and torch.equal(pos_score, ps) and torch.equal(auc, below.float() / n_neg.clamp(min=1))


def test_nobody_asked(case):
    """zero users and Q == 0: empty outputs of the right dtype and shape, and n_neg still counted per user"""
    scores, _, excl = case
    block, pairs = callbacks(scores, u_nids=[])
    none = torch.zeros(0, dtype=torch.int64)
    outs = evaluators.rank_full(block, pairs, none, (LO, HI), csr([]))
    assert [(t.dtype, tuple(t.shape)) for t in outs] == [(torch.int32, (0,)), (torch.float32, (0,)), (torch.float32, (0,))]
    outs = evaluators.recommend(block, 0, 7, (LO, HI), csr([]))
    assert [(t.dtype, tuple(t.shape)) for t in outs] == [(torch.int64, (0, 7)), (torch.float32, (0, 7))]
    outs = evaluators.rank_full_multi(block, pairs, torch.zeros(1, dtype=torch.int64), none, (LO, HI))
    assert [(t.dtype, tuple(t.shape)) for t in outs] == [(torch.int32, (0,))] * 2 + [(torch.float32, (0,)), (torch.int32, (0,))]
    above, below, ps, n_neg = evaluators.rank_full_multi(*callbacks(scores), torch.zeros(6, dtype=torch.int64), none, (LO, HI),
                                                         csr(excl), 2, 5)
    assert [(t.dtype, tuple(t.shape)) for t in (above, below, ps)] == [(torch.int32, (0,))] * 2 + [(torch.float32, (0,))]
    assert n_neg.dtype == torch.int32 and n_neg.tolist() == [len(eligible(u, ex)) for u, ex in zip(U_NIDS, excl)]
    assert n_neg[3] == 2 and n_neg[0] == HI - LO


def test_evaluators_imports_torch_alone():
    with open(os.path.join(os.path.dirname(evaluators.__file__), 'evaluators.py')) as f:
        imports = [line.strip() for line in f if re.match(r'\s*(import|from)\s', line)]
    assert imports == ['import torch', 'import torch.nn.functional as F']
