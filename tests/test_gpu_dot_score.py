"""GPU: the inner-product scorer (csrc/dot_score.hip) -- pair prediction, the sampled evaluator, full-catalogue top-K and
the all-item rank -- against float64.

The float64 side is torch float64 of s(u, i) = sum_d repr[u, d] repr[i, d] on the same fp32 inputs.  The kernels compute
that sum as one fma chain of length D, whose rigorous error bound is
    |s32 - s| <= b(u, i) = g sum_d |repr[u, d] repr[i, d]|,   g = D 2^-24 / (1 - D 2^-24)
(computed in float64 here).  Two items can swap places at the K-th place only if their float64 scores are closer than the
sum of their bounds, so membership at the cut is checked with the window b(u, j) + b(u, K-th item); the integer-valued
tables have no rounding at all and are compared exactly.
"""
import numpy as np
import pytest
import torch

import helpers
from graph_recsys_benchmark_amd import _lib, engine

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NINF = float('-inf')


def gamma(D):
    return D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------ inputs
def table(seed, n_nodes, D, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        return torch.randint(-3, 4, (n_nodes, D), generator=g).float().to(DEV)
    return torch.randn(n_nodes, D, generator=g).to(DEV)


def f64_scores(repr_, unids, lo, n):
    """([U, n] float64 scores, [U, n] error bounds b) of the requested users against the catalogue [lo, lo + n)"""
    u, v = repr_[unids].double(), repr_[lo:lo + n].double()
    return u @ v.T, gamma(repr_.shape[1]) * (u.abs() @ v.abs().T)


def random_exclusion(rng, U, lo, n, n_nodes, cmin=11, cmax=299):
    """per user cmin..cmax distinct catalogue items (at most half the catalogue) plus a few ids outside it, ascending"""
    rows = []
    for _ in range(U):
        c = int(rng.integers(min(cmin, max(n // 2, 1)), min(cmax, max(n // 2, 1)) + 1))
        inside = rng.choice(n, size=c, replace=False) if n < 4096 else np.unique(rng.integers(0, n, size=c))
        outside = np.concatenate([rng.integers(0, max(lo, 1), size=2), rng.integers(lo + n, n_nodes, size=2)])
        outside = outside[(outside < lo) | (outside >= lo + n)]
        rows.append(np.unique(np.concatenate([inside + lo, outside])).astype(np.int64))
    return rows


def to_csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(items.astype(np.int64)).to(DEV)


def eligible_mask(U, lo, n, exclude):
    mask = torch.ones((U, n), dtype=torch.bool, device=DEV)
    if exclude is not None:
        ptr, items = exclude
        rows = torch.repeat_interleave(torch.arange(U, device=DEV), ptr[1:] - ptr[:-1])
        cols = items - lo
        inside = (cols >= 0) & (cols < n)
        mask[rows[inside], cols[inside]] = False
    return mask


def layout(U, n, seed):
    """catalogue in the middle of the node range; users drawn with repeats, in random order, from a block before it"""
    rng = np.random.default_rng(seed)
    n_users = max(U * 7 // 10, 1)
    lo = n_users + 13
    n_nodes = lo + n + 29
    unids = torch.from_numpy(rng.integers(0, n_users, size=U)).to(DEV)
    return rng, lo, n_nodes, unids


def kth_band(s64, b, elig, K):
    """From float64 alone: per user the K-th eligible score s64_K with its item's bound b_K (users with >= K eligible
    items), the window w[u, j] = b[u, j] + b_K[u], and the number of OTHER eligible items inside it."""
    masked = torch.where(elig, s64, torch.full_like(s64, NINF))
    n_elig = elig.sum(1)
    full = n_elig >= K
    kk = min(K, s64.shape[1])
    top = masked.topk(kk, dim=1)
    if kk == K:
        sK, bK = top.values[:, K - 1], b.gather(1, top.indices[:, K - 1:K])[:, 0]
    else:
        sK = torch.zeros(s64.shape[0], dtype=torch.float64, device=DEV)
        bK = torch.zeros_like(sK)
    sK = torch.where(full, sK, torch.zeros_like(sK))
    w = b + bK[:, None]
    in_band = (((masked - sK[:, None]).abs() <= w) & elig).sum(1) - 1
    in_band = torch.where(full, in_band, torch.zeros_like(in_band))
    return masked, n_elig, full, sK, w, in_band


def check_topk(items, scores, s64, b, elig, K, lo, band):
    masked, n_elig, full, sK, w, _ = band
    U, n = s64.shape
    assert items.shape == (U, K) and scores.shape == (U, K) and items.dtype == torch.int64 and scores.dtype == torch.float32
    valid = items >= 0
    n_ret = valid.sum(1)
    assert torch.equal(n_ret, torch.clamp(n_elig, max=K)), 'number of returned items'
    pos = torch.arange(K, device=DEV)[None, :]
    assert torch.equal(valid, pos < n_ret[:, None]), 'valid entries must be a prefix'
    assert bool((items[~valid] == -1).all()) and bool((scores[~valid] == NINF).all()), 'padding is (-1, -inf)'
    idx = torch.where(valid, items - lo, torch.zeros_like(items))
    assert bool(((idx >= 0) & (idx < n)).all()), 'item outside the catalogue'
    assert bool(elig.gather(1, idx)[valid].all()), 'excluded item returned'
    srt = torch.where(valid, items, torch.full_like(items, -1)).sort(dim=1).values
    dup = (srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)
    assert not bool(dup.any()), 'duplicate item'
    own, own_b, own_w = s64.gather(1, idx), b.gather(1, idx), w.gather(1, idx)
    sc = scores.double()
    err = torch.where(valid, (sc - own).abs(), torch.zeros_like(own))
    if bool(valid.any()):
        print('score error / bound: worst %.3f' % float((err / own_b.clamp_min(1e-300))[valid].max()))
    assert bool((err <= own_b).all()), 'score outside the fma-chain bound'
    both = valid[:, 1:] & valid[:, :-1]
    ordered = (scores[:, :-1] > scores[:, 1:]) | ((scores[:, :-1] == scores[:, 1:]) & (items[:, :-1] < items[:, 1:]))
    assert bool((ordered | ~both).all()), 'list not sorted by (score descending, id ascending)'
    must = ((masked - sK[:, None] > w) & elig).sum(1)
    got_must = ((own - sK[:, None] > own_w) & valid).sum(1)
    assert torch.equal(must[full], got_must[full]), 'an eligible item above the band was left out'
    low = (sK[:, None] - own > own_w) & valid
    assert not bool(low[full].any()), 'an item below the band was returned'


def call_topk(tb, unids, K, lo, n, exclude=None):
    return engine.dot_recommend_topk(tb, unids, K, (lo, lo + n), exclude=exclude)


# ------------------------------------------------------------------------------------------------ 1. top-K vs float64
def near_tie_cap(D, K, n):
    """Largest share of a case's users that may have another eligible item inside the window at the K-th place.  The
    window grows with D (the bound is D 2^-24 sum |u v|) and the spacing of the scores at the cut shrinks with K, so the
    caps do; they were measured on float64 scores of standard-normal rows before any kernel existed (D = 112 at K = 128:
    4.3-8.0 % of the users; D = 224 at K = 20: 1.7-3.7 %; D = 224 at K = 128, 11-20 %, is left to the exact test)."""
    if K <= 20 or K > n:
        return 0.05 if D == 224 else 0.02
    return 0.10 if D == 112 else 0.02


MATRIX = [(U, n, K, D, ex)
          for U, n in ((1, 7), (1, 2121), (64, 7), (64, 2121), (64, 59047), (1000, 7), (1000, 2121))
          for K in (1, 20, 128) for D in (4, 28, 112, 224) if not (D == 224 and K == 128) for ex in (False, True)]
SEED_TRIES = 8


def band_case(U, n, K, D, with_excl, seed_offset=0):
    seed = 2000 + 17 * U + n + 3 * K + D + 1000003 * seed_offset
    rng, lo, n_nodes, unids = layout(U, n, seed)
    tb = table(seed, n_nodes, D)
    exclude = to_csr(random_exclusion(rng, U, lo, n, n_nodes)) if with_excl else None
    s64, b = f64_scores(tb, unids, lo, n)
    elig = eligible_mask(U, lo, n, exclude)
    return tb, unids, lo, exclude, s64, b, elig, kth_band(s64, b, elig, K)


@pytest.fixture(scope='module')
def near_ties():
    """Per case the first of SEED_TRIES seeds whose float64 scores meet the case's cap (else the best of them), decided
    from float64 alone and before any kernel of the test runs."""
    counts, offsets = {}, {}
    for case in MATRIX:
        for off in range(SEED_TRIES):
            c = int((band_case(*case, seed_offset=off)[7][5] > 0).sum())
            if case not in counts or c < counts[case]:
                counts[case], offsets[case] = c, off
            if c <= near_tie_cap(case[3], case[2], case[1]) * case[0]:
                break
    torch.cuda.empty_cache()
    return counts, offsets


@pytest.mark.parametrize('U,n,K,D,with_excl', MATRIX,
                         ids=['%d-%d-%d-%d-%s' % (c[:4] + ('excl' if c[4] else 'all',)) for c in MATRIX])
def test_topk_against_float64(near_ties, U, n, K, D, with_excl):
    counts, offsets = near_ties
    case = (U, n, K, D, with_excl)
    tb, unids, lo, exclude, s64, b, elig, band = band_case(*case, seed_offset=offsets[case])
    near = int((band[5] > 0).sum())
    assert near == counts[case]
    assert near <= near_tie_cap(D, K, n) * U, '%d of %d users have a near-tie at the K-th place' % (near, U)
    items, scores = call_topk(tb, unids, K, lo, n, exclude)
    check_topk(items, scores, s64, b, elig, K, lo, band)


# ------------------------------------------------------------------------------------------------ 2. exact
def exact_order(s64, elig, K, lo):
    """float64 result under (score descending, id ascending): a stable ascending sort of the negated scores"""
    masked = torch.where(elig, s64, torch.full_like(s64, NINF))
    order = torch.sort(-masked, dim=1, stable=True).indices[:, :K]
    sc = masked.gather(1, order)
    items = torch.where(sc > NINF, order + lo, torch.full_like(order, -1))
    return items, sc


def pick_positives(rng, U, lo, n, rows):
    """a catalogue item per user; every fifth user's positive sits in its own exclusion list"""
    pos = rng.integers(lo, lo + n, size=U)
    for q in range(0, U, 5):
        inside = rows[q][(rows[q] >= lo) & (rows[q] < lo + n)]
        if inside.size:
            pos[q] = inside[int(rng.integers(0, inside.size))]
    return pos.astype(np.int64)


def f64_rank_counts(s64, elig, pos_idx):
    """others = eligible minus the positive; counts of others strictly above / strictly below the positive's score"""
    U = s64.shape[0]
    others = elig.clone()
    others[torch.arange(U, device=DEV), pos_idx] = False
    p = s64.gather(1, pos_idx[:, None])
    return others, p[:, 0], ((s64 > p) & others).sum(1), ((s64 < p) & others).sum(1), others.sum(1)


@pytest.mark.parametrize('U,n,D,K', [(608, 2121, 112, 20), (300, 59047, 28, 50), (64, 2121, 224, 128)])
def test_integer_tables_are_exact(U, n, D, K):
    rng, lo, n_nodes, unids = layout(U, n, 5)
    tb = table(5, n_nodes, D, integer=True)
    rows = random_exclusion(rng, U, lo, n, n_nodes)
    exclude = to_csr(rows)
    s64, _ = f64_scores(tb, unids, lo, n)
    assert bool((s64 == s64.round()).all()) and float(s64.abs().max()) < 2 ** 20
    elig = eligible_mask(U, lo, n, exclude)
    straddle = 0
    for excl in (exclude, None):
        e = elig if excl is not None else torch.ones_like(elig)
        want_items, want_sc = exact_order(s64, e, K, lo)
        items, scores = call_topk(tb, unids, K, lo, n, excl)
        assert torch.equal(items, want_items), 'items differ from the float64 order'
        assert torch.equal(scores.double(), want_sc), 'scores differ'
        masked = torch.where(e, s64, torch.full_like(s64, NINF))
        straddle += int(((masked == want_sc[:, -1:]).sum(1) > (want_sc == want_sc[:, -1:]).sum(1)).sum())
    assert straddle > 0, 'no tie group straddles the K-th place: the cut rule is not exercised'
    pos = pick_positives(rng, U, lo, n, rows)
    pos_t = torch.from_numpy(pos).to(DEV)
    for excl in (exclude, None):
        e = elig if excl is not None else torch.ones_like(elig)
        _, p, above, below, n_oth = f64_rank_counts(s64, e, pos_t - lo)
        rank, auc, ps = engine.dot_rank_full(tb, unids, pos_t, (lo, lo + n), exclude=excl)
        assert torch.equal(ps.double(), p)
        assert torch.equal(rank.long(), above), 'rank differs from the float64 count'
        assert torch.equal(torch.round(auc.double() * n_oth).long(), below), 'auc count differs'
        assert float((auc.double() - below.double() / n_oth).abs().max()) <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------ 3. same pair, same bits
@pytest.mark.parametrize('D', [28, 112])
def test_same_pair_same_bits(D):
    """Also the hardware check that the f32-input MFMA tile accumulates like the fmaf chain of the pair kernels."""
    U, n = 1000, 59047
    rng, lo, n_nodes, unids = layout(U, n, 21)
    tb = table(21, n_nodes, D)
    i50, s50 = call_topk(tb, unids, 50, lo, n)
    i5, s5 = call_topk(tb, unids, 5, lo, n)
    assert torch.equal(i5, i50[:, :5]) and torch.equal(s5, s50[:, :5]), 'K = 5 is not the prefix of K = 50'
    for q in (0, 1, 499, 999):
        i1, s1 = call_topk(tb, unids[q:q + 1], 50, lo, n)
        assert torch.equal(i1[0], i50[q]) and torch.equal(s1[0], s50[q]), 'U = 1 row differs from its U = 1000 row'
    # an exclusion list that does not touch the top 50 changes nothing
    i50c = i50.cpu().numpy()
    rows = []
    for q in range(U):
        cand = rng.integers(lo, lo + n, size=40)
        rows.append(np.unique(cand[~np.isin(cand, i50c[q])]))
    ie, se = call_topk(tb, unids, 50, lo, n, to_csr(rows))
    assert torch.equal(ie, i50) and torch.equal(se, s50)
    # a catalogue cut elsewhere: the items of the list that fall into a sub-block score the same there
    sub_lo, sub_n = lo + 1000, 30011
    isub, ssub = call_topk(tb, unids, 50, sub_lo, sub_n)
    full_in_sub = (i50 >= sub_lo) & (i50 < sub_lo + sub_n)
    for q in (0, 17, 999):
        want = s50[q][full_in_sub[q]]
        assert torch.equal(ssub[q, :want.numel()], want) and torch.equal(isub[q, :want.numel()], i50[q][full_in_sub[q]])
    # the pair kernels give the same bits
    uu = unids[:, None].expand(U, 50).reshape(-1)
    pred = engine.dot_predict(tb, uu, i50.reshape(-1)).view(U, 50)
    assert torch.equal(pred, s50), 'dot_predict differs from the scan (%d of %d scores)' % (int((pred != s50).sum()), pred.numel())
    sc, _, _, _ = engine.dot_rank_eval(tb, unids, i50)
    assert torch.equal(sc, s50), 'dot_rank_eval scores differ from the scan'
    pos = i50[:, 7].contiguous()
    _, _, ps = engine.dot_rank_full(tb, unids, pos, (lo, lo + n))
    assert torch.equal(ps, s50[:, 7])


# ------------------------------------------------------------------------------------------------ 4. sampled evaluator
def reference_loop(s64_rows):
    """The reference's per-user evaluation (solvers.py:72, 85-95) on float64 scores [U, C], column 0 the positive: sort
    descending (stable), hit vector, auc = share of negatives the positive beats, loss = -sum log sigmoid(pos - neg)."""
    ranks, aucs, losses = [], [], []
    for row in s64_rows:
        order = np.argsort(-row, kind='stable')
        ranks.append(int(np.argmax(order == 0)))
        aucs.append(float((row[0] > row[1:]).mean()))
        losses.append(float(-np.log(1.0 / (1.0 + np.exp(-(row[0] - row[1:])))).sum()))
    return np.asarray(ranks), np.asarray(aucs), np.asarray(losses)


@pytest.mark.parametrize('integer', [True, False], ids=['integer', 'real'])
def test_rank_eval_against_per_user_loop(integer):
    U, C, D = 608, 100, 112
    rng, lo, n_nodes, unids = layout(U, 2121, 31)
    tb = table(31, n_nodes, D, integer=integer)
    cand = torch.from_numpy(rng.integers(lo, lo + 2121, size=(U, C))).to(DEV)
    u, v = tb[unids].double(), tb[cand].double()
    s64 = (u[:, None, :] * v).sum(-1)
    b = gamma(D) * (u[:, None, :].abs() * v.abs()).sum(-1)
    rank64, auc64, loss64 = reference_loop(s64.cpu().numpy())
    scores, rank, auc, loss = engine.dot_rank_eval(tb, unids, cand)
    assert bool(((scores.double() - s64).abs() <= b).all()), 'score outside the fma-chain bound'
    rank_c, auc_c = rank.cpu().numpy(), auc.double().cpu().numpy()
    if integer:
        assert torch.equal(scores.double(), s64)
        np.testing.assert_array_equal(rank_c, rank64)
        np.testing.assert_allclose(auc_c, auc64, rtol=0, atol=2.0 ** -23)
        assert (np.round(auc_c * (C - 1)) == np.round(auc64 * (C - 1))).all()
    else:
        w = b[:, 1:] + b[:, :1]                                   # a negative can swap sides only inside this window
        d = s64[:, 1:] - s64[:, :1]
        r_lo, r_hi = (d > w).sum(1).cpu().numpy(), (d >= -w).sum(1).cpu().numpy()
        g_lo, g_hi = (d < -w).sum(1).cpu().numpy(), (d <= w).sum(1).cpu().numpy()
        assert ((rank_c >= r_lo) & (rank_c <= r_hi)).all(), 'rank outside its float64 interval'
        np.testing.assert_array_equal(rank_c[r_lo == r_hi], rank64[r_lo == r_hi])
        assert ((auc_c >= g_lo / (C - 1) - 1e-6) & (auc_c <= g_hi / (C - 1) + 1e-6)).all()
        assert (r_lo == r_hi).mean() > 0.9
    # loss: the fp32 torch formula on the kernel's own scores is the fp32 peer, float64 the truth
    gap = scores[:, :1] - scores[:, 1:]
    peer = -gap.sigmoid().log().sum(1).cpu().numpy()
    loss_c = loss.cpu().numpy()
    assert np.isfinite(loss64).all()
    if not integer:
        helpers.assert_fp32_close(loss_c, peer, loss64, what='eval loss')
        return
    # Integer score gaps reach hundreds.  sigmoid then log in fp32 with no clamp: exp(-gap) overflows past 88.72, so a row
    # with a gap <= -89 has loss +inf, and a row whose gaps are all >= -87 (sigmoid still a normal number) is finite and
    # is held to float64 like the real rows.  A gap of -88 lands among the denormals and is left to neither side.
    worst = gap.min(1).values.cpu().numpy()
    finite, inf = worst >= -87, worst <= -89
    assert finite.sum() >= 20 and inf.sum() >= 20, 'the table no longer gives both kinds of row'
    assert np.isposinf(loss_c[inf]).all(), 'a clamp crept in: log(sigmoid) of a gap <= -89 is -inf in fp32'
    assert np.isfinite(loss_c[finite]).all()
    helpers.assert_fp32_close(loss_c[finite], peer[finite], loss64[finite], what='eval loss, integer rows')


# ------------------------------------------------------------------------------------------------ 5. exclusion, errors
def test_all_but_m_items_excluded():
    U, n, K, D = 64, 2121, 20, 28
    rng, lo, n_nodes, unids = layout(U, n, 12)
    tb = table(12, n_nodes, D)
    s64, b = f64_scores(tb, unids, lo, n)
    keep, rows = [], []
    for q in range(U):
        m = int(rng.integers(0, K))                     # m < K eligible items, some users none at all
        k = np.sort(rng.choice(n, size=m, replace=False))
        keep.append(k)
        rows.append(np.setdiff1d(np.arange(n), k) + lo)
    items, scores = call_topk(tb, unids, K, lo, n, to_csr(rows))
    items_c, scores_c = items.cpu().numpy(), scores.cpu().numpy()
    s64c, bc = s64.cpu().numpy(), b.cpu().numpy()
    for q in range(U):
        m = len(keep[q])
        assert sorted(items_c[q, :m].tolist()) == (keep[q] + lo).tolist()
        assert (items_c[q, m:] == -1).all() and np.isneginf(scores_c[q, m:]).all()
        own = s64c[q, items_c[q, :m] - lo]
        assert (np.abs(scores_c[q, :m] - own) <= bc[q, items_c[q, :m] - lo]).all()
        assert (np.diff(scores_c[q, :m]) <= 0).all()


def test_exclusion_entries_outside_the_catalogue_are_ignored():
    U, n, K, D = 100, 2121, 20, 112
    rng, lo, n_nodes, unids = layout(U, n, 13)
    tb = table(13, n_nodes, D)
    rows = [np.unique(np.concatenate([rng.integers(0, lo, size=5), rng.integers(lo + n, n_nodes, size=5)])) for _ in range(U)]
    a = call_topk(tb, unids, K, lo, n, to_csr(rows))
    bb = call_topk(tb, unids, K, lo, n, None)
    assert torch.equal(a[0], bb[0]) and torch.equal(a[1], bb[1])
    pos = torch.from_numpy(rng.integers(lo, lo + n, size=U)).to(DEV)
    ra = engine.dot_rank_full(tb, unids, pos, (lo, lo + n), exclude=to_csr(rows))
    rb = engine.dot_rank_full(tb, unids, pos, (lo, lo + n))
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))


def test_k_larger_than_the_catalogue():
    U, n, K, D = 33, 7, 20, 28
    rng, lo, n_nodes, unids = layout(U, n, 14)
    tb = table(14, n_nodes, D)
    s64, b = f64_scores(tb, unids, lo, n)
    items, scores = call_topk(tb, unids, K, lo, n)
    assert bool((items[:, n:] == -1).all()) and bool((scores[:, n:] == NINF).all())
    assert bool((items[:, :n].sort(dim=1).values == torch.arange(lo, lo + n, device=DEV)[None, :]).all())
    assert bool(((scores[:, :n].double() - s64.gather(1, items[:, :n] - lo)).abs() <= b.gather(1, items[:, :n] - lo)).all())


def test_errors():
    U, n = 8, 100
    rng, lo, n_nodes, unids = layout(U, n, 51)
    tb = table(51, n_nodes, 28)
    pos = torch.full((U,), lo + 3, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    p = _lib.ptr
    for k in (0, 129):
        with pytest.raises(_lib.PeaError) as e:
            call_topk(tb, unids, k, lo, n)
        assert e.value.code == -1
    # a bad width: refused by the host layer, and by the library itself as an error code
    oi = torch.empty((U, 5), dtype=torch.int64, device=DEV)
    os_ = torch.empty((U, 5), dtype=torch.float32, device=DEV)
    big = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for d in (6, 260):
        bad_tb = table(51, n_nodes, d)
        for call in (lambda: call_topk(bad_tb, unids, 5, lo, n), lambda: engine.dot_predict(bad_tb, unids, unids),
                     lambda: engine.dot_rank_eval(bad_tb, unids, unids[:, None].expand(U, 2)),
                     lambda: engine.dot_rank_full(bad_tb, unids, pos, (lo, lo + n))):
            with pytest.raises(ValueError):
                call()
        assert int(lib.pea_dot_topk_workspace_bytes(U, n, 5, d)) == 0
        assert lib.pea_dot_recommend_topk(U, 5, d, n_nodes, p(bad_tb), p(unids), lo, n, None, None, p(oi), p(os_), p(big),
                                          big.numel(), _lib.current_stream()) == -1
        assert lib.pea_dot_predict(U, d, n_nodes, p(bad_tb), p(unids), p(unids), p(os_), _lib.current_stream()) == -1
        assert lib.pea_dot_rank_eval(U, 2, d, n_nodes, p(bad_tb), p(unids), p(oi), None, None, None, None,
                                     _lib.current_stream()) == -1
        assert lib.pea_dot_rank_full(U, d, n_nodes, p(bad_tb), p(unids), p(pos), lo, n, None, None, None, None, None, p(big),
                                     big.numel(), _lib.current_stream()) == -1
    bad = unids.clone()
    bad[3] = n_nodes
    with pytest.raises(IndexError):
        call_topk(tb, bad, 5, lo, n)
    with pytest.raises(IndexError):
        engine.dot_predict(tb, bad, unids)
    with pytest.raises(IndexError):
        engine.dot_rank_eval(tb, bad, unids[:, None].expand(U, 3).contiguous())
    bad[3] = -1
    with pytest.raises(IndexError):
        engine.dot_rank_full(tb, bad, pos, (lo, lo + n))
    with pytest.raises(IndexError):
        engine.dot_rank_eval(tb, unids, bad[:, None].expand(U, 3).contiguous())
    bad_pos = pos.clone()
    bad_pos[5] = n_nodes + 7
    with pytest.raises(IndexError):
        engine.dot_rank_full(tb, unids, bad_pos, (lo, lo + n))
    with pytest.raises(IndexError):
        call_topk(tb, unids, 5, n_nodes - 10, n)              # catalogue block past num_nodes
    with pytest.raises(IndexError):
        engine.dot_rank_full(tb, unids, pos, (n_nodes - 10, n_nodes - 10 + n))
    # a short workspace through the raw C call
    need = int(lib.pea_dot_topk_workspace_bytes(U, n, 5, 28))
    assert need > 0 and int(lib.pea_dot_topk_workspace_bytes(U, n, 0, 28)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def raw(ws_bytes):
        return lib.pea_dot_recommend_topk(U, 5, 28, n_nodes, p(tb), p(unids), lo, n, None, None, p(oi), p(os_), p(ws), ws_bytes,
                                          _lib.current_stream())
    assert raw(need - 1) == -4
    assert raw(need) == 0
    torch.cuda.synchronize()
    want = call_topk(tb, unids, 5, lo, n)
    assert torch.equal(oi, want[0]) and torch.equal(os_, want[1])
    rk = torch.empty(U, dtype=torch.int32, device=DEV)
    need_r = int(lib.pea_dot_topk_workspace_bytes(U, n, 1, 28))
    rc = lib.pea_dot_rank_full(U, 28, n_nodes, p(tb), p(unids), p(pos), lo, n, None, None, p(rk), None, None, p(ws), need_r - 1,
                               _lib.current_stream())
    assert rc == -4
    # the library is still usable after every refusal
    items, _ = call_topk(tb, unids, 5, lo, n)
    assert bool((items >= lo).all())
