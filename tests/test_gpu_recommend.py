"""GPU: full-catalogue top-K recommendation and all-item ranking (csrc/topk.hip) against float64.

The float64 side is torch float64 of the formula the header states, on the same fp32 inputs:
    A = repr[u] W_u^T + b1,  B = repr[i] W_i^T,  s(u, i) = relu(A + B) . w2 + b2.
Tolerance of a score: tol(s) = 1e-5 |s| + 1e-6 (the project's fp32 bound).  Two fp32 evaluations may order near-equal
scores differently, so membership at the K-th place is checked with the two-sided band t = 2 tol(s64_K) around the float64
K-th eligible score; the integer-valued tables (test 2) have no rounding at all and are compared exactly.
"""

import numpy as np
import pytest
import torch

import helpers
from graph_recsys_benchmark_amd import _lib, engine, solvers
from graph_recsys_benchmark_amd.utils import SyntheticHIN, seen_items_csr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NINF = float('-inf')


def tol(s):
    return 1e-5 * s.abs() + 1e-6


# ------------------------------------------------------------------------------------------------ inputs
class Tables:
    """repr [N, R] and the scorer's weights.  Real-valued: repr rows standard normal, fc1 / fc2 with torch.nn.Linear's
    default initialisation (unit scale keeps near-ties at the K-th place rare).  Integer-valued: every product and
    partial sum is an integer far below 2^24, so fp32 in any order equals float64 bit for bit."""

    def __init__(self, seed, n_nodes, R, integer=False):
        g = torch.Generator().manual_seed(seed)
        if integer:
            self.repr = torch.randint(-3, 4, (n_nodes, R), generator=g).float()
            self.w1 = torch.randint(-1, 2, (R, 2 * R), generator=g).float()
            self.b1 = torch.randint(-2, 3, (R,), generator=g).float()
            self.w2 = torch.randint(-2, 3, (1, R), generator=g).float()
            self.b2 = torch.randint(-2, 3, (1,), generator=g).float()
        else:
            self.repr = torch.randn(n_nodes, R, generator=g)
            torch.manual_seed(seed)
            fc1, fc2 = torch.nn.Linear(2 * R, R), torch.nn.Linear(R, 1)
            self.w1, self.b1 = fc1.weight.detach().clone(), fc1.bias.detach().clone()
            self.w2, self.b2 = fc2.weight.detach().clone(), fc2.bias.detach().clone()
        for k in ('repr', 'w1', 'b1', 'w2', 'b2'):
            setattr(self, k, getattr(self, k).to(DEV))

    @property
    def weights(self):
        return self.w1, self.b1, self.w2, self.b2


def f64_scores(repr_, unids, lo, n, w1, b1, w2, b2):
    """[U, n] float64 scores of the requested users against the catalogue [lo, lo + n)"""
    R = repr_.shape[1]
    A = repr_[unids].double() @ w1[:, :R].double().T + b1.double()
    B = repr_[lo:lo + n].double() @ w1[:, R:].double().T
    out = torch.empty((A.shape[0], n), dtype=torch.float64, device=repr_.device)
    chunk = max(1, (1 << 25) // max(n * R, 1))
    w2d, b2d = w2.double().reshape(-1), b2.double().reshape(())
    for s in range(0, A.shape[0], chunk):
        out[s:s + chunk] = torch.relu(A[s:s + chunk, None, :] + B[None, :, :]) @ w2d + b2d
    return out


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


def kth_band(s64, elig, K):
    """From float64 alone: n_elig [U], the K-th eligible score s64_K and band t (users with >= K eligible items), and
    the number of OTHER eligible items inside the band around s64_K."""
    masked = torch.where(elig, s64, torch.full_like(s64, NINF))
    n_elig = elig.sum(1)
    kk = min(K, s64.shape[1])
    top = masked.topk(kk, dim=1).values if kk > 0 else masked[:, :0]
    full = n_elig >= K
    sK = top[:, K - 1] if kk == K else torch.full((s64.shape[0],), NINF, dtype=torch.float64, device=s64.device)
    sK = torch.where(full, sK, torch.zeros_like(sK))
    t = 2.0 * tol(sK)
    in_band = (((masked - sK[:, None]).abs() <= t[:, None]) & elig).sum(1) - 1
    in_band = torch.where(full, in_band, torch.zeros_like(in_band))
    return masked, n_elig, full, sK, t, in_band


def check_topk(items, scores, s64, elig, K, lo, band):
    """every property test 1 lists, vectorised over the users"""
    masked, n_elig, full, sK, t, _ = band
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
    own = s64.gather(1, idx)
    sc = scores.double()
    err_ok = ((sc - own).abs() <= tol(own)) | ~valid
    assert bool(err_ok.all()), 'score off: worst %.3e x tol' % float((((sc - own).abs() / tol(own))[valid]).max())
    both = valid[:, 1:] & valid[:, :-1]
    ordered = (scores[:, :-1] > scores[:, 1:]) | ((scores[:, :-1] == scores[:, 1:]) & (items[:, :-1] < items[:, 1:]))
    assert bool((ordered | ~both).all()), 'list not sorted by (score descending, id ascending)'
    must = ((masked > (sK + t)[:, None]) & elig).sum(1)
    got_must = ((own > (sK + t)[:, None]) & valid).sum(1)
    assert torch.equal(must[full], got_must[full]), 'an eligible item above the band was left out'
    low = (own < (sK - t)[:, None]) & valid
    assert not bool(low[full].any()), 'an item below the band was returned'


def call_topk(tb, unids, K, lo, n, exclude=None):
    return engine.recommend_topk(tb.repr, unids, K, (lo, lo + n), *tb.weights, exclude=exclude)


def layout(U, n, seed):
    """catalogue in the middle of the node range; users drawn with repeats, in random order, from a block before it"""
    rng = np.random.default_rng(seed)
    n_users = max(U * 7 // 10, 1)
    lo = n_users + 13
    n_nodes = lo + n + 29
    unids = torch.from_numpy(rng.integers(0, n_users, size=U)).to(DEV)
    return rng, lo, n_nodes, unids


# ------------------------------------------------------------------------------------------------ 1. top-K vs float64
MATRIX = [(U, n, K, R, ex) for U in (1, 64, 1000) for n in (7, 2121, 59047) for K in (1, 20, 128) for R in (4, 16, 32, 64)
          for ex in (False, True)]


SEED_TRIES = 8


def near_tie_limit(U, n, K):
    """Largest number of users of a case that may have another eligible item inside the band around s64_K.

    K <= 20 (and K > n, where there is no K-th place): 2 % of the case's users, the figure the band test was specified
    with -- for U = 1 that is no user at all, for U = 64 one.
    K = 128 <= n: 10 %.  The 2 % cannot be met there with the inputs the test is bound to (repr standard normal,
    torch.nn.Linear's default weights).  The expected number of neighbours is the band's width over the spacing of the
    scores at the K-th place: 2 t = 6e-5 at |s| = 1.5, and at the top 0.2 % of 59,047 unit-scale scores the spacing is
    about sigma / (K z) = 0.35 / (128 x 2.9) = 1e-3, so 6 % of the users whatever the seed (float64 on the CPU, 1,000
    users x 59,047 items: R = 64 31..103 users over 32 seeds, R = 32 20..80, R = 16 14..87; at 2,121 items 19..55).  The
    cap is that expectation with room for its spread over weight draws (the walk stops at the first seed under it); a case beyond
    it would mean the inputs have degenerated (one tie group swallowing the cut), which is what the condition is there
    to catch.  For U = 1 the 10 % is again no user at all."""
    return (0.02 if K <= 20 or K > n else 0.10) * U


def band_case(U, n, K, R, with_excl, seed_offset=0):
    """inputs and float64 side of one case of the matrix (seeded by the case and the offset alone)"""
    seed = 1000 + 17 * U + n + 3 * K + R + 1000003 * seed_offset
    rng, lo, n_nodes, unids = layout(U, n, seed)
    tb = Tables(seed, n_nodes, R)
    exclude = to_csr(random_exclusion(rng, U, lo, n, n_nodes)) if with_excl else None
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights)
    elig = eligible_mask(U, lo, n, exclude)
    return tb, unids, lo, exclude, s64, elig, kth_band(s64, elig, K)


@pytest.fixture(scope='module')
def near_ties():
    """The condition that keeps the band from hiding a failure, from float64 alone and before any kernel of the test runs:
    the number of users with any OTHER eligible item inside the band around s64_K, per case of the matrix.

    Per case the seed is the first of SEED_TRIES whose float64 scores meet the case's limit (near_tie_limit), else the
    one of them with the fewest such users -- a fixed walk, decided from float64 alone: with R = 4 the count swings with
    the weights by two orders of magnitude (1..954 of 1,000 users).  Every case then ASSERTS its limit before its kernel
    runs, and the matrix as a whole asserts 2 % of all its users on top.  The users that do have a neighbour inside the
    band are still held to every property of check_topk (the band only admits either of two float64-indistinguishable
    items at the cut), and exactness at the cut itself is pinned without any band by the integer-valued tables of test 2."""
    counts, offsets = {}, {}
    for case in MATRIX:
        for off in range(SEED_TRIES):
            c = int((band_case(*case, seed_offset=off)[6][5] > 0).sum())
            if case not in counts or c < counts[case]:
                counts[case], offsets[case] = c, off
            if c <= near_tie_limit(case[0], case[1], case[2]):
                break
    torch.cuda.empty_cache()
    users = sum(c[0] for c in MATRIX)
    for case, c in counts.items():
        if c > 0.02 * case[0]:
            print('near-ties above 2 %% of the case (K = 128, limit 10 %%): U=%d n=%d K=%d R=%d excl=%s: %d users' % (case + (c,)))
    print('near-ties pooled: %d of %d users = %.2f %%' % (sum(counts.values()), users, 100.0 * sum(counts.values()) / users))
    return counts, offsets, sum(counts.values()) / users


@pytest.mark.parametrize('U,n,K,R,with_excl', MATRIX,
                         ids=['%d-%d-%d-%d-%s' % (c[:4] + ('excl' if c[4] else 'all',)) for c in MATRIX])
def test_topk_against_float64(near_ties, U, n, K, R, with_excl):
    counts, offsets, pooled = near_ties
    assert pooled <= 0.02, 'more than 2 %% of the users of the matrix have a near-tie at the K-th place'
    tb, unids, lo, exclude, s64, elig, band = band_case(U, n, K, R, with_excl, offsets[(U, n, K, R, with_excl)])
    near = int((band[5] > 0).sum())
    assert near == counts[(U, n, K, R, with_excl)]
    assert near <= near_tie_limit(U, n, K), '%d of %d users have a near-tie at the K-th place' % (near, U)
    items, scores = call_topk(tb, unids, K, lo, n, exclude)
    check_topk(items, scores, s64, elig, K, lo, band)


# ------------------------------------------------------------------------------------------------ 2. exact
def exact_order(s64, elig, K, lo):
    """float64 result under (score descending, id ascending): a stable ascending sort of the negated scores"""
    masked = torch.where(elig, s64, torch.full_like(s64, NINF))
    order = torch.sort(-masked, dim=1, stable=True).indices[:, :K]
    sc = masked.gather(1, order)
    items = torch.where(sc > NINF, order + lo, torch.full_like(order, -1))
    if order.shape[1] < K:
        pad = K - order.shape[1]
        items = torch.cat([items, torch.full((items.shape[0], pad), -1, dtype=items.dtype, device=DEV)], 1)
        sc = torch.cat([sc, torch.full((sc.shape[0], pad), NINF, dtype=sc.dtype, device=DEV)], 1)
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


@pytest.mark.parametrize('U,n', [(608, 2121), (300, 59047)])
def test_integer_tables_are_exact(U, n):
    rng, lo, n_nodes, unids = layout(U, n, 5)
    tb = Tables(5, n_nodes, 16, integer=True)
    rows = random_exclusion(rng, U, lo, n, n_nodes)
    exclude = to_csr(rows)
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights)
    assert bool((s64 == s64.round()).all()) and float(s64.abs().max()) < 2 ** 20
    elig = eligible_mask(U, lo, n, exclude)
    assert torch.unique(s64[0]).numel() < n // 4, 'scores must fall onto few integers (large tie groups)'
    for K in (1, 20, 128):
        straddle = 0
        for excl in (exclude, None):
            e = elig if excl is not None else torch.ones_like(elig)
            want_items, want_sc = exact_order(s64, e, K, lo)
            items, scores = call_topk(tb, unids, K, lo, n, excl)
            assert torch.equal(items, want_items), 'K=%d: items differ from the float64 order' % K
            assert torch.equal(scores.double(), want_sc), 'K=%d: scores differ' % K
            masked = torch.where(e, s64, torch.full_like(s64, NINF))
            straddle += int(((masked == want_sc[:, -1:]).sum(1) > (want_sc == want_sc[:, -1:]).sum(1)).sum())
        assert straddle > 0, 'no tie group straddles the K-th place: the cut rule is not exercised'
    pos = pick_positives(rng, U, lo, n, rows)
    pos_t = torch.from_numpy(pos).to(DEV)
    for excl in (exclude, None):
        e = elig if excl is not None else torch.ones_like(elig)
        _, p, above, below, n_oth = f64_rank_counts(s64, e, pos_t - lo)
        rank, auc, ps = engine.rank_full(tb.repr, unids, pos_t, (lo, lo + n), *tb.weights, exclude=excl)
        assert torch.equal(ps.double(), p)
        assert torch.equal(rank.long(), above), 'rank differs from the float64 count'
        assert torch.equal(torch.round(auc.double() * n_oth).long(), below), 'auc count differs'
        assert float((auc.double() - below.double() / n_oth).abs().max()) <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------ 3. exclusion
def test_excluding_the_float64_top_items():
    U, n, K = 200, 2121, 20
    rng, lo, n_nodes, unids = layout(U, n, 11)
    tb = Tables(11, n_nodes, 16)
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights)
    top = s64.topk(K, dim=1).indices
    rows = [np.sort(r) + lo for r in top.cpu().numpy()]
    exclude = to_csr(rows)
    items, scores = call_topk(tb, unids, K, lo, n, exclude)
    hit = (items[:, :, None] == (top + lo)[:, None, :]).any()
    assert not bool(hit), 'an excluded item was returned'
    elig = eligible_mask(U, lo, n, exclude)
    check_topk(items, scores, s64, elig, K, lo, kth_band(s64, elig, K))


def test_all_but_m_items_excluded():
    U, n, K = 64, 2121, 20
    rng, lo, n_nodes, unids = layout(U, n, 12)
    tb = Tables(12, n_nodes, 16)
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights)
    keep, rows = [], []
    for q in range(U):
        m = int(rng.integers(0, K))                     # m < K eligible items, some users none at all
        k = np.sort(rng.choice(n, size=m, replace=False))
        keep.append(k)
        rows.append(np.setdiff1d(np.arange(n), k) + lo)
    items, scores = call_topk(tb, unids, K, lo, n, to_csr(rows))
    items_c, scores_c = items.cpu().numpy(), scores.cpu().numpy()
    s64c = s64.cpu().numpy()
    for q in range(U):
        m = len(keep[q])
        assert sorted(items_c[q, :m].tolist()) == (keep[q] + lo).tolist()
        assert (items_c[q, m:] == -1).all() and np.isneginf(scores_c[q, m:]).all()
        own = s64c[q, items_c[q, :m] - lo]
        assert (np.abs(scores_c[q, :m] - own) <= 1e-5 * np.abs(own) + 1e-6).all()
        assert (np.diff(scores_c[q, :m]) <= 0).all()
        gaps = -np.diff(np.sort(s64c[q, keep[q]])[::-1])
        if m > 1 and gaps.min() > 2 * (1e-5 * np.abs(own).max() + 1e-6):      # float64 order is unambiguous: same order
            assert items_c[q, :m].tolist() == (keep[q][np.argsort(-s64c[q, keep[q]], kind='stable')] + lo).tolist()


def test_exclusion_entries_outside_the_catalogue_are_ignored():
    U, n, K = 100, 2121, 20
    rng, lo, n_nodes, unids = layout(U, n, 13)
    tb = Tables(13, n_nodes, 16)
    rows = [np.unique(np.concatenate([rng.integers(0, lo, size=5), rng.integers(lo + n, n_nodes, size=5)])) for _ in range(U)]
    a = call_topk(tb, unids, K, lo, n, to_csr(rows))
    b = call_topk(tb, unids, K, lo, n, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ 4. same pair, same bits
def test_same_pair_same_bits():
    U, n = 1000, 59047
    rng, lo, n_nodes, unids = layout(U, n, 21)
    tb = Tables(21, n_nodes, 16)
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
    i50b, s50b = call_topk(tb, unids, 50, lo, n)
    assert i50b.cpu().numpy().tobytes() == i50c.tobytes() and s50b.cpu().numpy().tobytes() == s50.cpu().numpy().tobytes()
    # and the rank entry point scores the same pairs with the same bits
    pos = i50[:, 7].contiguous()
    _, _, ps = engine.rank_full(tb.repr, unids, pos, (lo, lo + n), *tb.weights)
    assert torch.equal(ps, s50[:, 7])


# ------------------------------------------------------------------------------------------------ 5. all-item rank
@pytest.mark.parametrize('U,n', [(608, 2121), (1024, 59047)])
def test_rank_full_real_tables(U, n):
    K = 20
    rng, lo, n_nodes, unids = layout(U, n, 31)
    tb = Tables(31, n_nodes, 16)
    rows = random_exclusion(rng, U, lo, n, n_nodes)
    exclude = to_csr(rows)
    pos = pick_positives(rng, U, lo, n, rows)
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights)
    elig = eligible_mask(U, lo, n, exclude)
    # a uniformly drawn positive almost never ranks inside the top K of 59,047 items: every third user's positive is taken
    # from around the cut of its own float64 list (places 0 .. K + 9 among the eligible), so that the exact cross-check
    # against recommend_topk below has subjects on both sides of K at both sizes
    near_top = torch.where(elig, s64, torch.full_like(s64, NINF)).topk(K + 10, dim=1).indices.cpu().numpy()
    for q in range(1, U, 3):
        pos[q] = lo + near_top[q, int(rng.integers(0, K + 10))]
    pos_t = torch.from_numpy(pos).to(DEV)
    others, p64, _, _, n_oth = f64_rank_counts(s64, elig, pos_t - lo)
    t = 2.0 * tol(p64)
    r_lo = ((s64 > (p64 + t)[:, None]) & others).sum(1)
    r_hi = ((s64 >= (p64 - t)[:, None]) & others).sum(1)
    b_lo = ((s64 < (p64 - t)[:, None]) & others).sum(1)
    b_hi = ((s64 <= (p64 + t)[:, None]) & others).sum(1)
    exact_share = float((r_lo == r_hi).double().mean())
    print('rank_full %d x %d: %.1f %% of the users held to the exact rank, widest interval %d'
          % (U, n, 100 * exact_share, int((r_hi - r_lo).max())))
    if n == 2121:
        assert exact_share >= 0.9, 'the float64 intervals are too wide for this size to test anything'
    rank, auc, ps = engine.rank_full(tb.repr, unids, pos_t, (lo, lo + n), *tb.weights, exclude=exclude)
    assert bool(((ps.double() - p64).abs() <= tol(p64)).all())
    assert bool(((rank.long() >= r_lo) & (rank.long() <= r_hi)).all()), 'rank outside its float64 interval'
    a = auc.double()
    assert bool(((a >= b_lo / n_oth - 1e-6) & (a <= b_hi / n_oth + 1e-6)).all()), 'auc outside its float64 interval'
    # exactly, against recommend_topk of the same users: the positive stands where its rank says
    items, scores = call_topk(tb, unids, K, lo, n, exclude)
    pos_elig = elig.gather(1, (pos_t - lo)[:, None])[:, 0].cpu().numpy()
    items_c, scores_c, rank_c, ps_c = items.cpu().numpy(), scores.cpu().numpy(), rank.cpu().numpy(), ps.cpu().numpy()
    checked = beyond = 0
    for q in np.flatnonzero(pos_elig & (rank_c < K)):
        where = np.flatnonzero(items_c[q] == pos[q])
        assert where.size == 1, 'user %d: rank %d < K but the positive is not in the list' % (q, rank_c[q])
        j = int(where[0])
        assert scores_c[q, j].tobytes() == ps_c[q].tobytes()
        assert j >= rank_c[q]
        if (scores_c[q] == ps_c[q]).sum() == 1:
            assert j == rank_c[q]
        checked += 1
    for q in np.flatnonzero(pos_elig & (rank_c >= K)):
        assert pos[q] not in items_c[q]
        beyond += 1
    assert checked >= U // 6 and beyond > 0, 'the cross-check against the list ran on %d users' % checked


# ------------------------------------------------------------------------------------------------ 6. model level
def reference_style_metrics(scores_of, dataset, u_nids):
    """The reference's per-user evaluation loop restated with ALL of neg_unid_inid_map[u] as candidates: scores of
    [positive] + negatives sorted descending (stable), the hit vector, HR@5..20, NDCG@5..20, AUC = share of negatives the
    positive beats.  Returns per-user arrays."""
    hrs, ndcgs, aucs, ranks = [], [], [], []
    for u in u_nids:
        pos, negs = dataset.test_pos_unid_inid_map[u], dataset.neg_unid_inid_map[u]
        sp, sn = scores_of(u, pos), scores_of(u, negs)
        order = np.argsort(-np.concatenate([sp, sn]), kind='stable')
        hit = order < len(pos)
        place = int(np.argmax(hit))
        ranks.append(place)
        hrs.append([1.0 if hit[:k].any() else 0.0 for k in range(5, 21)])
        ndcgs.append([(1.0 / np.log2(place + 2)) if hit[:k].any() else 0.0 for k in range(5, 21)])
        aucs.append(float((sp[0] > sn).mean()))
    return np.asarray(hrs), np.asarray(ndcgs), np.asarray(aucs), np.asarray(ranks)


def test_model_recommend_and_full_metrics():
    ds = SyntheticHIN('ml_small', seed=2019)
    ds.eval_split()
    edges = helpers.dataset_edges(ds)
    model = helpers.build_model('gat', ds.num_nodes, edges, [2] * 9, 64, 64, 16, device=DEV)
    model.load_state_dict(helpers.random_state_dict(model, 2))
    lo = ds.type_accs['iid']
    n, K = ds.num_iids, 20
    u_nids = list(ds.test_pos_unid_inid_map.keys())
    u_t = torch.tensor(u_nids, device=DEV)
    exclude = seen_items_csr(ds.edge_index_nps['user2item'], u_t, (lo, lo + n))
    model.train()
    with pytest.raises(RuntimeError):
        model.recommend(u_t, K, (lo, lo + n), exclude=exclude)
    model.eval()
    tbl = model.cached_repr
    w = (model.fc1.weight.detach(), model.fc1.bias.detach(), model.fc2.weight.detach(), model.fc2.bias.detach())
    s64 = f64_scores(tbl, u_t, lo, n, *w)
    elig = eligible_mask(len(u_nids), lo, n, exclude)
    band = kth_band(s64, elig, K)
    assert int((band[5] > 0).sum()) <= 0.02 * len(u_nids), 'more than 2 %% of the users have a near-tie at the K-th place'
    items, scores = model.recommend(u_t, K, (lo, lo + n), exclude=exclude)
    check_topk(items, scores, s64, elig, K, lo, band)

    # metrics over all negatives: float64 per-user loop in the reference's shape against the kernel's ranks
    s64c = s64.cpu().numpy()
    row_of = {u: q for q, u in enumerate(u_nids)}
    hr64, ndcg64, auc64, rank64 = reference_style_metrics(
        lambda u, ids: s64c[row_of[u], np.asarray(ids, dtype=np.int64) - lo], ds, u_nids)
    pos = np.asarray([ds.test_pos_unid_inid_map[u][0] for u in u_nids], dtype=np.int64)
    pos_t = torch.from_numpy(pos).to(DEV)
    # the dataset's negatives are exactly the eligible others of the kernel's protocol
    others, p64, above, below, n_oth = f64_rank_counts(s64, elig, pos_t - lo)
    assert n_oth.cpu().tolist() == [len(ds.neg_unid_inid_map[u]) for u in u_nids]
    np.testing.assert_array_equal(above.cpu().numpy(), rank64)
    t = 2.0 * tol(p64)
    r_lo = ((s64 > (p64 + t)[:, None]) & others).sum(1).cpu().numpy()
    r_hi = ((s64 >= (p64 - t)[:, None]) & others).sum(1).cpu().numpy()
    ambiguous = r_lo != r_hi
    rank, auc, _ = engine.rank_full(tbl, u_t, pos_t, (lo, lo + n), *w, exclude=exclude)
    rank_c = rank.cpu().numpy()
    assert ((rank_c >= r_lo) & (rank_c <= r_hi)).all()
    np.testing.assert_array_equal(rank_c[~ambiguous], rank64[~ambiguous])
    hr, ndcg, a = solvers.metrics_full_from_dataset(model, ds)
    want_hr, want_ndcg = solvers.metrics_from_ranks(rank_c)
    np.testing.assert_array_equal(hr, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg, want_ndcg.mean(axis=0))
    slack = ambiguous.sum() / len(u_nids)               # an ambiguous user moves a mean by at most 1 / U
    assert (np.abs(hr - hr64.mean(axis=0)) <= slack + 1e-12).all()
    assert (np.abs(ndcg - ndcg64.mean(axis=0)) <= slack + 1e-12).all()
    width = ((r_hi - r_lo) / n_oth.cpu().numpy()).sum() / len(u_nids)
    assert abs(a[0] - auc64.mean()) <= width + 1e-6
    if not ambiguous.any():
        np.testing.assert_array_equal(hr, hr64.mean(axis=0))
        np.testing.assert_allclose(ndcg, ndcg64.mean(axis=0), rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 7. existing scorer
@pytest.mark.parametrize('R', [16, 32])
def test_scores_agree_with_predict(R):
    U, n, K = 64, 2121, 20
    rng, lo, n_nodes, unids = layout(U, n, 41)
    tb = Tables(41, n_nodes, R)
    items, scores = call_topk(tb, unids, K, lo, n)
    pred = engine.predict(tb.repr, unids[:, None].expand(U, K).reshape(-1), items.reshape(-1), *tb.weights).view(U, K)
    s64 = f64_scores(tb.repr, unids, lo, n, *tb.weights).gather(1, items - lo)
    assert bool(((pred.double() - scores.double()).abs() <= 2.0 * tol(s64)).all())


# ------------------------------------------------------------------------------------------------ 7b. sampled evaluator
def rank_eval_case(C, R, integer):
    """N = 700 nodes, U = 37 users (the last four-user workgroup is partial), per user C distinct candidates (column 0 the
    positive; distinct, so that no negative IS the positive), and the float64 scores of the header's formula."""
    N, U = 700, 37
    rng = np.random.default_rng(1000 * C + R)
    tb = Tables(61, N, R, integer=integer)
    unids = torch.from_numpy(rng.integers(0, N, size=U)).to(DEV)
    cand = torch.from_numpy(np.stack([rng.permutation(N)[:C] for _ in range(U)])).to(DEV)
    A = tb.repr[unids].double() @ tb.w1[:, :R].double().T + tb.b1.double()
    B = tb.repr[cand].double() @ tb.w1[:, R:].double().T
    s64 = torch.relu(A[:, None, :] + B) @ tb.w2.double().reshape(-1) + tb.b2.double().reshape(())
    return tb, unids, cand, s64


def rank_intervals(s64):
    """what tol allows: a negative can change sides of the positive only inside w = tol(negative) + tol(positive)"""
    b = tol(s64)
    w = b[:, 1:] + b[:, :1]
    d = s64[:, 1:] - s64[:, :1]
    return (d > w).sum(1), (d >= -w).sum(1), (d < -w).sum(1), (d <= w).sum(1)


def per_user_loop(s64_rows):
    """The reference's per-user evaluation (solvers.py:72, 85-95) on float64 scores [U, C], column 0 the positive: stable
    descending sort, auc = share of negatives the positive beats, loss = -sum log sigmoid(pos - neg)."""
    ranks, aucs, losses = [], [], []
    for row in s64_rows:
        ranks.append(int(np.argmax(np.argsort(-row, kind='stable') == 0)))
        aucs.append(float((row[0] > row[1:]).mean()))
        losses.append(float(-np.log(1.0 / (1.0 + np.exp(-(row[0] - row[1:])))).sum()))
    return np.asarray(ranks), np.asarray(aucs), np.asarray(losses)


# C: one negative; the reference's 1 + 99 (two wave passes); past the two register-cached id passes of the evaluator.
# R: 16 is the register path, 8 and 64 the generic one.
@pytest.mark.parametrize('C,R,integer', [(C, R, False) for C in (2, 100, 201) for R in (16, 8, 64)] + [(100, 16, True)])
def test_rank_eval_against_per_user_loop(C, R, integer):
    """engine.rank_eval against the reference's loop over users on float64 scores.  pea_rank_eval runs the multi-table
    evaluator with one table, so rank_eval_multi == rank_eval (test_gpu_ablation.py) compares the kernel with itself; this
    is the independent check of the MLP evaluator."""
    tb, unids, cand, s64 = rank_eval_case(C, R, integer)
    U = unids.shape[0]
    rank64, auc64, loss64 = per_user_loop(s64.cpu().numpy())
    scores, rank, auc, loss = engine.rank_eval(tb.repr, unids, cand, *tb.weights)
    assert scores.shape == (U, C) and rank.dtype == torch.int32
    err = (scores.double() - s64).abs()
    print('C=%d R=%d: max score error %.3g, max error / tol %.3g' % (C, R, float(err.max()), float((err / tol(s64)).max())))
    assert bool((err <= tol(s64)).all()), 'score outside tol'
    rank_c, auc_c = rank.cpu().numpy(), auc.double().cpu().numpy()
    if integer:
        assert bool((s64 == s64.round()).all()) and float(s64.abs().max()) < 2 ** 20
        assert torch.equal(scores.double(), s64)
        np.testing.assert_array_equal(rank_c, rank64)
        assert (np.round(auc_c * (C - 1)) == np.round(auc64 * (C - 1))).all(), 'auc count differs'
        np.testing.assert_allclose(auc_c, auc64, rtol=0, atol=2.0 ** -23)
    else:
        r_lo, r_hi, g_lo, g_hi = (t.cpu().numpy() for t in rank_intervals(s64))
        single = r_lo == r_hi
        print('users with a single-valued rank interval: %d of %d' % (single.sum(), U))
        assert single.mean() >= 0.9, 'the float64 scores leave too many ranks open: pick another seed'
        assert ((rank_c >= r_lo) & (rank_c <= r_hi)).all(), 'rank outside its float64 interval'
        np.testing.assert_array_equal(rank_c[single], rank64[single])
        assert ((auc_c >= g_lo / (C - 1) - 1e-6) & (auc_c <= g_hi / (C - 1) + 1e-6)).all(), 'auc outside its interval'
        np.testing.assert_allclose(auc_c[g_lo == g_hi], auc64[g_lo == g_hi], rtol=0, atol=2.0 ** -23)
    # loss: the fp32 torch formula on the kernel's own scores is the fp32 peer, float64 the truth.  sigmoid then log in
    # fp32 with no clamp: exp(-gap) overflows past 88.72, so a row with a gap <= -89 has loss +inf (integer scores reach
    # that); a row whose gaps are all >= -87 is finite.  A gap of -88 lands among the denormals and is left to neither.
    gap = scores[:, :1] - scores[:, 1:]
    peer = -gap.sigmoid().log().sum(1).cpu().numpy()
    loss_c = loss.cpu().numpy()
    worst = gap.min(1).values.cpu().numpy()
    finite, inf = worst >= -87, worst <= -89
    assert finite.all() or integer
    assert np.isposinf(loss_c[inf]).all(), 'a clamp crept in: log(sigmoid) of a gap <= -89 is -inf in fp32'
    assert finite.any() and np.isfinite(loss_c[finite]).all() and np.isfinite(loss64[finite]).all()
    helpers.assert_fp32_close(loss_c[finite], peer[finite], loss64[finite], what='eval loss')


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors():
    U, n = 8, 100
    rng, lo, n_nodes, unids = layout(U, n, 51)
    tb = Tables(51, n_nodes, 16)
    pos = torch.full((U,), lo + 3, dtype=torch.int64, device=DEV)
    for k in (0, 129):
        with pytest.raises(_lib.PeaError) as e:
            call_topk(tb, unids, k, lo, n)
        assert e.value.code == -1
    tb6 = Tables(51, n_nodes, 6)
    with pytest.raises(_lib.PeaError) as e:
        call_topk(tb6, unids, 5, lo, n)
    assert e.value.code == -1
    with pytest.raises(_lib.PeaError) as e:
        engine.rank_full(tb6.repr, unids, pos, (lo, lo + n), *tb6.weights)
    assert e.value.code == -1
    bad = unids.clone()
    bad[3] = n_nodes
    with pytest.raises(IndexError):
        call_topk(tb, bad, 5, lo, n)
    bad[3] = -1
    with pytest.raises(IndexError):
        engine.rank_full(tb.repr, bad, pos, (lo, lo + n), *tb.weights)
    bad_pos = pos.clone()
    bad_pos[5] = n_nodes + 7
    with pytest.raises(IndexError):
        engine.rank_full(tb.repr, unids, bad_pos, (lo, lo + n), *tb.weights)
    with pytest.raises(IndexError):
        call_topk(tb, unids, 5, n_nodes - 10, n)              # catalogue block past num_nodes
    with pytest.raises(IndexError):
        engine.rank_full(tb.repr, unids, pos, (n_nodes - 10, n_nodes - 10 + n), *tb.weights)
    # a short workspace through the raw C call
    lib = _lib.load()
    need = int(lib.pea_topk_workspace_bytes(U, n, 5, 16))
    assert need > 0 and int(lib.pea_topk_workspace_bytes(U, n, 0, 16)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    oi = torch.empty((U, 5), dtype=torch.int64, device=DEV)
    os_ = torch.empty((U, 5), dtype=torch.float32, device=DEV)
    p = _lib.ptr

    def raw(ws_bytes):
        return lib.pea_recommend_topk(U, 5, 16, n_nodes, p(tb.repr), p(unids), lo, n, None, None, p(tb.w1), p(tb.b1), p(tb.w2),
                                      p(tb.b2), p(oi), p(os_), p(ws), ws_bytes, _lib.current_stream())
    assert raw(need - 1) == -4
    assert raw(need) == 0
    torch.cuda.synchronize()
    want = call_topk(tb, unids, 5, lo, n)
    assert torch.equal(oi, want[0]) and torch.equal(os_, want[1])
    rk = torch.empty(U, dtype=torch.int32, device=DEV)
    need_r = int(lib.pea_topk_workspace_bytes(U, n, 1, 16))
    rc = lib.pea_rank_full(U, 16, n_nodes, p(tb.repr), p(unids), p(pos), lo, n, None, None, p(tb.w1), p(tb.b1), p(tb.w2),
                           p(tb.b2), p(rk), None, None, p(ws), need_r - 1, _lib.current_stream())
    assert rc == -4
    # the library is still usable after every refusal
    items, _ = call_topk(tb, unids, 5, lo, n)
    assert bool((items >= lo).all())


# ------------------------------------------------------------------------------------------------ 9. headline catalogue
def test_headline_catalogue():
    U, n, K = 4096, 59047, 20
    rng = np.random.default_rng(61)
    n_users = 162541
    lo, n_nodes = n_users, n_users + n + 1000
    unids = torch.from_numpy(rng.permutation(n_users)[:U]).to(DEV)
    tb = Tables(61, n_nodes, 16)
    rows = [np.unique(rng.integers(lo, lo + n, size=int(rng.integers(11, 300)))) for _ in range(U)]
    exclude = to_csr(rows)
    items, scores = call_topk(tb, unids, K, lo, n, exclude)
    items2, scores2 = call_topk(tb, unids, K, lo, n, exclude)
    assert torch.equal(items, items2) and torch.equal(scores, scores2)
    pick = torch.from_numpy(np.sort(rng.choice(U, size=64, replace=False))).to(DEV)
    sub = to_csr([rows[q] for q in pick.cpu().tolist()])
    s64 = f64_scores(tb.repr, unids[pick], lo, n, *tb.weights)
    elig = eligible_mask(64, lo, n, sub)
    band = kth_band(s64, elig, K)
    assert int((band[5] > 0).sum()) <= 0.02 * 64
    check_topk(items[pick], scores[pick], s64, elig, K, lo, band)
    pos = torch.from_numpy(rng.integers(lo, lo + n, size=U)).to(DEV)
    rank, auc, ps = engine.rank_full(tb.repr, unids, pos, (lo, lo + n), *tb.weights, exclude=exclude)
    rank2, auc2, ps2 = engine.rank_full(tb.repr, unids, pos, (lo, lo + n), *tb.weights, exclude=exclude)
    assert torch.equal(rank, rank2) and torch.equal(auc, auc2) and torch.equal(ps, ps2)
    others, p64, _, _, n_oth = f64_rank_counts(s64, elig, pos[pick] - lo)
    t = 2.0 * tol(p64)
    r_lo = ((s64 > (p64 + t)[:, None]) & others).sum(1)
    r_hi = ((s64 >= (p64 - t)[:, None]) & others).sum(1)
    r = rank[pick].long()
    assert bool(((r >= r_lo) & (r <= r_hi)).all())
