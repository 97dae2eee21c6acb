"""GPU: the all-item evaluation with several positives per user (include/peahip_eval.h: engine.rank_full_multi on the fc1 / fc2
scorer, engine.dot_rank_full_multi on the inner product), on the smallest shapes that reach every branch.

  integer inputs   every score is exact in float32 and ties are plentiful: above / below / n_neg equal a float64 brute force
                   over the definition, pos_score is exact
  random floats    above / pos_score / n_neg equal the flattened route (one rank_full call per positive, the user's other
                   positives excluded too: for the inner product the same kernels with one row per flat pair), below through
                   the bits of its auc; and above / below lie inside the intervals the float64 scores leave them
  one positive     engine.rank_full (a scan of its own) and engine.dot_rank_full (the several-positives body without a row
                   pointer): exact on integer inputs against the same brute force, each of their three outputs may be NULL in
                   the C call, and the inner product's thread-per-user finish for very many users equals its wave-per-user one
Rows of one call mix 0, 1, PC - 1, PC, PC + 1, 2 PC + 1 and 40 positives per user (PC = the thresholds of one scan row), positives
outside the catalogue and inside the exclusion row, exclusion entries outside the catalogue, a user without negatives, an empty
exclusion row and repeated users."""
import numpy as np
import pytest
import torch

import helpers
from graph_recsys_benchmark_amd import _lib, engine, solvers
from graph_recsys_benchmark_amd.utils import SyntheticHIN, positives_csr, seen_items_csr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
PC = _lib.RANK_MULTI_CHUNK
COUNTS = [0, 1, PC - 1, PC, PC + 1, 2 * PC + 1, 40]
N_USER_NODES, TAIL = 70, 30          # node ids: [0, 70) users, then the catalogue, then 30 more nodes


# ------------------------------------------------------------------------------------------------ inputs
class Scorer:
    """a table [N, W] and, for the 'mlp' form, the fc weights; integer: every product and partial sum an integer far below 2^24"""

    def __init__(self, form, seed, n_nodes, width, integer):
        g = torch.Generator().manual_seed(seed)
        self.form, self.fc = form, ()
        if integer:
            self.repr = torch.randint(-3, 4, (n_nodes, width), generator=g).float().to(DEV)
            if form == 'mlp':
                self.fc = tuple(torch.randint(-1, 2, s, generator=g).float().to(DEV)
                                for s in ((width, 2 * width), (width,), (1, width), (1,)))
        else:
            self.repr = torch.randn(n_nodes, width, generator=g).to(DEV)
            if form == 'mlp':
                torch.manual_seed(seed)
                fc1, fc2 = torch.nn.Linear(2 * width, width), torch.nn.Linear(width, 1)
                self.fc = tuple(t.detach().clone().to(DEV) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))

    def multi(self, unids, rowptr, items, item_range, exclude=None, table=None):
        fn = engine.rank_full_multi if self.form == 'mlp' else engine.dot_rank_full_multi
        return fn(self.repr if table is None else table, unids, rowptr, items, item_range, *self.fc, exclude=exclude)

    def single(self, unids, pos, item_range, exclude=None):
        fn = engine.rank_full if self.form == 'mlp' else engine.dot_rank_full
        return fn(self.repr, unids, pos, item_range, *self.fc, exclude=exclude)

    def f64_scores(self, unids):
        """[U, N] float64 scores of the requested users against EVERY node (a positive may lie outside the catalogue)"""
        x = self.repr.double()
        if self.form == 'dot':
            return x[unids] @ x.T
        w1, b1, w2, b2 = (t.double() for t in self.fc)
        r = x.shape[1]
        a, b = x[unids] @ w1[:, :r].T + b1, x @ w1[:, r:].T
        return torch.relu(a[:, None, :] + b[None, :, :]) @ w2.reshape(-1) + b2.reshape(())


def to_csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(items.astype(np.int64)).to(DEV)


def make_rows(seed, U, n):
    """(unids, positive rows, exclusion rows) of a call over the catalogue [70, 70 + n): the positive counts cycle through COUNTS
    from a seed-dependent start; users repeat; see the module docstring for the row forms"""
    rng = np.random.default_rng(seed)
    lo, n_nodes = N_USER_NODES, N_USER_NODES + n + TAIL
    outside = np.concatenate([np.arange(0, lo), np.arange(lo + n, n_nodes)])
    unids = rng.integers(0, lo, size=U)
    if U > 2:
        unids[2] = unids[0]                                            # a repeated user with another positive row
    pos_rows, excl_rows = [], []
    for q in range(U):
        p = COUNTS[(q + seed) % len(COUNTS)]
        k_in = int(rng.integers(0, min(p, n) + 1))
        k_in = max(k_in, p - outside.size)
        inside = lo + rng.choice(n, size=k_in, replace=False)
        pos = np.sort(np.concatenate([inside, rng.choice(outside, size=p - k_in, replace=False)])).astype(np.int64)
        c = int(rng.integers(0, n // 2 + 1))
        ex = [lo + rng.choice(n, size=c, replace=False), rng.choice(outside, size=2, replace=False)]   # two entries outside the catalogue
        if pos.size:
            ex.append(pos[:(pos.size + 1) // 2])                       # positives inside the exclusion row
        ex = np.unique(np.concatenate(ex)).astype(np.int64)
        if q % 5 == 1:
            ex = np.zeros(0, np.int64)                                 # an empty exclusion row
        if q % 7 == 3:                                                 # no negative left: everything excluded or positive
            ex = np.setdiff1d(np.arange(lo, lo + n), pos[::2]).astype(np.int64)
        pos_rows.append(pos)
        excl_rows.append(ex)
    return unids.astype(np.int64), pos_rows, excl_rows, (lo, lo + n), n_nodes


def brute_force(s64, pos_rows, excl_rows, item_range):
    """the definition of include/peahip_eval.h on float64 scores [U, N]"""
    lo, hi = item_range
    above, below, ps, n_neg = [], [], [], []
    s64 = s64.cpu().numpy()
    for q, (pos, ex) in enumerate(zip(pos_rows, excl_rows)):
        neg = np.ones(hi - lo, dtype=bool)
        for ids in (pos, ex):
            ids = np.asarray(ids, dtype=np.int64)
            ids = ids[(ids >= lo) & (ids < hi)]
            neg[ids - lo] = False
        sn = s64[q, lo:hi][neg]
        n_neg.append(int(neg.sum()))
        for p in pos:
            above.append(int((sn > s64[q, p]).sum())); below.append(int((sn < s64[q, p]).sum())); ps.append(s64[q, p])
    return (torch.tensor(above, dtype=torch.int32), torch.tensor(below, dtype=torch.int32), torch.tensor(ps, dtype=torch.float64),
            torch.tensor(n_neg, dtype=torch.int32))


def tol(s):
    """tests/test_gpu_recommend.py: what a float32 score may be away from the float64 one"""
    return 1e-5 * np.abs(s) + 1e-6


def f64_intervals(s64, pos_rows, excl_rows, item_range):
    """per (user, positive) in flat order, from float64 scores [U, N] alone: (r_lo, r_hi, b_lo, b_hi), the bounds of above and
    below once every negative within 2 tol of the positive's score may fall on either side (test_rank_full_real_tables)"""
    lo, hi = item_range
    s64 = s64.cpu().numpy()
    out = []
    for q, (pos, ex) in enumerate(zip(pos_rows, excl_rows)):
        neg = np.ones(hi - lo, dtype=bool)
        for ids in (pos, ex):
            ids = np.asarray(ids, dtype=np.int64)
            neg[ids[(ids >= lo) & (ids < hi)] - lo] = False
        sn = s64[q, lo:hi][neg]
        for p in pos:
            p64 = s64[q, p]
            t = 2.0 * tol(p64)
            out.append((int((sn > p64 + t).sum()), int((sn >= p64 - t).sum()), int((sn < p64 - t).sum()), int((sn <= p64 + t).sum())))
    return np.asarray(out, dtype=np.int64).reshape(-1, 4).T


def flattened(sc, unids, pos_rows, excl_rows, item_range):
    """the identity of include/peahip_eval.h, spelled out on the single-positive entry point: (rank, auc, pos_score) of one call
    over the Q (user, positive) pairs, each with the union of the user's exclusion row and positive row excluded"""
    flat_u, flat_p, unions = [], [], []
    for q, (pos, ex) in enumerate(zip(pos_rows, excl_rows)):
        un = np.union1d(pos, ex).astype(np.int64)
        for p in pos:
            flat_u.append(unids[q]); flat_p.append(p); unions.append(un)
    if not flat_u:
        return (torch.zeros(0, dtype=torch.int32), torch.zeros(0), torch.zeros(0))
    u_t, p_t = torch.tensor(flat_u, device=DEV), torch.tensor(flat_p, device=DEV)
    return tuple(t.cpu() for t in sc.single(u_t, p_t, item_range, exclude=to_csr(unions)))


# (U, catalogue items, width): every catalogue size and user count of the issue, every padded width class of either scorer
DOT_CASES = [(1, 1, 4), (17, 31, 20), (33, 32, 64), (129, 33, 128), (17, 129, 256), (129, 129, 20), (1, 129, 64), (33, 1, 128),
             (3, 1536, 112)]
MLP_CASES = [(1, 1, 4), (17, 31, 16), (33, 32, 32), (129, 33, 64), (17, 129, 64), (129, 129, 16), (1, 129, 32), (33, 1, 4),
             (3, 1536, 16)]
CASES = [('dot',) + c for c in DOT_CASES] + [('mlp',) + c for c in MLP_CASES]


def case(form, U, n, width, integer):
    seed = 7 * U + n + width
    unids, pos_rows, excl_rows, item_range, n_nodes = make_rows(seed, U, n)
    sc = Scorer(form, seed, n_nodes, width, integer)
    u_t = torch.from_numpy(unids).to(DEV)
    rowptr, items = to_csr(pos_rows)
    return sc, unids, u_t, pos_rows, excl_rows, item_range, rowptr, items


def test_the_cases_reach_every_row_form():
    seen = set()
    for form, U, n, width in CASES:
        unids, pos_rows, excl_rows, (lo, hi), _ = make_rows(7 * U + n + width, U, n)
        seen |= {len(p) for p in pos_rows}
        if U >= 17:
            assert any(((p < lo) | (p >= hi)).any() for p in pos_rows if len(p))
            assert any(np.intersect1d(p, e).size for p, e in zip(pos_rows, excl_rows))
            assert any(len(e) == 0 for e in excl_rows) and len(set(unids.tolist())) < U
    assert seen == set(COUNTS)
    # the inner product's workspace holds nothing that grows with the catalogue but one set of counters per item range: the
    # (3, 1536) case is cut in more than one range
    lib = _lib.load()
    assert lib.pea_dot_rank_multi_workspace_bytes(3, 34, 1536, 112) > lib.pea_dot_rank_multi_workspace_bytes(3, 34, 511, 112)


@pytest.mark.parametrize('form,U,n,width', CASES)
def test_integer_inputs_are_exact(form, U, n, width):
    sc, unids, u_t, pos_rows, excl_rows, item_range, rowptr, items = case(form, U, n, width, integer=True)
    want = brute_force(sc.f64_scores(u_t), pos_rows, excl_rows, item_range)
    got = sc.multi(u_t, rowptr, items, item_range, exclude=to_csr(excl_rows))
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.int32]
    for name, g, w in zip(('above', 'below', 'pos_score', 'n_neg'), got, want):
        assert torch.equal(g.cpu() if name != 'pos_score' else g.cpu().double(), w), name
    if U >= 17:
        assert int((want[3] == 0).sum()) > 0, 'no user without negatives in this case'
    # exclude=None: the positives alone leave the negatives
    want = brute_force(sc.f64_scores(u_t), pos_rows, [[]] * U, item_range)
    got = sc.multi(u_t, rowptr, items, item_range)
    for name, g, w in zip(('above', 'below', 'pos_score', 'n_neg'), got, want):
        assert torch.equal(g.cpu() if name != 'pos_score' else g.cpu().double(), w), name + ' without exclusion'
    # an exclusion list that holds nothing is no exclusion
    for g, e in zip(got, sc.multi(u_t, rowptr, items, item_range, exclude=to_csr([[]] * U))):
        assert torch.equal(g, e)


@pytest.mark.parametrize('form,U,n,width', CASES)
def test_random_floats_equal_the_flattened_route(form, U, n, width):
    sc, unids, u_t, pos_rows, excl_rows, item_range, rowptr, items = case(form, U, n, width, integer=False)
    exclude = to_csr(excl_rows)
    above, below, pos_score, n_neg = (t.cpu() for t in sc.multi(u_t, rowptr, items, item_range, exclude=exclude))
    rank, auc, ps = flattened(sc, unids, pos_rows, excl_rows, item_range)
    assert torch.equal(above, rank) and torch.equal(pos_score, ps)
    # a yardstick that is none of the kernels: the float64 scores hold most pairs to one rank and every pair to an interval
    r_lo, r_hi, b_lo, b_hi = f64_intervals(sc.f64_scores(u_t), pos_rows, excl_rows, item_range)
    assert r_lo.size == 0 or (r_lo == r_hi).mean() >= 0.9, 'the float64 intervals are too wide for this case to test anything'
    assert np.all((above.numpy() >= r_lo) & (above.numpy() <= r_hi)), 'above outside its float64 interval'
    assert np.all((below.numpy() >= b_lo) & (below.numpy() <= b_hi)), 'below outside its float64 interval'
    flat_q = torch.repeat_interleave(torch.arange(U), rowptr.cpu()[1:] - rowptr.cpu()[:-1])
    others = n_neg[flat_q]
    want_auc = torch.where(others > 0, below.float() / others.float(), torch.zeros(()))
    assert torch.equal(auc, want_auc)                                   # the bits of (float)below / (float)n_neg
    lo, hi = item_range
    for q in range(U):
        un = np.union1d(pos_rows[q], excl_rows[q])
        assert int(n_neg[q]) == (hi - lo) - int(((un >= lo) & (un < hi)).sum())
    # the helper solvers keeps for models with a rank_full of their own gives the same integers
    h = solvers.rank_full_multi_flattened(lambda *a, **k: sc.single(*a, **k), unids, rowptr.cpu().numpy(), items.cpu().numpy(),
                                          item_range, exclude, device=DEV)
    assert np.array_equal(h[0], above.numpy()) and np.array_equal(h[1], below.numpy())
    assert np.array_equal(h[2], pos_score.numpy()) and np.array_equal(h[3], n_neg.numpy())
    # and a second run has the same bits
    again = sc.multi(u_t, rowptr, items, item_range, exclude=exclude)
    for a, b in zip((above, below, pos_score, n_neg), again):
        assert torch.equal(a, b.cpu())


def one_positive_per_user(seed, pos_rows, item_range):
    """the first positive of every row of make_rows; a user whose row is empty gets an arbitrary node"""
    rng = np.random.default_rng(seed)
    return np.asarray([p[0] if len(p) else rng.integers(0, item_range[1] + TAIL) for p in pos_rows], dtype=np.int64)


def single_positive_rows(pos_rows, excl_rows):
    """the exclusion rows of make_rows for a call that keeps one positive per user: the user make_rows leaves without negatives
    (q % 7 == 3: everything excluded or positive) has its other positives excluded too, so that it still has none"""
    return [np.union1d(ex, pos[1:]).astype(np.int64) if q % 7 == 3 else ex for q, (pos, ex) in enumerate(zip(pos_rows, excl_rows))]


@pytest.mark.parametrize('form,U,n,width', CASES)
def test_single_positive_entry_points_are_exact(form, U, n, width):
    sc, unids, u_t, pos_rows, excl_rows, item_range, _, _ = case(form, U, n, width, integer=True)
    pos = one_positive_per_user(U + n, pos_rows, item_range)
    excl_rows = single_positive_rows(pos_rows, excl_rows)
    lo, hi = item_range
    if U >= 17:
        assert ((pos < lo) | (pos >= hi)).any() and any(p in e for p, e in zip(pos, excl_rows))
    s64 = sc.f64_scores(u_t)
    for rows in (excl_rows, None):
        above, below, ps, n_neg = brute_force(s64, [[p] for p in pos], rows if rows is not None else [[]] * U, item_range)
        rank, auc, pos_score = sc.single(u_t, torch.from_numpy(pos).to(DEV), item_range, exclude=to_csr(rows) if rows is not None else None)
        assert [t.dtype for t in (rank, auc, pos_score)] == [torch.int32, torch.float32, torch.float32]
        what = 'with exclusion' if rows is not None else 'without exclusion'
        assert torch.equal(rank.cpu(), above), what
        want_auc = torch.where(n_neg > 0, below.float() / n_neg.float(), torch.zeros(()))   # the bits of (float)below / (float)n_neg
        assert torch.equal(auc.cpu(), want_auc), what
        assert torch.equal(pos_score.cpu().double(), ps), what
        if rows is not None and U > 3:
            assert int((n_neg == 0).sum()) > 0 and bool((auc.cpu()[n_neg == 0] == 0).all()), 'no user without negatives in this case'


def test_single_positive_finish_by_threads_equals_the_finish_by_waves(form='dot', width=20):
    """engine.dot_rank_full over at least _lib.RANK_THREAD_FINISH_USERS users scores its positives and finishes by one thread per
    user, a smaller call by one wave per user: the call at the threshold has the bytes of its two halves, which are below it, and
    on integer inputs its first users have the counts of the float64 brute force"""
    U, n = _lib.RANK_THREAD_FINISH_USERS, 33
    lo, n_nodes = N_USER_NODES, N_USER_NODES + n + TAIL
    sc = Scorer(form, 11, n_nodes, width, integer=False)
    g = torch.Generator(device=DEV).manual_seed(11)
    u_t = torch.randint(0, lo, (U,), device=DEV, generator=g)
    pos = torch.randint(0, n_nodes, (U,), device=DEV, generator=g)            # inside and outside the catalogue
    mask = torch.rand((U, n + 1), device=DEV, generator=g) < 0.3             # column 0: node 0, an entry outside the catalogue
    mask[torch.arange(0, U, 5, device=DEV)] = False                           # empty rows
    mask[torch.arange(3, U, 7, device=DEV), 1:] = True                        # nothing left but (perhaps) the positive
    rowptr = torch.zeros(U + 1, dtype=torch.int64, device=DEV)
    rowptr[1:] = torch.cumsum(mask.sum(1), 0)
    col = mask.nonzero()[:, 1]                                                # row-major: every row ascends
    items = torch.where(col == 0, torch.zeros_like(col), lo + col - 1)
    whole = sc.single(u_t, pos, (lo, lo + n), exclude=(rowptr, items))
    assert int((whole[1] == 0).sum()) > 0 and int((whole[0] > 0).sum()) > 0
    h = U // 2
    for part, cut in ((slice(0, h), (0, h)), (slice(h, U), (h, U))):
        e0 = int(rowptr[cut[0]])
        ex = ((rowptr[cut[0]:cut[1] + 1] - e0).contiguous(), items[e0:int(rowptr[cut[1]])].contiguous())
        half = sc.single(u_t[part].contiguous(), pos[part].contiguous(), (lo, lo + n), exclude=ex)
        for w, got in zip(whole, half):
            assert torch.equal(w[part], got)
    for w, got in zip(sc.single(u_t, pos, (lo, lo + n)), (torch.cat(t) for t in zip(sc.single(u_t[:h].contiguous(), pos[:h].contiguous(), (lo, lo + n)),
                                                                                   sc.single(u_t[h:].contiguous(), pos[h:].contiguous(), (lo, lo + n))))):
        assert torch.equal(w, got)
    # a yardstick that is neither finish: integer tables, the first 70 users (empty rows, rows that leave nothing, positives
    # outside the catalogue among them) against the definition
    sci = Scorer(form, 12, n_nodes, width, integer=True)
    rank, auc, pos_score = (t[:70].cpu() for t in sci.single(u_t, pos, (lo, lo + n), exclude=(rowptr, items)))
    ptr, flat = rowptr[:71].cpu().numpy(), items[:int(rowptr[70])].cpu().numpy()
    rows = [flat[ptr[q]:ptr[q + 1]] for q in range(70)]
    above, below, ps, n_neg = brute_force(sci.f64_scores(u_t[:70]), [[int(p)] for p in pos[:70].cpu()], rows, (lo, lo + n))
    assert int((n_neg == 0).sum()) > 0 and int((above > 0).sum()) > 0
    assert torch.equal(rank, above) and torch.equal(pos_score.double(), ps)
    assert torch.equal(auc, torch.where(n_neg > 0, below.float() / n_neg.float(), torch.zeros(())))


@pytest.mark.parametrize('form,width', [('dot', 20), ('mlp', 16)])
def test_single_positive_outputs_may_be_null(form, width):
    """the raw C entry points at (U, n) = (33, 129): each of rank, auc and pos_score NULL in turn leaves the other two as the
    all-three call writes them"""
    sc, unids, u_t, pos_rows, excl_rows, item_range, _, _ = case(form, 33, 129, width, integer=False)
    pos = torch.from_numpy(one_positive_per_user(33 + 129, pos_rows, item_range)).to(DEV)
    exclude = to_csr(excl_rows)
    lib, p = _lib.load(), _lib.ptr
    (lo, hi), (n_nodes, w) = item_range, sc.repr.shape
    query = lib.pea_topk_workspace_bytes if form == 'mlp' else lib.pea_dot_topk_workspace_bytes
    need = int(query(33, hi - lo, 1, w))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    fn = lib.pea_rank_full if form == 'mlp' else lib.pea_dot_rank_full

    def call(skip):
        outs = [torch.full((33,), -7, dtype=torch.int32, device=DEV), torch.full((33,), -7.0, device=DEV), torch.full((33,), -7.0, device=DEV)]
        rc = fn(33, w, n_nodes, p(sc.repr), p(u_t), p(pos), lo, hi - lo, p(exclude[0]), p(exclude[1]), *[p(t) for t in sc.fc],
                *[None if i == skip else p(t) for i, t in enumerate(outs)], p(ws), need, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == 0
        return [t.cpu() for t in outs]

    full = call(None)
    for g, e in zip(full, sc.single(u_t, pos, item_range, exclude=exclude)):
        assert torch.equal(g, e.cpu())
    for skip in range(3):
        got = call(skip)
        for i in range(3):
            if i == skip:
                assert bool((got[i] == -7).all()), 'an output that was not asked for was written'
            else:
                assert got[i].numpy().tobytes() == full[i].numpy().tobytes()


@pytest.mark.parametrize('form,width', [('dot', 20), ('mlp', 16)])
def test_no_positives_at_all_and_no_users(form, width):
    sc, unids, u_t, pos_rows, excl_rows, item_range, _, _ = case(form, 17, 33, width, integer=True)
    rowptr, items = to_csr([[]] * 17)
    above, below, pos_score, n_neg = sc.multi(u_t, rowptr, items, item_range, exclude=to_csr(excl_rows))
    assert above.numel() == below.numel() == pos_score.numel() == 0
    want = brute_force(sc.f64_scores(u_t), [[]] * 17, excl_rows, item_range)
    assert torch.equal(n_neg.cpu(), want[3])
    none = sc.multi(u_t[:0], rowptr[:1], items, item_range)
    assert all(t.numel() == 0 for t in none)


@pytest.mark.parametrize('form,width', [('dot', 20), ('mlp', 16)])
def test_non_contiguous_table(form, width):
    sc, unids, u_t, pos_rows, excl_rows, item_range, rowptr, items = case(form, 33, 129, width, integer=False)
    wide = torch.zeros((sc.repr.shape[0], width + 12), device=DEV)
    wide[:, 4:4 + width] = sc.repr
    view = wide[:, 4:4 + width]
    assert not view.is_contiguous()
    exclude = to_csr(excl_rows)
    for a, b in zip(sc.multi(u_t, rowptr, items, item_range, exclude=exclude),
                    sc.multi(u_t, rowptr, items, item_range, exclude=exclude, table=view)):
        assert torch.equal(a, b)


def raw_call(sc, u_t, rowptr, items, item_range, exclude):
    """the C entry point itself: the return code AND the outputs of a call that reports an id out of range"""
    lib, p = _lib.load(), _lib.ptr
    U, Q, (lo, hi) = u_t.numel(), items.numel(), item_range
    n_nodes, w = sc.repr.shape
    above, below = (torch.full((Q,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    ps, n_neg = torch.empty(Q, device=DEV), torch.empty(U, dtype=torch.int32, device=DEV)
    query = lib.pea_rank_multi_workspace_bytes if sc.form == 'mlp' else lib.pea_dot_rank_multi_workspace_bytes
    need = query(U, Q, hi - lo, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    head = (U, w, n_nodes, p(sc.repr), p(u_t), p(rowptr), p(items), Q, lo, hi - lo, p(exclude[0]), p(exclude[1]))
    tail = (p(above), p(below), p(ps), p(n_neg), p(ws), need, _lib.current_stream())
    fn = lib.pea_rank_full_multi if sc.form == 'mlp' else lib.pea_dot_rank_full_multi
    rc = fn(*head, *[p(t) for t in sc.fc], *tail)
    torch.cuda.synchronize()
    return rc, (above.cpu(), below.cpu(), ps.cpu(), n_neg.cpu())


@pytest.mark.parametrize('form,width', [('dot', 20), ('mlp', 16)])
@pytest.mark.parametrize('what', ['user', 'positive'])
def test_an_id_out_of_range_is_reported_and_spoils_nobody_else(form, width, what):
    sc, unids, u_t, pos_rows, excl_rows, item_range, rowptr, items = case(form, 33, 129, width, integer=False)
    exclude = to_csr(excl_rows)
    good = [t.cpu() for t in sc.multi(u_t, rowptr, items, item_range, exclude=exclude)]
    n_nodes = sc.repr.shape[0]
    victim = next(q for q in range(33) if len(pos_rows[q]) == PC + 1)
    bad_u, bad_items = u_t.clone(), items.clone()
    b, e = int(rowptr[victim]), int(rowptr[victim + 1])
    if what == 'user':
        bad_u[victim] = n_nodes + 5
    else:
        bad_items[e - 1] = n_nodes + 5                      # the row's last entry: it still ascends
    with pytest.raises(IndexError):
        sc.multi(bad_u, rowptr, bad_items, item_range, exclude=exclude)
    engine.check_pending_errors()
    rc, out = raw_call(sc, bad_u, rowptr, bad_items, item_range, exclude)
    assert rc == -2
    keep = torch.ones(items.numel(), dtype=torch.bool)
    keep[b:e] = False
    users = torch.ones(33, dtype=torch.bool)
    users[victim] = False
    for g, o in zip(good[:3], out[:3]):
        assert torch.equal(g[keep], o[keep])
    assert torch.equal(good[3][users], out[3][users])
    # and the library is as good as before
    for g, o in zip(good, sc.multi(u_t, rowptr, items, item_range, exclude=exclude)):
        assert torch.equal(g, o.cpu())


# ------------------------------------------------------------------------------------------------ end to end
def three_positive_split(ds, num_users, seed=5):
    """test_pos_unid_inid_map with three unseen items per user"""
    rng = np.random.default_rng(seed)
    u2i = ds.edge_index_nps['user2item'].astype(np.int64)
    u0, i0 = ds.type_accs['uid'], ds.type_accs['iid']
    ds.test_pos_unid_inid_map = {}
    for u in range(u0, u0 + num_users):
        unseen = np.setdiff1d(np.arange(i0, i0 + ds.num_iids), u2i[1][u2i[0] == u])
        ds.test_pos_unid_inid_map[u] = [int(v) for v in rng.choice(unseen, size=3, replace=False)]       # in drawn order, unsorted
    return ds


def brute_metrics(pos, neg):
    """the metrics from the merged list itself (a stable descending sort of [pos || neg]), and whether the float32 scores
    leave the order in no doubt"""
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    p = pos.size
    both = np.concatenate([pos, neg])
    gaps = np.abs(both[None, :] - pos[:, None])
    gaps[np.arange(p), np.arange(p)] = np.inf
    hit = np.argsort(-both, kind='stable') < p
    places = np.flatnonzero(hit)
    ks = range(5, 21)
    out = {'HR': np.array([float(hit[:k].any()) for k in ks]),
           'NDCG_ref': np.array([hit[:k].sum() / np.log2(np.argmax(hit[:k]) + 2) for k in ks]),
           'Recall': np.array([hit[:k].sum() / p for k in ks]), 'Precision': np.array([hit[:k].sum() / k for k in ks]),
           'NDCG': np.array([sum(1.0 / np.log2(i + 2) for i in range(k) if hit[i]) / sum(1.0 / np.log2(i + 2) for i in range(min(p, k)))
                             for k in ks]),
           'MRR': 1.0 / (places[0] + 1.0), 'AP': np.mean([hit[:i + 1].sum() / (i + 1.0) for i in places]),
           'AUC': float((pos[:, None] > neg[None, :]).mean())}
    return out, gaps.min() > 1e-4 * max(1.0, np.abs(both).max())


def check_end_to_end(model, ds):
    lo, n = ds.type_accs['iid'], ds.num_iids
    u2i = ds.edge_index_nps['user2item'].astype(np.int64)
    got = solvers.metrics_full_multi_from_dataset(model, ds)
    per_user, sure = [], []
    cat = torch.arange(lo, lo + n, device=DEV)
    for u, pos in ds.test_pos_unid_inid_map.items():
        with torch.no_grad():
            s = model.predict(torch.full((n,), u, device=DEV), cat).reshape(-1).cpu().numpy()
        neg = np.ones(n, dtype=bool)
        neg[u2i[1][u2i[0] == u] - lo] = False
        neg[np.asarray(pos) - lo] = False
        m, ok = brute_metrics(s[np.sort(pos) - lo], s[neg])      # row order is ascending node id (positives_csr)
        per_user.append(m); sure.append(ok)
    sure = np.asarray(sure)
    assert sure.mean() >= 0.9, 'the float32 order is in doubt for too many users to test anything'
    assert sorted(got) == sorted(solvers.MULTI_METRICS)
    for name in solvers.MULTI_METRICS:
        want = np.mean([m[name] for m in per_user], axis=0)
        top = 3.0 if name == 'NDCG_ref' else 1.0                 # a user in doubt moves a mean by at most its range / U
        assert np.all(np.abs(got[name] - want) <= top * (~sure).sum() / len(sure) + 1e-9), name
    return got


def test_end_to_end_pea_model():
    ds = three_positive_split(SyntheticHIN('ml_small', seed=2019, scale=0.1), 40)
    model = helpers.build_model('gat', ds.num_nodes, helpers.dataset_edges(ds), [2] * 9, 64, 64, 16, device=DEV)
    model.load_state_dict(helpers.random_state_dict(model, 2))
    model.eval()
    got = check_end_to_end(model, ds)
    # the native route and the flattened route on the model's scorer give the same dict
    u_nids = list(ds.test_pos_unid_inid_map)
    u_t = torch.tensor(u_nids, device=DEV)
    item_range = (ds.type_accs['iid'], ds.type_accs['iid'] + ds.num_iids)
    exclude = seen_items_csr(ds.edge_index_nps['user2item'], u_t, item_range)
    rowptr, items = positives_csr([ds.test_pos_unid_inid_map[u] for u in u_nids], u_t)
    fl = solvers.rank_full_multi_flattened(lambda *a, **k: type(model).scored(model, 'rank_full', *a, **k), u_nids,
                                           rowptr.cpu().numpy(), items.cpu().numpy(), item_range, exclude, device=DEV)
    per_user = solvers.multi_metrics_from_counts(fl[0], fl[2], fl[1], rowptr.cpu().numpy(), fl[3])
    for name in solvers.MULTI_METRICS:
        assert np.array_equal(got[name], per_user[name].mean(axis=0)), name


def test_end_to_end_dot_model():
    from graph_recsys_benchmark_amd.models import NGCFRecsysModel
    ds = three_positive_split(SyntheticHIN('ml_small', seed=2019, scale=0.1), 40)
    u2i = torch.from_numpy(ds.edge_index_nps['user2item'].astype(np.int64)).to(DEV)
    edge_index = torch.cat([u2i, torch.flip(u2i, dims=[0])], dim=1).contiguous()

    class Model(NGCFRecsysModel):
        def update_graph_input(self, dataset):
            return edge_index

    torch.manual_seed(1)
    model = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0, entity_aware=False, entity_aware_coff=0.0,
                  if_use_features=False).to(DEV)
    model.eval()
    assert model.scorer == 'dot'
    check_end_to_end(model, ds)


class _RankFullAlone:
    """what solvers.metrics_full_multi reads of a model with a rank_full of its own and no rank_full_multi: here the Walk model's
    rank_full without its other hooks"""

    def __init__(self, model):
        self.cached_repr, self.rank_full = model.cached_repr, model.rank_full


def test_a_model_with_rank_full_alone_goes_through_the_flattened_route():
    from graph_recsys_benchmark_amd.models import WalkBasedRecsysModel
    g = torch.Generator().manual_seed(64)
    table = torch.randn((75, 64), generator=g) * 0.4
    model = WalkBasedRecsysModel(embedding=table, embedding_dim=64)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    model = model.cuda().eval()
    walk, model = model, _RankFullAlone(model)
    assert hasattr(model, 'rank_full') and not hasattr(model, 'rank_full_multi')
    rng = np.random.default_rng(2)
    u_nids = list(range(0, 40, 3))
    lists = [sorted(rng.choice(np.arange(40, 70), size=int(k), replace=False).tolist()) for k in rng.integers(1, 6, len(u_nids))]
    u_t = torch.tensor(u_nids, device=DEV)
    exclude = (torch.arange(0, 2 * len(u_nids) + 1, 2, device=DEV), torch.tensor([40, 41], device=DEV).repeat(len(u_nids)))
    calls = []
    real = model.rank_full
    model.rank_full = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    got = solvers.metrics_full_multi(model, u_nids, lists, (40, 70), exclude)
    assert calls == [1]
    # the same table through the native route of an 'mlp' model: the very same counts
    rowptr, items = positives_csr(lists, u_t)
    nat = engine.rank_full_multi(walk.cached_repr, u_t, rowptr, items, (40, 70), walk.fc1.weight, walk.fc1.bias,
                                 walk.fc2.weight, walk.fc2.bias, exclude=exclude)
    a, b, ps, nn = (t.cpu().numpy() for t in nat)
    per_user = solvers.multi_metrics_from_counts(a, ps, b, rowptr.cpu().numpy(), nn)
    for name in solvers.MULTI_METRICS:
        assert np.array_equal(got[name], per_user[name].mean(axis=0)), name
    # the Walk model itself has the hook: one scan, no call of its rank_full, the same numbers
    del calls[:]
    walk.rank_full = model.rank_full
    own = solvers.metrics_full_multi(walk, u_nids, lists, (40, 70), exclude)
    assert hasattr(walk, 'rank_full_multi') and calls == []
    for name in solvers.MULTI_METRICS:
        assert np.array_equal(own[name], got[name]), name
