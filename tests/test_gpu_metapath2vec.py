"""GPU: the MetaPath2Vec and WalkBasedRecsysModel classes end to end on the toy graph of tests/walk_ref.py."""
import numpy as np
import pytest
import torch

import walk_ref
from helpers import assert_fp32_close

pytestmark = pytest.mark.gpu


def _model(d=64, sparse=False, native=True, seed=walk_ref.WALK_SEED):
    from graph_recsys_benchmark_amd.models import MetaPath2Vec
    hin = walk_ref.toy_hin()
    model = MetaPath2Vec({k: torch.from_numpy(v) for k, v in hin['edge_index_dict'].items()}, d, hin['metapath'], 12, 5,
                         hin['num_nodes_dict'], hin['types'], hin['type_accs'], walks_per_node=2, num_negative_samples=3,
                         sparse=sparse, native=native, seed=seed).cuda()
    with torch.no_grad():
        g = torch.Generator().manual_seed(8)
        model.embedding.weight.copy_(torch.randn(model.embedding.weight.shape, generator=g) * 0.3)
    return model, hin


def test_sample_is_the_restated_stream_in_repeat_order():
    model, hin = _model()
    batch = torch.tensor([3, 0, 39, 17])
    for call in range(2):
        pos, neg = model.sample(batch)
        starts = np.tile(batch.numpy(), 2)                                 # batch.repeat(walks_per_node)
        csrs = [walk_ref.csr_of(hin['edge_index_dict'][k], hin['num_nodes']) for k in hin['metapath']]
        want, _ = walk_ref.metapath_walks(csrs, [0, 1, 2, 3], starts, 12, walk_ref.WALK_SEED, 2 * call, hin['num_nodes'])
        np.testing.assert_array_equal(pos.cpu().numpy(), want)
        lo = [hin['type_accs'][k[-1]] for k in hin['metapath']]
        cnt = [hin['num_nodes_dict'][k[-1]] for k in hin['metapath']]
        want_neg = walk_ref.uniform_walks(lo, cnt, np.tile(batch.numpy(), 6), 12, walk_ref.WALK_SEED, 2 * call + 1)
        np.testing.assert_array_equal(neg.cpu().numpy(), want_neg)


def test_native_and_torch_models_agree():
    native, hin = _model(native=True)
    plain, _ = _model(native=False)
    pos, neg = native.sample(torch.arange(40))
    assert bool((pos < 0).any())
    l_native, l_plain = native.loss(pos, neg), plain.loss(pos, neg)
    l_native.backward()
    l_plain.backward()
    w = native.embedding.weight.detach().cpu().numpy()
    l64, g64, _ = walk_ref.skipgram_loss(w, walk_ref.windows(pos.cpu().numpy(), 5), walk_ref.windows(neg.cpu().numpy(), 5),
                                         torch.float64)
    assert_fp32_close(np.array([l_native.item()]), np.array([l_plain.item()]), l64[:1], what='loss')
    assert_fp32_close(native.embedding.weight.grad.cpu().numpy(), plain.embedding.weight.grad.cpu().numpy(), g64, what='grad')


@pytest.mark.parametrize('sparse', [True, False])
def test_training_lowers_the_held_out_loss(sparse):
    model, _ = _model(d=32, sparse=sparse)
    held_pos, held_neg = _model(seed=31)[0].sample(torch.arange(40))       # a FIXED pair of walk batches from another stream
    opt = (torch.optim.SparseAdam if sparse else torch.optim.Adam)(list(model.parameters()), lr=0.01)
    with torch.no_grad():
        before = model.loss(held_pos, held_neg).item()
    for step in range(30):
        pos, neg = model.sample(torch.arange(40))
        opt.zero_grad()
        loss = model.loss(pos, neg)
        loss.backward()
        assert model.embedding.weight.grad.is_sparse == sparse
        opt.step()
    with torch.no_grad():
        after = model.loss(held_pos, held_neg).item()
    assert np.isfinite(after) and after < before - 0.05, (before, after)


def _recsys(dim):
    from graph_recsys_benchmark_amd.models import WalkBasedRecsysModel
    g = torch.Generator().manual_seed(dim)
    table = torch.randn((75, dim), generator=g) * 0.4
    model = WalkBasedRecsysModel(embedding=table, embedding_dim=dim)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    return model.cuda(), table


def _mlp(model, table, u, i, dtype):
    sd = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    x = torch.cat([table.to(dtype)[u], table.to(dtype)[i]], dim=-1)
    h = torch.relu(x @ sd['fc1.weight'].t() + sd['fc1.bias'])
    return h @ sd['fc2.weight'].t() + sd['fc2.bias']


@pytest.mark.parametrize('dim', [64, 32, 20, 72, 18])
def test_walk_model_scores_ranks_and_trains(dim):
    model, table = _recsys(dim)
    assert model.cached_repr.is_cuda and not isinstance(model.cached_repr, torch.nn.Parameter)
    u = torch.arange(40).repeat_interleave(3)
    i = 40 + (torch.arange(120) * 7) % 30
    model.eval()
    with torch.no_grad():
        got = model.predict(u.cuda(), i.cuda()).cpu().numpy()
    assert_fp32_close(got, _mlp(model, table, u, i, torch.float32).numpy(), _mlp(model, table, u, i, torch.float64).numpy(),
                      what='predict')
    # recommend = brute-force top-k of predict, ties by id
    users = torch.tensor([0, 5, 39], device='cuda')
    items, scores = model.recommend(users, 7, (40, 70))
    with torch.no_grad():
        cat = torch.arange(40, 70, device='cuda')
        full = torch.stack([model.predict(uu.repeat(30), cat).view(-1) for uu in users])
    order = torch.sort(full, dim=1, descending=True, stable=True).indices[:, :7]
    assert torch.equal(items, cat[order])
    truth = torch.stack([_mlp(model, table, uu.cpu().repeat(30), cat.cpu(), torch.float64).view(-1) for uu in users])
    assert_fp32_close(scores.cpu().numpy(), torch.gather(full, 1, order).cpu().numpy(),
                      torch.gather(truth, 1, order.cpu()).numpy(), what='recommend scores')      # two kernels, two summation orders
    # the BPR loss of the driver and where its gradients go
    model.train()
    batch = torch.stack([u[:60], i[:60], 40 + (i[:60] - 40 + 11) % 30], dim=1).cuda()
    loss = model.loss(batch)
    loss.backward()
    want = -(_mlp(model, table, batch[:, 0].cpu(), batch[:, 1].cpu(), torch.float64) -
             _mlp(model, table, batch[:, 0].cpu(), batch[:, 2].cpu(), torch.float64)).sigmoid().log().sum()
    np.testing.assert_allclose(loss.item(), want.item(), rtol=2e-5)
    assert sorted(n for n, p in model.named_parameters() if p.grad is not None) == ['fc1.bias', 'fc1.weight', 'fc2.bias', 'fc2.weight']
    assert model.cached_repr.grad is None and not model.cached_repr.requires_grad


def test_walk_model_takes_the_hip_scorer_where_it_fits_and_torch_elsewhere():
    """the HIP scorer takes a width that is a multiple of 4 and at most 64 (so 20 too); 18 and 72 stay on torch"""
    from graph_recsys_benchmark_amd import engine
    calls = []
    real = engine.predict
    engine.predict = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        for dim, want in ((64, 1), (32, 1), (20, 1), (18, 0), (72, 0)):
            model, _ = _recsys(dim)
            model.eval()
            del calls[:]
            with torch.no_grad():
                model.predict(torch.tensor([0], device='cuda'), torch.tensor([41], device='cuda'))
            assert len(calls) == want, dim
    finally:
        engine.predict = real


class _EvalData:
    """what solvers.metrics reads of a dataset: one held-out positive and a pool of negatives per test user"""

    def __init__(self):
        rng = np.random.default_rng(3)
        self.test_pos_unid_inid_map = {u: [40 + int(rng.integers(0, 30))] for u in range(0, 40, 3)}
        self.neg_unid_inid_map = {u: [i for i in range(40, 70) if i != p[0]][::2] for u, p in self.test_pos_unid_inid_map.items()}


@pytest.mark.parametrize('dim', [64, 72, 18])
def test_walk_model_evaluators_at_every_width(dim):
    """rank_eval / rank_full and the solvers' metrics / metrics_full on top of them, HIP (64) or torch (72, 18), against the
    ranks, aucs and losses worked out in numpy from the model's own pair scores"""
    from graph_recsys_benchmark_amd import solvers
    model, table = _recsys(dim)
    model.eval()
    rng = np.random.default_rng(dim)
    users = torch.arange(0, 40, 3, device='cuda')
    cand = torch.from_numpy(40 + rng.integers(0, 30, size=(users.numel(), 12))).cuda()
    scores, rank, auc, loss = model.rank_eval(users, cand)
    with torch.no_grad():
        want = model.predict(users.repeat_interleave(12), cand.reshape(-1)).view(-1, 12).double().cpu().numpy()
    truth = _mlp(model, table, users.cpu().repeat_interleave(12), cand.cpu().reshape(-1), torch.float64).view(-1, 12).numpy()
    assert_fp32_close(scores.cpu().numpy(), want, truth, what='scores')
    got = scores.double().cpu().numpy()
    assert rank.dtype == torch.int32 and rank.cpu().tolist() == (got[:, 1:] > got[:, :1]).sum(1).tolist()
    np.testing.assert_allclose(auc.cpu().numpy(), (got[:, 1:] < got[:, :1]).sum(1) / 11.0, rtol=1e-6)
    np.testing.assert_allclose(loss.cpu().numpy(), np.log1p(np.exp(-(got[:, :1] - got[:, 1:]))).sum(1), rtol=1e-4)
    # all-item ranks: the user's first three catalogue items excluded
    pos_items = cand[:, 0].contiguous()
    rowptr = torch.arange(0, 3 * users.numel() + 1, 3, device='cuda')
    excl = torch.tensor([40, 41, 42], device='cuda').repeat(users.numel())
    frank, fauc, fpos = model.rank_full(users, pos_items, (40, 70), exclude=(rowptr, excl))
    with torch.no_grad():
        cat = torch.arange(40, 70, device='cuda')
        full = model.predict(users.repeat_interleave(30), cat.repeat(users.numel())).view(-1, 30).double().cpu().numpy()
    pos_np = pos_items.cpu().numpy()
    ok = np.ones_like(full, dtype=bool)
    ok[:, :3] = False
    ok[np.arange(users.numel()), pos_np - 40] = False
    ps = full[np.arange(users.numel()), pos_np - 40][:, None]
    np.testing.assert_allclose(fpos.cpu().numpy(), ps[:, 0], rtol=1e-4, atol=1e-5)
    margin = np.abs(full - ps)[ok].min()
    if margin > 1e-4:                      # no eligible item within rounding of the positive: the ranks are determined
        assert frank.cpu().tolist() == ((full > ps) & ok).sum(1).tolist()
        np.testing.assert_allclose(fauc.cpu().numpy(), ((full < ps) & ok).sum(1) / ok.sum(1), rtol=1e-6)
    # the solvers' entry points run on either path
    data = _EvalData()
    np.random.seed(0)
    hr, ndcg, auc1, loss1 = solvers.metrics(model, data, num_neg_candidates=9)
    assert hr.shape == (16,) and ndcg.shape == (16,) and 0.0 <= auc1[0] <= 1.0 and np.isfinite(loss1[0])
    u_nids = list(data.test_pos_unid_inid_map)
    hr2, ndcg2, auc2 = solvers.metrics_full(model, u_nids, [data.test_pos_unid_inid_map[u][0] for u in u_nids], (40, 70))
    assert hr2.shape == (16,) and 0.0 <= auc2[0] <= 1.0 and (np.diff(hr2) >= 0).all()


def _int_recsys(dim):
    """a Walk model of small integers: table in {-2..2}, fc weights and biases in {-1, 0, 1}.  Every score is an integer below
    2^24, exact in fp32 whatever the blocking or the summation order: HIP and torch routes agree to the bit"""
    from graph_recsys_benchmark_amd.models import WalkBasedRecsysModel
    g = torch.Generator().manual_seed(100 + dim)
    table = torch.randint(-2, 3, (75, dim), generator=g).float()
    model = WalkBasedRecsysModel(embedding=table, embedding_dim=dim)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    return model.cuda().eval()


@pytest.mark.parametrize('dim', [64, 72])
def test_walk_model_ranks_several_positives_in_one_scan(dim):
    """rank_full_multi, on the HIP scorer (64) or the torch composition (72), against the flattened route over the model's own
    rank_full: all four outputs, and solvers.metrics_full_multi on top of the hook"""
    from graph_recsys_benchmark_amd import solvers
    model = _int_recsys(dim)
    assert model._hip_scorer() == (dim == 64)
    rng = np.random.default_rng(dim)
    u_nids = np.arange(0, 39, 3)
    assert u_nids.size == 13
    lists = [np.sort(rng.choice(np.arange(40, 70), size=1 + q % 4, replace=False)) for q in range(13)]
    pos_rowptr = torch.tensor(np.cumsum([0] + [len(r) for r in lists]), device='cuda')
    pos_items = torch.tensor(np.concatenate(lists), device='cuda')
    exclude = (torch.arange(0, 3 * 13 + 1, 3, device='cuda'),
               torch.tensor(np.concatenate([np.sort(rng.choice(np.arange(40, 70), size=3, replace=False)) for _ in range(13)]), device='cuda'))
    model.USER_CHUNK, model.POS_CHUNK = 5, 3                 # the torch route: several blocks of users and of positives
    got = model.rank_full_multi(torch.as_tensor(u_nids, device='cuda'), pos_rowptr, pos_items, (40, 70), exclude=exclude)
    want = solvers.rank_full_multi_flattened(model.rank_full, u_nids, pos_rowptr.cpu().numpy(), pos_items.cpu().numpy(), (40, 70),
                                             exclude, device='cuda')
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.int32]
    for g, w, what in zip(got, want, ('above', 'below', 'pos_score', 'n_neg')):
        assert np.array_equal(g.cpu().numpy(), w), what
    assert got[0].sum() > 0 and got[1].sum() > 0
    # metrics_full_multi takes the hook, once, and no longer flattens
    calls, hook = [], model.rank_full_multi
    model.rank_full_multi = lambda *a, **kw: calls.append(1) or hook(*a, **kw)
    try:
        metrics = solvers.metrics_full_multi(model, u_nids, (pos_rowptr, pos_items), (40, 70), exclude=exclude)
    finally:
        del model.rank_full_multi
    assert calls == [1]
    per_user = solvers.multi_metrics_from_counts(want[0], want[2], want[1], pos_rowptr.cpu().numpy(), want[3])
    assert sorted(metrics) == sorted(solvers.MULTI_METRICS)
    for name, v in per_user.items():
        np.testing.assert_array_equal(metrics[name], v.mean(axis=0), err_msg=name)
    if dim == 72:                                            # the torch recommend: all but 2 items excluded, k = 7
        left = [47, 62]
        rows = (torch.tensor([0, 28], device='cuda'), torch.tensor([i for i in range(40, 70) if i not in left], device='cuda'))
        user = torch.tensor([6], device='cuda')
        items, scores = model.recommend(user, 7, (40, 70), exclude=rows)
        with torch.no_grad():
            s = model.predict(user.repeat(2), torch.tensor(left, device='cuda')).view(-1).tolist()
        assert items.shape == scores.shape == (1, 7)
        assert items[0, :2].tolist() == sorted(left, key=lambda i: (-s[left.index(i)], i))
        assert scores[0, :2].tolist() == sorted(s, reverse=True)
        assert (items[0, 2:] == -1).all() and (scores[0, 2:] == float('-inf')).all()
