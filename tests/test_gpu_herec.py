"""GPU: the HeRec kernels (csrc/herec.hip) and HeRecRecsysModel on them, against the float64 restatement (tests/herec_ref.py)
with the fp32 torch composition on the same GPU as peer, and against the reference fixture (tests/golden/herec_small.npz).
Batch sizes 1 / 15 / 16 / 17 sit around the 16-pair tile, 1000 is many tiles on many workgroups, and 5000 is 313 tiles on the
grid's 256 workgroups: more than one tile per workgroup."""
import os

import numpy as np
import pytest
import torch

import helpers
import herec_ref
import walk_ref
from graph_recsys_benchmark_amd import engine, solvers
from graph_recsys_benchmark_amd.models import HeRecRecsysModel, MetaPath2Vec
from graph_recsys_benchmark_amd.utils import seen_items_csr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(4, 1), (20, 3), (64, 2), (64, 4), (128, 1)]
BATCHES = [1, 15, 16, 17, 1000, 5000]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'herec_small.npz')
DENSE = ('d_user_emb', 'd_item_emb', 'd_user_rk_bias', 'd_item_rk_bias')

_cache = {}


def inputs(d, m, b, **kw):
    key = (d, m, b, tuple(sorted(kw.items())))
    if key not in _cache:
        inp = herec_ref.make_inputs(d, m, b, **kw)
        _cache[key] = (inp, herec_ref.run(inp, torch.float64, 'cpu'), herec_ref.run(inp, torch.float32, DEV))
    return _cache[key]


def on_gpu(inp):
    out = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    out['tables'] = [t.to(DEV) for t in inp['tables']]
    return out


def raw(g, need_grad=True, **over):
    a = dict(g, **over)
    return engine.herec_train_raw(a['tables'], a['w'], a['b'], a['user_emb'], a['item_emb'], a['user_rk_bias'], a['item_rk_bias'],
                                  a['acc_uids'], a['acc_iids'], a['unids'], a['inids'], a['labels'], need_grad=need_grad)


def native(g):
    """engine.herec_mse_loss + backward(): (loss, {name: dense gradient}) as numpy"""
    p = {k: g[k].clone().requires_grad_(True) for k in herec_ref.KEYS}
    loss = engine.herec_mse_loss(g['tables'], p['w'], p['b'], p['user_emb'], p['item_emb'], p['user_rk_bias'], p['item_rk_bias'],
                                 g['acc_uids'], g['acc_iids'], g['unids'], g['inids'], g['labels'])
    loss.backward()
    return loss.detach().cpu().numpy().reshape(1), {'d_' + k: p[k].grad.cpu().numpy() for k in herec_ref.KEYS}


def check(got, peer, truth, keys, what):
    for k in keys:
        helpers.assert_fp32_close(np.asarray(got[k]).reshape(peer[k].shape), peer[k], truth[k], what='%s %s' % (what, k))


def exact_inputs(d, m, b):
    """E, W, b zero: s_m = 0.5 and S = M / 2 exactly; embedding tables in {-1, 0, 1}: every partial sum of pred is an exact
    multiple of 0.5, so pred equals the float64 value whatever the order.  CPU tensors, and pred in float64"""
    inp = dict(herec_ref.make_inputs(d, m, b))
    gen = torch.Generator().manual_seed(d + m + b)
    for k in ('user_emb', 'item_emb', 'user_rk_bias', 'item_rk_bias'):
        inp[k] = torch.randint(-1, 2, inp[k].shape, generator=gen).float()
    inp['tables'] = [torch.zeros_like(t) for t in inp['tables']]
    inp['w'], inp['b'] = torch.zeros_like(inp['w']), torch.zeros_like(inp['b'])
    lu, li = inp['unids'] - inp['acc_uids'], inp['inids'] - inp['acc_iids']
    want = ((inp['user_emb'][lu].double() * inp['item_emb'][li].double()).sum(-1) + 0.5 * m * inp['user_rk_bias'][lu].double().sum(-1) +
            0.5 * m * inp['item_rk_bias'][li].double().sum(-1))
    return inp, want


def check_exact(d, m, b):
    inp, want = exact_inputs(d, m, b)
    g = on_gpu(inp)
    want = want.to(DEV)
    engine.check_pending_errors()
    for need_grad in (False, True):
        out = raw(g, need_grad)
        assert torch.equal(out[1].double(), want), need_grad
        assert int(out[6]) == 0
        want_loss = ((want - g['labels'].double()) ** 2).sum() / b
        assert abs(float(out[0]) - float(want_loss)) <= 1e-5 * float(want_loss) + 1e-6


@pytest.mark.parametrize('b', BATCHES)
@pytest.mark.parametrize('d,m', SHAPES)
def test_exact_case(d, m, b):
    check_exact(d, m, b)


def check_loss_and_gradients(d, m, b):
    inp, truth, peer = inputs(d, m, b)
    g = on_gpu(inp)
    engine.check_pending_errors()
    loss, grads = native(g)
    first = raw(g)
    assert int(first[6]) == 0
    got = dict(grads, loss=loss, pred=first[1].cpu().numpy(), g_user=first[4].cpu().numpy(), g_item=first[5].cpu().numpy())
    one = {k: np.asarray(v).reshape(-1) if k == 'loss' else v for k, v in peer.items()}
    two = {k: np.asarray(v).reshape(-1) if k == 'loss' else v for k, v in truth.items()}
    check(got, one, two, ('loss', 'pred', 'd_w', 'd_b') + DENSE + ('g_user', 'g_item'), '(%d, %d, %d)' % (d, m, b))
    # the raw launch gives the same dW / db the autograd function hands on
    assert np.array_equal(first[2].cpu().numpy(), grads['d_w']) and np.array_equal(first[3].cpu().numpy(), grads['d_b'])
    # rows of users and items outside the batch are exactly zero
    lu = np.unique((inp['unids'] - inp['acc_uids']).numpy())
    li = np.unique((inp['inids'] - inp['acc_iids']).numpy())
    for k, used in (('d_user_emb', lu), ('d_user_rk_bias', lu), ('d_item_emb', li), ('d_item_rk_bias', li)):
        rest = np.ones(grads[k].shape[0], dtype=bool)
        rest[used] = False
        assert not grads[k][rest].any(), k
        assert grads[k][used].any(), k
    # identical calls give identical bytes
    second = raw(g)
    for x, y in zip(first[:6], second[:6]):
        assert torch.equal(x, y)
    loss2, grads2 = native(g)
    assert np.array_equal(loss, loss2) and all(np.array_equal(grads[k], grads2[k]) for k in grads)


@pytest.mark.parametrize('b', BATCHES)
@pytest.mark.parametrize('d,m', SHAPES)
def test_loss_and_gradients(d, m, b):
    check_loss_and_gradients(d, m, b)


def test_forward_only_matches_and_does_no_backward():
    inp, truth, peer = inputs(64, 2, 1000)
    g = on_gpu(inp)
    full, fwd = raw(g), raw(g, need_grad=False)
    assert torch.equal(full[0], fwd[0]) and torch.equal(full[1], fwd[1]) and fwd[2] is None and fwd[5] is None
    with torch.no_grad():
        loss = engine.herec_mse_loss(g['tables'], g['w'].requires_grad_(True), g['b'], g['user_emb'], g['item_emb'],
                                     g['user_rk_bias'], g['item_rk_bias'], g['acc_uids'], g['acc_iids'], g['unids'], g['inids'],
                                     g['labels'])
    assert not loss.requires_grad and torch.equal(loss, full[0])


def test_strided_tables_and_another_block_layout():
    """tables that are column blocks of one wider buffer (row stride 2 D + 4) give the bytes of contiguous ones; users and
    items behind leading other nodes, with a gap between the blocks"""
    inp, truth, peer = inputs(20, 2, 100, lead=7, gap=5, seed=3)
    g = on_gpu(inp)
    wide = torch.zeros((inp['num_nodes'], 44), device=DEV)
    wide[:, :20], wide[:, 24:] = g['tables'][0], g['tables'][1]
    a, b = raw(g), raw(g, tables=[wide[:, :20], wide[:, 24:]])
    assert wide[:, 24:].stride(0) == 44 and all(torch.equal(x, y) for x, y in zip(a[:6], b[:6]))
    loss, grads = native(g)
    got = dict(grads, loss=loss, pred=a[1].cpu().numpy())
    one = dict(peer, loss=peer['loss'].reshape(1))
    two = dict(truth, loss=truth['loss'].reshape(1))
    check(got, one, two, ('loss', 'pred', 'd_w', 'd_b') + DENSE, 'lead / gap')
    t1 = engine.herec_table(g['tables'], g['w'], g['b'], g['user_emb'], g['item_emb'], g['user_rk_bias'], g['item_rk_bias'], 7, 162)
    t2 = engine.herec_table([wide[:, :20], wide[:, 24:]], g['w'], g['b'], g['user_emb'], g['item_emb'], g['user_rk_bias'],
                            g['item_rk_bias'], 7, 162)
    assert torch.equal(t1, t2)
    helpers.assert_fp32_close(t1.cpu().numpy(), herec_ref.table_of(inp, torch.float32, DEV), herec_ref.table_of(inp), what='table')
    other = np.r_[0:7, 157:162, 462:inp['num_nodes']]
    assert not t1.cpu().numpy()[other].any()


def test_fixture():
    z = dict(np.load(GOLDEN))
    inp = herec_ref.golden_inputs(z)
    truth = herec_ref.run(inp, torch.float64)
    g = on_gpu(inp)
    loss, grads = native(g)
    pred = raw(g, need_grad=False)[1].cpu().numpy()
    helpers.assert_fp32_close(loss, z['loss'].reshape(1), truth['loss'].reshape(1), what='loss')
    helpers.assert_fp32_close(pred, z['pred'], truth['pred'], what='pred')
    for k, name in zip(DENSE, ('user_emb', 'item_emb', 'user_rk_bias', 'item_rk_bias')):
        helpers.assert_fp32_close(grads[k], z['grad.%s.weight' % name], truth[k], what=k)
    for m in range(3):
        helpers.assert_fp32_close(grads['d_w'][m], z['grad.emb_trans.%d.weight' % m], truth['d_w'][m], what='dW %d' % m)
        helpers.assert_fp32_close(grads['d_b'][m], z['grad.emb_trans.%d.bias' % m], truth['d_b'][m], what='db %d' % m)


def test_bad_ids_are_dropped_and_reported():
    """one user id that lies in the item block and one item id >= N: the range check, not a device fault -- nothing is read
    through either id"""
    inp, _, _ = inputs(20, 3, 50)
    bad = dict(inp, unids=inp['unids'].clone(), inids=inp['inids'].clone())
    bad['unids'][3] = inp['acc_iids'] + 11
    bad['inids'][7] = inp['num_nodes'] + 5
    keep = torch.ones(50, dtype=torch.bool)
    keep[[3, 7]] = False
    rest = dict(inp, unids=inp['unids'][keep], inids=inp['inids'][keep], labels=inp['labels'][keep])
    truth, peer = herec_ref.run(rest, torch.float64, 'cpu', divide_by=50), herec_ref.run(rest, torch.float32, DEV, divide_by=50)
    engine.check_pending_errors()
    g = on_gpu(bad)
    out = raw(g)
    assert int(out[6]) == 1
    for rows in (out[4], out[5]):
        assert not rows[[3, 7]].any() and rows[keep.to(DEV)].any()
    assert not out[1][[3, 7]].any()
    helpers.assert_fp32_close(out[1][keep.to(DEV)].cpu().numpy(), peer['pred'], truth['pred'], what='pred')
    loss, grads = native(g)
    got = dict(grads, loss=loss)
    check(got, dict(peer, loss=peer['loss'].reshape(1)), dict(truth, loss=truth['loss'].reshape(1)), ('loss', 'd_w', 'd_b') + DENSE,
          'bad ids')
    with pytest.raises(IndexError):
        engine.check_pending_errors()
    engine.check_pending_errors()          # the flag was consumed


def model_of(inp, native=True):
    d = inp['w'].shape[1]
    model = HeRecRecsysModel(embeddings=inp['tables'], num_uids=inp['user_emb'].shape[0], num_iids=inp['item_emb'].shape[0],
                             acc_uids=inp['acc_uids'], acc_iids=inp['acc_iids'], embedding_dim=d, native=native)
    return herec_ref.load_model(model, inp).to(DEV)


def check_table(inp, g):
    """the catalogue table against the float32 peer and the float64 truth, and its structure; returns it"""
    d = inp['w'].shape[1]
    table = engine.herec_table(g['tables'], g['w'], g['b'], g['user_emb'], g['item_emb'], g['user_rk_bias'], g['item_rk_bias'],
                               inp['acc_uids'], inp['acc_iids'])
    assert tuple(table.shape) == (inp['num_nodes'], d + 4)
    helpers.assert_fp32_close(table.cpu().numpy(), herec_ref.table_of(inp, torch.float32, DEV), herec_ref.table_of(inp), what='table')
    nu, ni = inp['user_emb'].shape[0], inp['item_emb'].shape[0]
    u0, i0 = inp['acc_uids'], inp['acc_iids']
    other = torch.ones(inp['num_nodes'], dtype=torch.bool, device=DEV)
    other[u0:u0 + nu] = False
    other[i0:i0 + ni] = False
    assert not table[other].any() and not table[:, d + 2:].any()
    assert bool((table[u0:u0 + nu, d] == 1).all()) and bool((table[i0:i0 + ni, d + 1] == 1).all())
    assert torch.equal(table[u0:u0 + nu, :d], g['user_emb']) and torch.equal(table[i0:i0 + ni, :d], g['item_emb'])
    return table


@pytest.mark.parametrize('d,m', SHAPES)
def test_table_and_scoring(d, m):
    inp, truth, peer = inputs(d, m, 1000)
    g = on_gpu(inp)
    table = check_table(inp, g)
    model = model_of(inp).eval()
    assert torch.equal(model.cached_repr, table) and all(t.is_cuda for t in model.rk_embeddings)
    got = model.predict(g['unids'], g['inids'])
    assert torch.equal(got, engine.dot_predict(model.cached_repr, g['unids'], g['inids'])) and not got.requires_grad
    helpers.assert_fp32_close(got.cpu().numpy(), peer['pred'], truth['pred'], what='predict')
    off = model_of(inp, native=False).eval()          # the torch-built table scores alike
    helpers.assert_fp32_close(off.cached_repr.cpu().numpy(), table.cpu().numpy(), herec_ref.table_of(inp), what='torch table')
    model.train()
    helpers.assert_fp32_close(model.predict(g['unids'], g['inids']).detach().cpu().numpy(), peer['pred'], truth['pred'],
                              what='training-mode predict')


class TinyRatings:
    """the users and items of make_inputs with random interactions: one held-out positive per user, every unseen item a negative"""

    def __init__(self, inp, seed=5):
        rng = np.random.default_rng(seed)
        self.num_uids, self.num_iids = inp['user_emb'].shape[0], inp['item_emb'].shape[0]
        lo = inp['acc_iids']
        self.type_accs = {'uid': inp['acc_uids'], 'iid': lo}
        self.num_nodes = inp['num_nodes']
        flat = rng.choice(self.num_uids * self.num_iids, size=12 * self.num_uids, replace=False)
        flat = np.union1d(flat, np.arange(self.num_uids) * self.num_iids + rng.integers(0, self.num_iids, self.num_uids))
        u2i = np.stack([inp['acc_uids'] + flat // self.num_iids, lo + flat % self.num_iids]).astype(np.int64)
        self.test_pos_unid_inid_map, self.neg_unid_inid_map = {}, {}
        keep = np.ones(u2i.shape[1], dtype=bool)
        for u in range(inp['acc_uids'], inp['acc_uids'] + self.num_uids):
            mine = np.flatnonzero(u2i[0] == u)
            keep[mine[0]] = False
            self.test_pos_unid_inid_map[u] = [int(u2i[1, mine[0]])]
            seen = set(u2i[1, mine].tolist())
            self.neg_unid_inid_map[u] = [i for i in range(lo, lo + self.num_iids) if i not in seen]
        self.edge_index_nps = {'user2item': u2i[:, keep]}

    def __getitem__(self, key):
        return getattr(self, key)


def test_ranking_and_metrics():
    inp, _, _ = inputs(64, 2, 1000)
    ds = TinyRatings(inp)
    model = model_of(inp)
    lo, n, K = inp['acc_iids'], inp['item_emb'].shape[0], 20
    u_nids = list(ds.test_pos_unid_inid_map.keys())
    u_t = torch.tensor(u_nids, device=DEV)
    exclude = seen_items_csr(ds.edge_index_nps['user2item'], u_t, (lo, lo + n))
    model.train()
    with pytest.raises(RuntimeError):
        model.recommend(u_t, K, (lo, lo + n), exclude=exclude)
    model.eval()
    items, scores = model.recommend(u_t, K, (lo, lo + n), exclude=exclude)
    ref_items, ref_scores = engine.dot_recommend_topk(model.cached_repr, u_t, K, (lo, lo + n), exclude=exclude)
    assert torch.equal(items, ref_items) and torch.equal(scores, ref_scores)
    assert bool(((items >= lo) & (items < lo + n)).all())
    elig = torch.ones((len(u_nids), n), dtype=torch.bool, device=DEV)
    rows = torch.repeat_interleave(torch.arange(len(u_nids), device=DEV), exclude[0][1:] - exclude[0][:-1])
    elig[rows, exclude[1] - lo] = False
    assert bool(elig.gather(1, items - lo).all()), 'an excluded item was recommended'
    assert torch.equal(scores.reshape(-1), model.predict(u_t.repeat_interleave(K), items.reshape(-1)))
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())

    # metrics: ranks and auc from dot_rank_eval on the same draw, the eval loss in the MSE form
    np.random.seed(11)
    hr, ndcg, auc, loss = solvers.metrics(model, ds)
    np.random.seed(11)
    cand = torch.from_numpy(solvers._draw_candidates(ds, u_nids, 99)).to(DEV)
    sc, rank, a, _ = engine.dot_rank_eval(model.cached_repr, u_t, cand)
    want_hr, want_ndcg = solvers.metrics_from_ranks(rank.cpu().numpy())
    np.testing.assert_array_equal(hr, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg, want_ndcg.mean(axis=0))
    assert abs(auc[0] - float(a.double().mean())) <= 1e-12
    label = torch.zeros_like(sc)
    label[:, 0] = 1
    want = float(((sc.double() - label.double()) ** 2).mean(dim=1).mean())
    assert abs(loss[0] - want) <= 1e-5 * want
    with torch.no_grad():          # the per-user form of the reference: loss() on rows (u, pos, neg)
        batch = torch.stack([u_t[:1].expand(99), cand[0, :1].expand(99), cand[0, 1:]], dim=1)
        one = float(model.loss(batch))
    assert abs(one - float(((sc[0].double() - label[0].double()) ** 2).mean())) <= 1e-5 * one

    # metrics_full: the inherited 'dot' route
    pos = np.asarray([ds.test_pos_unid_inid_map[u][0] for u in u_nids], dtype=np.int64)
    hr_f, ndcg_f, auc_f = solvers.metrics_full(model, u_nids, pos, (lo, lo + n), exclude=exclude)
    rank_f, a_f, _ = engine.dot_rank_full(model.cached_repr, u_t, torch.from_numpy(pos).to(DEV), (lo, lo + n), exclude=exclude)
    want_hr, want_ndcg = solvers.metrics_from_ranks(rank_f.cpu().numpy())
    np.testing.assert_array_equal(hr_f, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg_f, want_ndcg.mean(axis=0))
    assert abs(auc_f[0] - float(a_f.double().mean())) <= 1e-12


def _metapath2vec_table(hin, metapath, dim, seed):
    model = MetaPath2Vec({k: torch.from_numpy(v) for k, v in hin['edge_index_dict'].items()}, dim, metapath, 8, 4,
                         hin['num_nodes_dict'], hin['types'], hin['type_accs'], walks_per_node=2, num_negative_samples=3,
                         sparse=False, native=True, seed=seed).cuda()
    opt = torch.optim.Adam(list(model.parameters()), lr=0.01)
    for _ in range(3):
        pos, neg = model.sample(torch.arange(40))
        opt.zero_grad()
        model.loss(pos, neg).backward()
        opt.step()
    return model.embedding.weight.detach().clone()


def test_end_to_end_from_metapath2vec_tables():
    hin = walk_ref.toy_hin()
    short = [('uid', 'has watched', 'iid'), ('iid', 'has been watched by', 'uid')]
    tables = [_metapath2vec_table(hin, hin['metapath'], 32, walk_ref.WALK_SEED), _metapath2vec_table(hin, short, 32, 77)]
    assert all(tuple(t.shape) == (hin['num_nodes'], 32) for t in tables)
    gen = torch.Generator().manual_seed(2)
    batch = torch.stack([torch.randint(0, 40, (64,), generator=gen), 40 + torch.randint(0, 30, (64,), generator=gen),
                         torch.randint(1, 6, (64,), generator=gen)], dim=1).to(DEV)
    first, last = {}, {}
    state = None
    for nat in (True, False):
        torch.manual_seed(4)
        model = HeRecRecsysModel(embeddings=tables, num_uids=40, num_iids=30, acc_uids=0, acc_iids=40, embedding_dim=32,
                                 native=nat).to(DEV)
        if state is None:
            state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state, strict=True)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        for step in range(30):
            opt.zero_grad()
            loss = model.loss(batch)
            loss.backward()
            opt.step()
            if step == 0:
                first[nat] = loss.item()
        last[nat] = loss.item()
        assert np.isfinite(last[nat]) and last[nat] < first[nat], (nat, first, last)
    engine.check_pending_errors()
    inp = {'tables': [t.cpu() for t in tables], 'acc_uids': 0, 'acc_iids': 40, 'unids': batch[:, 0].cpu(), 'inids': batch[:, 1].cpu(),
           'labels': batch[:, 2].float().cpu(), 'user_emb': state['user_emb.weight'].cpu(), 'item_emb': state['item_emb.weight'].cpu(),
           'user_rk_bias': state['user_rk_bias.weight'].cpu(), 'item_rk_bias': state['item_rk_bias.weight'].cpu(),
           'w': torch.stack([state['emb_trans.%d.weight' % k] for k in range(2)]).cpu(),
           'b': torch.stack([state['emb_trans.%d.bias' % k] for k in range(2)]).cpu()}
    truth = herec_ref.run(inp, torch.float64)['loss'].reshape(1)
    helpers.assert_fp32_close(np.array([first[True]]), np.array([first[False]]), truth, what='first-step loss')
    model.eval()
    items, scores = model.recommend(torch.arange(40, device=DEV), 10, (40, 70))
    assert bool(torch.isfinite(scores).all()) and bool((scores[:, :-1] >= scores[:, 1:]).all())
    assert bool(((items >= 40) & (items < 70)).all())
