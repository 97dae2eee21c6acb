"""GPU: CFKG in HIP (csrc/cfkg.hip through engine.cfkg_train_raw / engine.cfkg_loss / CFKGRecsysModel) against the torch
composition of experiments/cfkg_solver_bpr.py:95-106 in fp32 (the peer) and in float64 (the truth), tests/cfkg_ref.py.

Inputs (cfkg_ref.make_inputs): a = 0.7 E^-0.25, x = a randn(N, E), r = a randn(R, E), N = 500, heads drawn from 40 nodes (many
repeated rows), three fixed rows with aliased nodes.  pos and neg then have a standard deviation near 0.7: neither half of the
loss saturates and no gradient vanishes.  Widths 4, 20, 64, 128 are L = 1, 8 (three idle lanes), 16 and 32 lanes per quadruple;
batches 15 / 16 / 17 and 63 / 64 / 65 straddle the 16-quadruple tile, 1000 is one tile per workgroup, 5461 (the largest the node
scatter takes) is 342 tiles on 128 workgroups: several tiles per workgroup, unevenly.

The exact cases: x, r in {-1, 0, 1} make every product and partial sum of pos / neg an integer below 2^9.  For the relation sum,
heads and r live in the first half of the columns and tails in the second: pos = neg = 0 for every row, so a = -1/2 and b = 1/2
exactly, GH = (x[t-] - x[t+]) / 2 is a multiple of 1/2 below 2^13 in any partial sum, and grad_r is exact in any order."""
import functools
import os

import numpy as np
import pytest
import torch

import cfkg_ref
import helpers
from graph_recsys_benchmark_amd import engine, solvers
from graph_recsys_benchmark_amd.models import CFKGRecsysModel
from graph_recsys_benchmark_amd.utils import SyntheticHIN
from graph_recsys_benchmark_amd.utils.interactions import seen_items_csr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, R = 500, 9
WIDTHS = [4, 20, 64, 128]
BATCHES = [1, 15, 16, 17, 63, 64, 65, 1000, 5461]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_(t):
    return t.detach().cpu().numpy()


def both_sides(x, r, batch):
    return dict(x=x, r=r, batch=batch, peer=cfkg_ref.run(x, r, batch, torch.float32), truth=cfkg_ref.run(x, r, batch, torch.float64))


@functools.lru_cache(maxsize=None)
def case(e, b, n_rel=R):
    """inputs and both torch sides of one shape, computed once and shared (nothing below changes them)"""
    inp = cfkg_ref.make_inputs(e, n_rel, b, seed=b % 97, n=N)
    return both_sides(inp['x'].to(DEV), inp['r'].to(DEV), inp['batch'].to(DEV))


def hip_side(x, r, batch):
    x, r = (t.detach().clone().requires_grad_(True) for t in (x, r))
    loss = engine.cfkg_loss(x, r, batch)
    loss.backward()
    return dict(loss=loss.detach(), dx=x.grad, dr=r.grad)


# ---------------------------------------------------------------- exact integer inputs
def exact_inputs(e, b, n_rel):
    g = torch.Generator().manual_seed(e + b + n_rel)
    x = torch.randint(-1, 2, (N, e), generator=g).float()
    r = torch.randint(-1, 2, (n_rel, e), generator=g).float()
    batch = cfkg_ref.make_inputs(e, n_rel, b, seed=3, n=N)['batch']
    return x.to(DEV), r.to(DEV), batch.to(DEV)


@pytest.mark.parametrize('b', [1, 15, 16, 17, 65, 1000])
@pytest.mark.parametrize('e', WIDTHS)
def test_exact_pos_and_neg(e, b):
    x, r, batch = exact_inputs(e, b, 3)
    _, pos, neg, _, _, flag = engine.cfkg_train_raw(x, r, batch)
    _, want_pos, want_neg = cfkg_ref.kg_compose(x.double(), r.double(), batch)
    assert torch.equal(pos.double(), want_pos) and torch.equal(neg.double(), want_neg) and int(flag) == 0
    assert float(want_pos.abs().max()) > 0 or b == 1


@pytest.mark.parametrize('b,n_rel', [(17, 1), (65, 3), (1000, 9), (5461, 9), (5461, 64)])
@pytest.mark.parametrize('e', WIDTHS)
def test_exact_relation_sum(e, b, n_rel):
    x, r, _ = exact_inputs(e, b, n_rel)
    half = e // 2
    x[:N // 2, half:] = 0           # heads: nodes of the first half, columns of the first half
    x[N // 2:, :half] = 0           # tails: the other nodes, the other columns
    r[:, half:] = 0
    g = torch.Generator().manual_seed(b)
    batch = torch.stack([torch.randint(0, N // 2, (b,), generator=g), torch.randint(N // 2, N, (b,), generator=g),
                         torch.randint(N // 2, N, (b,), generator=g), torch.randint(0, n_rel, (b,), generator=g)], dim=1).to(DEV)
    loss, pos, neg, grad_rows, grad_r, flag = engine.cfkg_train_raw(x, r, batch)
    assert not bool(pos.any()) and not bool(neg.any()) and int(flag) == 0
    gh = 0.5 * (x[batch[:, 2]].double() - x[batch[:, 1]].double())
    assert torch.equal(grad_rows.view(b, 3, e)[:, 0].double(), gh)
    want = torch.zeros((n_rel, e), dtype=torch.float64, device=DEV).index_add_(0, batch[:, 3], gh)
    assert torch.equal(grad_r.double(), want)
    assert float(want.abs().max()) > 0 or b == 17
    # the other two rows: a hr and b hr
    hr = x[batch[:, 0]].double() + r[batch[:, 3]].double()
    assert torch.equal(grad_rows.view(b, 3, e)[:, 1].double(), -0.5 * hr) and torch.equal(grad_rows.view(b, 3, e)[:, 2].double(), 0.5 * hr)
    assert abs(float(loss) - 2 * b * float(np.log(2.0))) <= 1e-5 * 2 * b


# ---------------------------------------------------------------- random floats
def check_case(c, what):
    got = hip_side(c['x'], c['r'], c['batch'])
    truth_loss = float(c['truth']['loss'])
    print('%s: loss %.9g truth %.9g rel %.3g' % (what, float(got['loss']), truth_loss,
                                                 abs(float(got['loss']) - truth_loss) / max(abs(truth_loss), 1e-30)))
    assert abs(float(got['loss']) - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-6, what
    for k in ('dx', 'dr'):
        helpers.assert_fp32_close(np_(got[k]), np_(c['peer'][k]), np_(c['truth'][k]), what='%s %s' % (what, k))
    touched = torch.zeros(c['x'].shape[0], dtype=torch.bool, device=DEV)
    touched[c['batch'][:, :3].reshape(-1)] = True
    assert not bool(got['dx'][~touched].any()), 'rows of x.grad outside the batch must be exactly zero'
    named = torch.zeros(c['r'].shape[0], dtype=torch.bool, device=DEV)
    named[c['batch'][:, 3]] = True
    assert not bool(got['dr'][~named].any()), 'relations absent from the batch must have exactly zero gradient'
    assert float(got['dx'].abs().max()) > 0 and float(got['dr'].abs().max()) > 0
    return got


@pytest.mark.parametrize('b', BATCHES)
@pytest.mark.parametrize('e', WIDTHS)
def test_loss_and_gradients(e, b):
    check_case(case(e, b), 'E=%d B=%d' % (e, b))


@pytest.mark.parametrize('e,b,n_rel', [(20, 17, 1), (128, 65, 3), (64, 17, 64), (64, 1000, 64), (128, 5461, 64)])
def test_other_relation_counts(e, b, n_rel):
    check_case(case(e, b, n_rel), 'E=%d B=%d R=%d' % (e, b, n_rel))


@pytest.mark.parametrize('e', [20, 64])
def test_skew_all_quadruples_in_one_relation(e):
    c = case(e, 5461)
    batch = c['batch'].clone()
    batch[:, 3] = 1
    got = check_case(both_sides(c['x'], c['r'], batch), 'skew E=%d' % e)
    assert bool(got['dr'][1].any()) and not bool(got['dr'][[0] + list(range(2, R))].any())


def test_aliased_nodes():
    c = case(64, 17)
    batch = torch.tensor([[9, 9, 9, 0], [9, 5, 6, 1], [5, 9, 6, 1], [5, 6, 9, 2], [9, 9, 5, 0], [5, 9, 9, 2], [6, 5, 5, 3]], device=DEV)
    check_case(both_sides(c['x'], c['r'], batch), 'alias')


@pytest.mark.parametrize('b', [17, 1000])
@pytest.mark.parametrize('e', WIDTHS)
def test_raw_gradient_rows(e, b):
    c = case(e, b)
    loss, pos, neg, grad_rows, grad_r, flag = engine.cfkg_train_raw(c['x'], c['r'], c['batch'])
    assert grad_rows.shape == (3 * b, e) and grad_r.shape == (R, e) and int(flag) == 0
    for got, k in ((pos, 'pos'), (neg, 'neg'), (grad_rows, 'grad_rows'), (grad_r, 'dr')):
        helpers.assert_fp32_close(np_(got), np_(c['peer'][k]), np_(c['truth'][k]), what=k)
    # the formulas of the header, from the kernel's own pos and neg
    xs, rs, q = c['x'], c['r'], c['batch']
    hr = xs[q[:, 0]] + rs[q[:, 3]]
    a, bb = (torch.sigmoid(pos.double()) - 1).unsqueeze(1), torch.sigmoid(neg.double()).unsqueeze(1)
    want = torch.stack([a * xs[q[:, 1]].double() + bb * xs[q[:, 2]].double(), a * hr.double(), bb * hr.double()], dim=1)
    np.testing.assert_allclose(np_(grad_rows.view(b, 3, e)), np_(want), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- ids out of range: validated by the kernel, nothing is read through them
@pytest.mark.parametrize('col,value', [(0, -1), (0, N), (1, -1), (1, N), (2, -1), (2, N + 7), (3, -1), (3, R)])
def test_bad_ids(col, value):
    c = case(64, 1000)
    x, r = c['x'], c['r']
    clean = c['batch'][:40].clone()
    row = 5 + 7 * col               # rows 5, 12, 19, 26: the first and the second tile
    bad = clean.clone()
    bad[row, col] = value
    want = engine.cfkg_train_raw(x, r, clean)
    got = engine.cfkg_train_raw(x, r, bad)
    assert int(want[5]) == 0 and int(got[5]) == 1
    assert bool(torch.isfinite(got[0])) and all(bool(torch.isfinite(t).all()) for t in got[1:5])
    ok = torch.ones(40, dtype=torch.bool, device=DEV)
    ok[row] = False
    rows_got, rows_want = got[3].view(40, 3, -1), want[3].view(40, 3, -1)
    assert not bool(rows_got[row].any()) and float(got[1][row]) == 0 and float(got[2][row]) == 0
    assert torch.equal(rows_got[ok], rows_want[ok]) and torch.equal(got[1][ok], want[1][ok]) and torch.equal(got[2][ok], want[2][ok])
    # the row contributes nothing to the loss and to the relation gradient.  Taking a row out moves the roundings of the sums it
    # was part of: the loss (about 60 here) by a few of its ulps, inside the bound the loss has everywhere in this file; a
    # relation's column sum (at most 40 terms near 0.2 in magnitude, partial sums below 4) by at most 40 * 2^-24 * 4 < 1e-5
    term =torch.nn.functional.logsigmoid(want[1][row].double()) + torch.nn.functional.logsigmoid(-want[2][row].double())
    assert abs(float(got[0]) - (float(want[0]) + float(term))) <= 1e-5 * abs(float(want[0]))
    less = want[4].double().clone()
    less[clean[row, 3]] -= rows_want[row, 0].double()
    np.testing.assert_allclose(np_(got[4]), np_(less), rtol=1e-5, atol=1e-5)
    # the differentiable form stays asynchronous and reports at the next check; a later good call is clean
    engine.check_pending_errors()
    xg = x.clone().requires_grad_(True)
    loss = engine.cfkg_loss(xg, r, bad)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(xg.grad).all())
    with pytest.raises(IndexError):
        engine.check_pending_errors()
    engine.check_pending_errors()       # the flag was consumed
    engine.cfkg_loss(x.clone().requires_grad_(True), r, clean).backward()
    engine.check_pending_errors()


def test_forward_only_gives_the_same_loss():
    for e, b in ((20, 17), (64, 1000), (128, 5461)):
        c = case(e, b)
        x = c['x'].clone().requires_grad_(True)
        with_grad = engine.cfkg_loss(x, c['r'], c['batch'])
        assert with_grad.requires_grad
        with torch.no_grad():
            without = engine.cfkg_loss(x, c['r'], c['batch'])
        assert not without.requires_grad and torch.equal(with_grad.detach(), without)
        assert not engine.cfkg_loss(c['x'], c['r'], c['batch']).requires_grad      # no input requires grad
        raw = engine.cfkg_train_raw(c['x'], c['r'], c['batch'], need_grad=False)
        assert raw[3] is None and raw[4] is None and torch.equal(raw[0], without)
        full = engine.cfkg_train_raw(c['x'], c['r'], c['batch'])
        assert torch.equal(full[0], raw[0]) and torch.equal(full[1], raw[1]) and torch.equal(full[2], raw[2])
        # only x or only r asks for a gradient: the other is None
        r = c['r'].clone().requires_grad_(True)
        engine.cfkg_loss(c['x'], r, c['batch']).backward()
        helpers.assert_fp32_close(np_(r.grad), np_(c['peer']['dr']), np_(c['truth']['dr']), what='dr alone')


def test_two_runs_agree_bitwise():
    for e, b in ((20, 1000), (64, 5461), (128, 5461)):
        c = case(e, b)
        a, again = engine.cfkg_train_raw(c['x'], c['r'], c['batch']), engine.cfkg_train_raw(c['x'], c['r'], c['batch'])
        for k in range(5):
            assert torch.equal(a[k], again[k]), k
        a, again = hip_side(c['x'], c['r'], c['batch']), hip_side(c['x'], c['r'], c['batch'])
        for k in ('loss', 'dx', 'dr'):
            assert torch.equal(a[k], again[k]), k


def test_strided_x_gives_the_contiguous_result():
    for e, b in ((20, 17), (64, 1000)):
        c = case(e, b)
        want = hip_side(c['x'], c['r'], c['batch'])
        wide = torch.zeros((N, e + 4), device=DEV)
        wide[:, 4:] = c['x']
        wide.requires_grad_(True)
        view = wide[:, 4:]
        assert view.stride(0) == e + 4
        r = c['r'].clone().requires_grad_(True)
        loss = engine.cfkg_loss(view, r, c['batch'])
        loss.backward()
        assert torch.equal(loss.detach(), want['loss']) and torch.equal(wide.grad[:, 4:], want['dx'])
        assert not bool(wide.grad[:, :4].any()) and torch.equal(r.grad, want['dr'])


# ---------------------------------------------------------------- the model
def build(e, n_rel, native, x=None, r=None, n=N, num_uids=150, acc_uids=0, rating_r_idx=0, seed=1):
    torch.manual_seed(seed)
    ds = cfkg_ref.model_dataset(n, num_uids, acc_uids, n_rel, rating_r_idx)
    model = CFKGRecsysModel(dataset=ds, emb_dim=e, native=native)
    if x is not None:
        cfkg_ref.load_model(model, np_(x), np_(r))
    return model.to(DEV)


def is_native(loss):
    return 'Cfkg' in type(loss.grad_fn).__name__


@pytest.mark.parametrize('e,n_rel,b', [(6, 9, 64), (64, 65, 64), (64, 9, 5462)])
def test_refused_shapes_take_the_torch_path(e, n_rel, b):
    assert not engine.cfkg_supported(e, n_rel, b)
    inp = cfkg_ref.make_inputs(e, n_rel, b, seed=2, n=N)
    batch = inp['batch'].to(DEV)
    out = {}
    for native in (True, False):
        model = build(e, n_rel, native, inp['x'], inp['r'])
        model.train()
        loss = model.kg_loss(batch)
        assert not is_native(loss)
        loss.backward()
        out[native] = (loss.detach(), model.x.grad, model.r.grad)
    for a, b_ in zip(out[True], out[False]):
        assert torch.equal(a, b_)
    with pytest.raises(ValueError):
        engine.cfkg_loss(inp['x'].to(DEV), inp['r'].to(DEV), batch)


def test_model_with_the_switch_on_and_off():
    c = case(64, 1000)
    got = {}
    for native in (True, False):
        model = build(64, R, native, c['x'], c['r'])
        model.train()
        loss = model.kg_loss(c['batch'])
        assert is_native(loss) == native
        loss.backward()
        got[native] = dict(loss=loss.detach(), dx=model.x.grad, dr=model.r.grad)
        assert not is_native(model.kg_loss(c['batch'].to(torch.int32)))       # not an int64 batch: the composition
        model.eval()
        assert is_native(model.kg_loss(c['batch'])) == native                 # eval mode takes the same route
        with torch.no_grad():
            again = model.kg_loss(c['batch'])
        assert not again.requires_grad and torch.equal(again, got[native]['loss'])
    truth = c['truth']
    for side in got.values():
        assert abs(float(side['loss']) - float(truth['loss'])) <= 1e-5 * abs(float(truth['loss'])) + 1e-6
    for k in ('dx', 'dr'):
        helpers.assert_fp32_close(np_(got[True][k]), np_(got[False][k]), np_(truth[k]), what='model ' + k)


def test_adam_run_on_kg_loss():
    c = case(64, 1000)
    model = build(64, R, True)
    with torch.no_grad():
        model.x.mul_(4.0)
        model.r.mul_(4.0)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    model.train()
    losses = []
    for it in range(21):
        opt.zero_grad()
        loss = model.kg_loss(c['batch'])
        assert is_native(loss)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    engine.check_pending_errors()
    assert losses[20] < losses[0], 'loss did not go down in 20 steps: %r -> %r' % (losses[0], losses[20])


# ---------------------------------------------------------------- evaluation routes
@pytest.fixture(scope='module')
def hin():
    ds = SyntheticHIN('ml_small', scale=0.1)
    ds.eval_split(num_users=40)
    return ds


def test_evaluation_routes(hin):
    torch.manual_seed(4)
    model = CFKGRecsysModel(dataset=hin, emb_dim=20).to(DEV)
    assert tuple(model.r.shape) == (len(hin.edge_index_nps), 20) and model.rating_r_idx == list(hin.edge_index_nps).index('user2item')
    with torch.no_grad():
        model.x.mul_(6.0)
        model.r.mul_(6.0)
    lo, n = hin.type_accs['iid'], hin.num_iids
    u_nids = list(hin.test_pos_unid_inid_map.keys())
    u_t = torch.tensor(u_nids, device=DEV)
    model.train()
    with pytest.raises(RuntimeError):
        model.recommend(u_t, 10, (lo, lo + n))
    model.eval()
    with torch.no_grad():       # the composition on every (user, item) pair: the predictions, and their logarithms for the ranks
        uu, ii = u_t.repeat_interleave(n), torch.arange(lo, lo + n, device=DEV).repeat(len(u_nids))
        full = model(uu, ii).view(len(u_nids), n)
        full_log = torch.sum((model.x[uu] + model.r[model.rating_r_idx]) * model.x[ii], dim=-1).view(len(u_nids), n)
    assert float(full.max() / full.min()) > 2.0                 # the scores are spread: the ranking is not a tie-break
    # predict in eval mode: exp of the table's row dots
    items = torch.arange(lo, lo + len(u_nids), device=DEV)
    np.testing.assert_allclose(np_(model.predict(u_t, items)), np_(full[torch.arange(len(u_nids)), items - lo]), rtol=1e-5)
    # metrics: the same draw ranked on the host from the composition's scores
    np.random.seed(11)
    hr, ndcg, auc, loss = solvers.metrics(model, hin)
    np.random.seed(11)
    cand = torch.from_numpy(solvers._draw_candidates(hin, u_nids, 99)).to(DEV)
    sc, sc_log = full.gather(1, cand - lo), full_log.gather(1, cand - lo)
    rank = (sc_log[:, 1:] > sc_log[:, :1]).sum(dim=1)
    want_hr, want_ndcg = solvers.metrics_from_ranks(np_(rank))
    np.testing.assert_array_equal(hr, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg, want_ndcg.mean(axis=0))
    assert abs(auc[0] - float((sc_log[:, 1:] < sc_log[:, :1]).double().mean(dim=1).mean())) <= 1e-6
    label = torch.zeros_like(sc)
    label[:, 0] = 1
    want = float(torch.nn.functional.binary_cross_entropy_with_logits(sc.double(), label.double()))
    assert abs(loss[0] - want) <= 1e-5 * want
    pred, k_rank, _, _ = model.rank_eval(u_t, cand)
    np.testing.assert_allclose(np_(pred), np_(sc), rtol=1e-5)
    assert torch.equal(k_rank.long(), rank)
    # metrics_full: every unseen item a negative
    exclude = seen_items_csr(hin.edge_index_nps['user2item'], u_t, (lo, lo + n))
    pos = np.asarray([hin.test_pos_unid_inid_map[u][0] for u in u_nids], dtype=np.int64)
    hr_f, ndcg_f, auc_f = solvers.metrics_full(model, u_nids, pos, (lo, lo + n), exclude=exclude)
    elig = torch.ones((len(u_nids), n), dtype=torch.bool, device=DEV)
    rows = torch.repeat_interleave(torch.arange(len(u_nids), device=DEV), exclude[0][1:] - exclude[0][:-1])
    elig[rows, exclude[1] - lo] = False
    pos_sc = full_log.gather(1, torch.from_numpy(pos).to(DEV).view(-1, 1) - lo)
    rank_f = ((full_log > pos_sc) & elig).sum(dim=1)
    want_hr, want_ndcg = solvers.metrics_from_ranks(np_(rank_f))
    np.testing.assert_array_equal(hr_f, want_hr.mean(axis=0))
    np.testing.assert_array_equal(ndcg_f, want_ndcg.mean(axis=0))
    # recommend: the ten best unseen items by the composition's score, ties to the lower id; scores are predictions
    got_items, got_scores = model.recommend(u_t, 10, (lo, lo + n), exclude=exclude)
    masked = torch.where(elig, full_log, torch.full_like(full_log, -1e30))
    order = torch.argsort(masked, dim=1, descending=True, stable=True)[:, :10]
    assert torch.equal(got_items, order + lo)
    np.testing.assert_allclose(np_(got_scores), np_(full.gather(1, order)), rtol=1e-5)


def test_fixture_on_the_gpu():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'cfkg_small.npz'))
    inp = cfkg_ref.golden_inputs(z)
    model = build(z['sd.x'].shape[1], z['sd.r'].shape[0], True, inp['x'], inp['r'], n=inp['num_nodes'], num_uids=inp['num_uids'],
                  acc_uids=inp['acc_uids'], rating_r_idx=inp['rating_r_idx'])
    model.train()
    loss = model.kg_loss(inp['batch'].to(DEV))
    assert is_native(loss)
    loss.backward()
    for want_loss, want_x, want_r in ((z['loss'], z['grad.x'], z['grad.r']), (z['f64.loss'], z['f64.x'], z['f64.r'])):
        np.testing.assert_allclose(np_(loss), want_loss, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(np_(model.x.grad), want_x, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(np_(model.r.grad), want_r, rtol=1e-5, atol=1e-6)
    u, i = inp['unids'].to(DEV), inp['inids'].to(DEV)
    with torch.no_grad():
        np.testing.assert_allclose(np_(model.predict(u, i)), z['pred'], rtol=1e-6)
    model.eval()
    np.testing.assert_allclose(np_(model.predict(u, i)), z['pred'], rtol=1e-6)
    engine.check_pending_errors()
