"""GPU: the KG phase in HIP (csrc/transr_train.hip through engine.transr_train_raw / engine.transr_loss) against the torch
composition of models/kg_base.py: kg_loss in fp32 (the peer) and in float64 (the truth).

Inputs: a = 0.7 E^-0.25, x = a randn(N, E), r = a randn(R, E), P = randn(E, E) / sqrt(E), N = 500, R = 5, heads drawn from 40
nodes (many repeated rows), and three fixed rows: (7, 7, 9, 0) has h == t+, (3, 50, 50, R-1) has t+ == t- (d = 0),
(3, 50, 61, R-1).  With these |d| has a median near 2 and stays below 27: the loss does not saturate and the gradients are not
all zero.  The exact case uses x, r, P in {-1, 0, 1}: |dpos_c| <= 2 E + 1, pos <= 128 * 257^2 < 2^24, so every partial sum is
an exact fp32 integer in any order."""
import functools

import pytest
import torch

import helpers
from graph_recsys_benchmark_amd import engine

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, R = 500, 5
WIDTHS = [4, 20, 64, 128]
BATCHES = [1, 15, 16, 17, 1000, 5461]      # the tile boundary, several tiles per workgroup, the largest batch the scatter takes


def make_batch(b, n_rel, seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(N, generator=g)[:40]
    batch = torch.stack([pool[torch.randint(0, 40, (b,), generator=g)], torch.randint(0, N, (b,), generator=g),
                         torch.randint(0, N, (b,), generator=g), torch.randint(0, n_rel, (b,), generator=g)], dim=1)
    fixed = torch.tensor([[7, 7, 9, 0], [3, 50, 50, n_rel - 1], [3, 50, 61, n_rel - 1]])
    k = min(b, 3)
    batch[:k] = fixed[:k]
    return batch.to(device)


def make_floats(e, n_rel, seed):
    g = torch.Generator().manual_seed(seed)
    a = 0.7 * e ** -0.25
    x = a * torch.randn(N, e, generator=g)
    r = a * torch.randn(n_rel, e, generator=g)
    p = torch.randn(e, e, generator=g) / e ** 0.5
    return x.to(DEV), p.to(DEV), r.to(DEV)


def compose(h, tp, tn, rr, p):
    """kg_loss of models/kg_base.py on the gathered rows"""
    head = torch.mm(h, p) + rr
    pos_diff = head - torch.mm(tp, p)
    neg_diff = head - torch.mm(tn, p)
    pos = (pos_diff * pos_diff).sum(-1)
    neg = (neg_diff * neg_diff).sum(-1)
    return -(pos - neg).sigmoid().log().sum(), pos, neg


def torch_side(x, p, r, batch, dtype):
    """loss, dx, dP, dr of the composition under autograd, and the gradients of the gathered rows ([3B, E] in the order
    h, t+, t- per quadruple, [B, E] for the relation rows)"""
    x, p, r = (t.detach().to(dtype).requires_grad_(True) for t in (x, p, r))
    rows = [x[batch[:, 0]], x[batch[:, 1]], x[batch[:, 2]], r[batch[:, 3]]]
    for t in rows:
        t.retain_grad()
    loss, pos, neg = compose(rows[0], rows[1], rows[2], rows[3], p)
    loss.backward()
    grad_rows = torch.stack([rows[0].grad, rows[1].grad, rows[2].grad], dim=1).reshape(-1, x.shape[1])
    return dict(loss=loss.detach(), pos=pos.detach(), neg=neg.detach(), dx=x.grad, dp=p.grad, dr=r.grad, grad_rows=grad_rows,
                grad_rel=rows[3].grad)


@functools.lru_cache(maxsize=None)
def case(e, b, n_rel=R):
    """inputs and both torch sides of one shape, computed once and shared (nothing below changes them)"""
    x, p, r = make_floats(e, n_rel, 100 + e)
    batch = make_batch(b, n_rel, 7 * b + e)
    return dict(x=x, p=p, r=r, batch=batch, peer=torch_side(x, p, r, batch, torch.float32),
                truth=torch_side(x, p, r, batch, torch.float64))


def hip_side(x, p, r, batch):
    x, p, r = (t.detach().clone().requires_grad_(True) for t in (x, p, r))
    loss = engine.transr_loss(x, p, r, batch)
    loss.backward()
    return dict(loss=loss.detach(), dx=x.grad, dp=p.grad, dr=r.grad)


def np_(t):
    return t.detach().cpu().numpy()


def exact_inputs(e, b, device=DEV):
    """x, P, r in {-1, 0, 1} and the batch of the exact case (the module's docstring says why every sum is an integer)"""
    g = torch.Generator().manual_seed(e + b)
    x = torch.randint(-1, 2, (N, e), generator=g).float().to(device)
    r = torch.randint(-1, 2, (R, e), generator=g).float().to(device)
    p = torch.randint(-1, 2, (e, e), generator=g).float().to(device)
    return x, p, r, make_batch(b, R, 3 * b + e, device)


def exact_pos_neg(x, p, r, batch, dtype):
    """pos, neg of the composition in `dtype`"""
    xd, pd, rd = x.to(dtype), p.to(dtype), r.to(dtype)
    _, pos, neg = compose(xd[batch[:, 0]], xd[batch[:, 1]], xd[batch[:, 2]], rd[batch[:, 3]], pd)
    return pos, neg


def check_exact(e, b):
    x, p, r, batch = exact_inputs(e, b)
    _, pos, neg, _, _, _, flag = engine.transr_train_raw(x, p, r, batch)
    want_pos, want_neg = exact_pos_neg(x, p, r, batch, torch.float64)
    assert float(want_pos.max()) < 2 ** 24
    assert torch.equal(pos.double(), want_pos) and torch.equal(neg.double(), want_neg)
    assert int(flag) == 0


@pytest.mark.parametrize('b', [1, 15, 16, 17, 1000])
@pytest.mark.parametrize('e', WIDTHS)
def test_exact_integer_case(e, b):
    check_exact(e, b)


def check_case(c, what):
    got = hip_side(c['x'], c['p'], c['r'], c['batch'])
    truth_loss = float(c['truth']['loss'])
    print('%s: loss %.9g truth %.9g rel %.3g' % (what, float(got['loss']), truth_loss,
                                                 abs(float(got['loss']) - truth_loss) / max(abs(truth_loss), 1e-30)))
    assert abs(float(got['loss']) - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-6, what
    for k in ('dx', 'dp', 'dr'):
        helpers.assert_fp32_close(np_(got[k]), np_(c['peer'][k]), np_(c['truth'][k]), what='%s %s' % (what, k))
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[c['batch'][:, :3].reshape(-1)] = True
    assert not bool(got['dx'][~touched].any()), 'rows of x.grad outside the batch must be exactly zero'
    assert float(got['dx'].abs().max()) > 0 and float(got['dp'].abs().max()) > 0 and float(got['dr'].abs().max()) > 0


@pytest.mark.parametrize('b', BATCHES)
@pytest.mark.parametrize('e', WIDTHS)
def test_loss_and_gradients(e, b):
    check_case(case(e, b), 'E=%d B=%d' % (e, b))


def test_one_relation():
    check_case(case(20, 17, 1), 'E=20 B=17 R=1')


def check_raw_rows(e, b):
    c = case(e, b)
    loss, pos, neg, grad_rows, grad_rel, dproj, flag = engine.transr_train_raw(c['x'], c['p'], c['r'], c['batch'])
    assert grad_rows.shape == (3 * b, e) and grad_rel.shape == (b, e) and dproj.shape == (e, e) and int(flag) == 0
    helpers.assert_fp32_close(np_(pos), np_(c['peer']['pos']), np_(c['truth']['pos']), what='pos')
    helpers.assert_fp32_close(np_(neg), np_(c['peer']['neg']), np_(c['truth']['neg']), what='neg')
    helpers.assert_fp32_close(np_(grad_rows), np_(c['peer']['grad_rows']), np_(c['truth']['grad_rows']), what='grad_rows')
    helpers.assert_fp32_close(np_(grad_rel), np_(c['peer']['grad_rel']), np_(c['truth']['grad_rel']), what='grad_rel_rows')
    helpers.assert_fp32_close(np_(dproj), np_(c['peer']['dp']), np_(c['truth']['dp']), what='dproj')


@pytest.mark.parametrize('b', [17, 1000])
@pytest.mark.parametrize('e', WIDTHS)
def test_raw_gradient_rows(e, b):
    check_raw_rows(e, b)


def test_bad_ids():
    c = case(64, 1000)
    x, p, r = c['x'], c['p'], c['r']
    clean = c['batch'][:40].clone()
    bad = clean.clone()
    bad[5, 1], bad[20, 0], bad[33, 3] = N, -1, R          # three different rows, in three different tiles
    bad_rows = [5, 20, 33]
    want = engine.transr_train_raw(x, p, r, clean)
    got = engine.transr_train_raw(x, p, r, bad)
    assert int(want[6]) == 0 and int(got[6]) == 1
    assert bool(torch.isfinite(got[0])) and all(bool(torch.isfinite(t).all()) for t in got[1:6])
    ok = torch.ones(40, dtype=torch.bool, device=DEV)
    ok[bad_rows] = False
    rows_got, rows_want = got[3].view(40, 3, -1), want[3].view(40, 3, -1)
    assert not bool(rows_got[~ok].any()) and not bool(got[4][~ok].any())
    assert torch.equal(rows_got[ok], rows_want[ok]) and torch.equal(got[4][ok], want[4][ok])
    assert torch.equal(got[1][ok], want[1][ok]) and torch.equal(got[2][ok], want[2][ok])
    # the differentiable form stays asynchronous and reports at the next check
    engine.check_pending_errors()
    xg = x.clone().requires_grad_(True)
    loss = engine.transr_loss(xg, p, r, bad)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(xg.grad).all())
    with pytest.raises(IndexError):
        engine.check_pending_errors()
    engine.check_pending_errors()       # the flag was consumed


def check_forward_only(e, b):
    c = case(e, b)
    x = c['x'].clone().requires_grad_(True)
    with_grad = engine.transr_loss(x, c['p'], c['r'], c['batch'])
    assert with_grad.requires_grad
    with torch.no_grad():
        without = engine.transr_loss(x, c['p'], c['r'], c['batch'])
    assert not without.requires_grad and torch.equal(with_grad.detach(), without)
    assert not engine.transr_loss(c['x'], c['p'], c['r'], c['batch']).requires_grad      # no input requires grad
    raw = engine.transr_train_raw(c['x'], c['p'], c['r'], c['batch'], need_grad=False)
    assert raw[3] is None and raw[4] is None and raw[5] is None and torch.equal(raw[0], without)


def test_forward_only_gives_the_same_loss():
    for e, b in ((20, 17), (64, 1000), (128, 1000)):
        check_forward_only(e, b)


def test_two_runs_agree_bitwise():
    for e, b in ((20, 1000), (128, 5461)):
        c = case(e, b)
        a, again = hip_side(c['x'], c['p'], c['r'], c['batch']), hip_side(c['x'], c['p'], c['r'], c['batch'])
        for k in ('loss', 'dx', 'dp', 'dr'):
            assert torch.equal(a[k], again[k]), k


def test_strided_x_gives_the_contiguous_result():
    for e, b in ((20, 17), (64, 1000)):
        c = case(e, b)
        want = hip_side(c['x'], c['p'], c['r'], c['batch'])
        wide = torch.zeros((N, e + 4), device=DEV)
        wide[:, 4:] = c['x']
        wide.requires_grad_(True)
        view = wide[:, 4:]
        assert view.stride(0) == e + 4
        p, r = (t.clone().requires_grad_(True) for t in (c['p'], c['r']))
        loss = engine.transr_loss(view, p, r, c['batch'])
        loss.backward()
        assert torch.equal(loss.detach(), want['loss']) and torch.equal(wide.grad[:, 4:], want['dx'])
        assert not bool(wide.grad[:, :4].any())
        assert torch.equal(p.grad, want['dp']) and torch.equal(r.grad, want['dr'])


def test_refusals():
    assert not engine.transr_supported(64, 5462) and not engine.transr_supported(132, 64)
    assert engine.transr_supported(64, 5461) and engine.transr_supported(128, 1)
    x, p, r = make_floats(64, R, 1)
    with pytest.raises(ValueError):
        engine.transr_loss(x, p, r, make_batch(5462, R, 1))
    x, p, r = make_floats(132, R, 1)
    with pytest.raises(ValueError):
        engine.transr_loss(x, p, r, make_batch(64, R, 1))


def test_a_queued_flag_does_not_pin_the_workspace():
    """the flag a transr_loss call queues stays alive until the next check (a KG phase only checks at eval()): it must not keep
    the step's workspace -- the [E, E] partials of every workgroup -- alive with it.  E = 64, B = 40 as in test_bad_ids."""
    from graph_recsys_benchmark_amd import _lib, errors
    assert int(_lib.load().pea_transr_train_workspace_bytes(40, 64)) > errors.WS_FLAG_VIEW_MAX == 4096
    c = case(64, 1000)
    x, p, r, clean = c['x'], c['p'], c['r'], c['batch'][:40].clone()
    engine.check_pending_errors()
    engine.transr_loss(x.clone().requires_grad_(True), p, r, clean).backward()
    assert engine._pending_err[-1].untyped_storage().nbytes() <= 4096
    bad = clean.clone()
    bad[5, 1] = N
    engine.transr_loss(x.clone().requires_grad_(True), p, r, bad).backward()
    assert engine._pending_err[-1].untyped_storage().nbytes() <= 4096
    with pytest.raises(IndexError):
        engine.check_pending_errors()
    assert not engine._pending_err


def test_a_queued_herec_flag_does_not_pin_the_workspace():
    """the same rule for herec_mse_loss at (D, M) = (64, 2), B = 40"""
    import herec_ref
    from graph_recsys_benchmark_amd import _lib, errors
    assert int(_lib.load().pea_herec_train_workspace_bytes(40, 64, 2)) > errors.WS_FLAG_VIEW_MAX == 4096
    inp = herec_ref.make_inputs(64, 2, 40)
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items()}
    g['tables'] = [t.to(DEV) for t in inp['tables']]
    params = [g[k].clone().requires_grad_(True) for k in ('w', 'b', 'user_emb', 'item_emb', 'user_rk_bias', 'item_rk_bias')]
    engine.check_pending_errors()
    engine.herec_mse_loss(g['tables'], *params, g['acc_uids'], g['acc_iids'], g['unids'], g['inids'], g['labels']).backward()
    assert engine._pending_err[-1].untyped_storage().nbytes() <= 4096
    engine.check_pending_errors()
    assert not engine._pending_err
