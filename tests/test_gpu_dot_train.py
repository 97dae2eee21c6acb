"""GPU: the training head of the inner-product scorer (csrc/dot_train.hip, engine.dot_bpr_loss) against a torch restatement:
table = cat_k normalize(block_k), pos / neg = row inner products, loss = -sum logsigmoid(pos - neg).  float64 is the truth,
the same restatement in float32 under autograd the peer helpers.assert_fp32_close asks for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
from graph_recsys_benchmark_amd import engine

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 500
WIDTHS = [(16, 8, 4), (64, 32, 16), (4,), (64, 64, 64, 64)]
BATCHES = [1, 63, 64, 65, 1000]
ZERO_NODE = 7          # the node whose middle (or only) block is all zero


def make_blocks(widths, seed):
    g = torch.Generator().manual_seed(seed)
    blocks = [torch.randn((N, w), generator=g).to(DEV) for w in widths]
    blocks[len(widths) // 2][ZERO_NODE] = 0.0
    return blocks


def make_batch(b, seed):
    """Triples with repeated users and items, i == j in one triple (B > 1), and ZERO_NODE as a user and as an item."""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.integers(0, 40, size=b), rng.integers(40, 120, size=b), rng.integers(40, N, size=b)], axis=1)
    t[0] = [ZERO_NODE, 41, 42]
    if b > 1:
        t[1] = [3, 50, 50]
    if b > 3:
        t[2] = [3, 50, 61]
        t[3] = [5, ZERO_NODE, 50]
    return torch.from_numpy(t.astype(np.int64)).to(DEV)


def restate(blocks, batch, dtype):
    """(loss, dense gradients per block) of the restatement in `dtype` under autograd."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in blocks]
    table = torch.cat([F.normalize(t, dim=-1) for t in leaves], dim=-1)
    pos = (table[batch[:, 0]] * table[batch[:, 1]]).sum(-1)
    neg = (table[batch[:, 0]] * table[batch[:, 2]]).sum(-1)
    loss = -F.logsigmoid(pos - neg).sum()
    loss.backward()
    return loss.detach(), [t.grad for t in leaves]


def split_zero_rows(blocks):
    """row mask per block: True where the row is all zero (its gradient is dn / 1e-12, of order 1e12)"""
    return [(t == 0).all(dim=1).cpu().numpy() for t in blocks]


@pytest.fixture(scope='module', params=WIDTHS, ids=lambda w: 'x'.join(map(str, w)))
def blocks(request):
    return request.param, make_blocks(request.param, seed=sum(request.param))


@pytest.mark.parametrize('b', BATCHES)
def test_loss_and_dense_gradients(blocks, b):
    widths, tensors = blocks
    batch = make_batch(b, seed=b)
    want_loss, want = restate(tensors, batch, torch.float32)
    true_loss, truth = restate(tensors, batch, torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    loss = engine.dot_bpr_loss(leaves, batch)
    assert loss.dim() == 0 and loss.requires_grad
    assert abs(float(loss.detach()) - float(true_loss)) <= 1e-5 * abs(float(true_loss)) + 1e-6
    loss.backward()
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[batch[:, :3].reshape(-1)] = True
    for k, (leaf, w32, w64, zero) in enumerate(zip(leaves, want, truth, split_zero_rows(tensors))):
        got = leaf.grad
        assert got.shape == leaf.shape
        assert bool((got[~touched] == 0).all()), 'a row outside the batch got a gradient'
        g, p, t = got.cpu().numpy(), w32.cpu().numpy(), w64.cpu().numpy()
        helpers.assert_fp32_close(g[~zero], p[~zero], t[~zero], what='block %d gradient' % k)
        if zero.any():
            assert np.abs(t[zero]).max() > 1e9, 'the zero row is in the batch and its gradient is dn / 1e-12'
            assert (np.abs(g[zero] - t[zero]) <= 1e-5 * np.abs(t[zero]).max()).all()
    engine.check_pending_errors()


@pytest.mark.parametrize('b', [65, 1000])
def test_grad_rows(blocks, b):
    widths, tensors = blocks
    batch = make_batch(b, seed=b + 1)
    loss, grad_rows, flag = engine.dot_bpr_train_raw(tensors, batch)
    assert grad_rows.shape == (3 * b, sum(widths)) and int(flag) == 0

    def rows_of(dtype):
        # the same restatement with the 3B gathered rows as leaves: d loss / d (the raw rows)
        ids = batch[:, :3].reshape(-1)
        rows = torch.cat([t.to(dtype)[ids] for t in tensors], dim=-1).detach().requires_grad_(True)
        off, parts = 0, []
        for w in widths:
            parts.append(F.normalize(rows[:, off:off + w], dim=-1))
            off += w
        tbl = torch.cat(parts, dim=-1).view(b, 3, -1)
        l = -F.logsigmoid((tbl[:, 0] * tbl[:, 1]).sum(-1) - (tbl[:, 0] * tbl[:, 2]).sum(-1)).sum()
        l.backward()
        return l.detach(), rows.grad

    (l32, g32), (l64, g64) = rows_of(torch.float32), rows_of(torch.float64)
    assert abs(float(loss) - float(l64)) <= 1e-5 * abs(float(l64)) + 1e-6
    off = 0
    for w, t in zip(widths, tensors):
        ids = batch[:, :3].reshape(-1)
        zero = (t[ids] == 0).all(dim=1).cpu().numpy()
        g, p, tr = (a[:, off:off + w].cpu().numpy() for a in (grad_rows, g32, g64))
        helpers.assert_fp32_close(g[~zero], p[~zero], tr[~zero], what='grad_rows block at column %d' % off)
        if zero.any():
            assert (np.abs(g[zero] - tr[zero]) <= 1e-5 * np.abs(tr[zero]).max()).all()
        off += w


def test_out_of_range_id_sets_the_flag_and_leaves_the_loss_finite():
    tensors = make_blocks((16, 8, 4), seed=1)
    batch = make_batch(65, seed=2)
    clean_loss, clean_rows, flag = engine.dot_bpr_train_raw(tensors, batch)
    assert int(flag) == 0
    bad = batch.clone()
    bad[10, 1] = N
    bad[20, 0] = -1
    loss, grad_rows, flag = engine.dot_bpr_train_raw(tensors, bad)
    assert int(flag) == 1 and bool(torch.isfinite(loss)) and bool(torch.isfinite(grad_rows).all())
    assert bool((grad_rows[30:33] == 0).all()) and bool((grad_rows[60:63] == 0).all())
    keep = torch.ones(65 * 3, dtype=torch.bool, device=DEV)
    keep[30:33] = False
    keep[60:63] = False
    assert torch.equal(grad_rows[keep], clean_rows[keep])
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    engine.dot_bpr_loss(leaves, bad).backward()
    with pytest.raises(IndexError):
        engine.check_pending_errors()


def test_unsupported_shapes_are_refused():
    assert not engine.dot_bpr_supported([20, 10, 5], 64) and not engine.dot_bpr_supported([16, 8, 4], 5462)
    assert engine.dot_bpr_supported([16, 8, 4], 5461)
    with pytest.raises(ValueError):
        engine.dot_bpr_loss([torch.zeros((N, 20), device=DEV), torch.zeros((N, 10), device=DEV)], make_batch(4, seed=1))
