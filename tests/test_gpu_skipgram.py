"""GPU: pea_skipgram_train (csrc/skipgram.hip) against the torch restatement of the reference's loss on the reference's window
layout (tests/walk_ref.py): the float32 restatement on the CPU is the yardstick, the float64 one the truth."""
import ctypes as C

import numpy as np
import pytest
import torch

import walk_ref
from helpers import assert_fp32_close

pytestmark = pytest.mark.gpu

N_NODES = 50
_REF = {}


def _table(n, d, seed=11):
    return (torch.randn((n, d), generator=torch.Generator().manual_seed(seed)) * 0.3).numpy()


def _rows(rng, m, t, n=N_NODES):
    return rng.integers(0, n, size=(m, t)).astype(np.int64)


def _reference(key, weight, pos, neg, c):
    """the two restatements of one case, computed once"""
    if key not in _REF:
        pw = walk_ref.windows(pos, c) if pos.shape[0] else np.zeros((0, c), np.int64)
        nw = walk_ref.windows(neg, c) if neg.shape[0] else np.zeros((0, c), np.int64)
        _REF[key] = (walk_ref.skipgram_loss(weight, pw, nw, torch.float32), walk_ref.skipgram_loss(weight, pw, nw, torch.float64))
    return _REF[key]


def _run(weight, pos, neg, c):
    from graph_recsys_benchmark_amd import engine
    out = engine.skipgram_train_raw(torch.from_numpy(weight).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), c)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(key, weight, pos, neg, c, flagged=False):
    got = _run(weight, pos, neg, c)
    (l32, g32, cnt32), (l64, g64, cnt64) = _reference(key, weight, pos, neg, c)
    assert got['n_valid'].tolist() == cnt64 == cnt32
    assert_fp32_close(got['loss'], l32, l64, what='loss %s' % (key,))
    assert_fp32_close(got['grad'], g32, g64, what='grad %s' % (key,))
    n = weight.shape[0]
    touched = got['touched'][:int(got['touched_count'][0])]
    assert (np.diff(touched) > 0).all() and (touched >= 0).all() and (touched < n).all()      # ascending, unique
    ids = np.concatenate([pos.reshape(-1), neg.reshape(-1)])
    np.testing.assert_array_equal(touched, np.unique(ids[(ids >= 0) & (ids < n)]))
    rest = np.setdiff1d(np.arange(n), touched)
    assert not got['grad'][rest].any()                                                         # exactly zero elsewhere
    assert int(got['flag']) == (1 if flagged else 0)
    return got


SHAPES = [(7, 7), (8, 2), (11, 7), (101, 7), (128, 16)]
SIDES = [(5, 25), (3, 0), (0, 4)]
CASES = ([(64, t, c, p, q) for t, c in SHAPES for p, q in SIDES] +
         [(d, t, c, 5, 25) for d in (4, 68, 128) for t, c in SHAPES] +
         [(4, 8, 2, 3, 0), (128, 11, 7, 0, 4)])


@pytest.mark.parametrize('d,t,c,n_pos,n_neg', CASES, ids=['D%d-T%d-C%d-%dx%d' % k for k in CASES])
def test_loss_and_gradient(d, t, c, n_pos, n_neg):
    rng = np.random.default_rng(1000 * t + c)
    pos, neg = _rows(rng, n_pos, t), _rows(rng, n_neg, t)
    _check(('rand', d, t, c, n_pos, n_neg), _table(N_NODES, d), pos, neg, c)


def _edge_rows(t=11):
    rng = np.random.default_rng(5)
    pos, neg = _rows(rng, 6, t), _rows(rng, 8, t)
    pos[1, 6:] = -1                      # dead-end tails
    pos[2, 1:] = -1                      # only the start left: no valid pair, still a touched node
    pos[3, :] = -1                       # nothing at all
    neg[0, 9:] = -1
    neg[5, :] = -1
    pos[4, 2] = pos[4, 0]                # a node revisited inside one window: a row dotted with itself
    pos[4, 5] = pos[4, 4]
    neg[2, 1] = neg[2, 0]
    return pos, neg


@pytest.mark.parametrize('d', [64, 68])
def test_dead_ends_and_revisits(d):
    pos, neg = _edge_rows()
    got = _check(('edge', d), _table(N_NODES, d), pos, neg, 7)
    assert got['n_valid'][0] < 6 * 5 * 6 and got['n_valid'][1] < 8 * 5 * 6


def test_id_beyond_the_table_is_skipped_and_flagged():
    pos, neg = _edge_rows()
    pos[0, 3] = N_NODES
    neg[1, 0] = N_NODES + 100
    _check(('beyond',), _table(N_NODES, 64), pos, neg, 7, flagged=True)


def test_two_nodes_own_twenty_thousand_positions_each():
    """400 rows of 101 ids over a two-node table: beyond the LDS sorter of rows_scatter.hip, and two very long runs"""
    rng = np.random.default_rng(9)
    pos, neg = _rows(rng, 80, 101, n=2), _rows(rng, 320, 101, n=2)
    got = _check(('hubs',), _table(2, 64, seed=3), pos, neg, 7)
    assert got['n_valid'].tolist() == [80 * 95 * 6, 320 * 95 * 6]


def test_identical_calls_give_identical_bytes():
    rng = np.random.default_rng(21)
    pos, neg = _rows(rng, 40, 101), _rows(rng, 200, 101)
    w = _table(N_NODES, 64)
    a, b = _run(w, pos, neg, 7), _run(w, pos, neg, 7)
    for k in ('loss', 'grad', 'n_valid', 'touched_count'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['touched'][:int(a['touched_count'][0])].tobytes() == b['touched'][:int(b['touched_count'][0])].tobytes()


def _toy_model(d=64, sparse=False, walk_length=10, context_size=4):
    from graph_recsys_benchmark_amd.models import MetaPath2Vec
    hin = walk_ref.toy_hin()
    model = MetaPath2Vec({k: torch.from_numpy(v) for k, v in hin['edge_index_dict'].items()}, d, hin['metapath'], walk_length,
                         context_size, hin['num_nodes_dict'], hin['types'], hin['type_accs'], walks_per_node=2,
                         num_negative_samples=3, sparse=sparse, seed=walk_ref.WALK_SEED).cuda()
    with torch.no_grad():
        model.embedding.weight.copy_(torch.from_numpy(_table(hin['num_nodes'], d, seed=4)))
    return model, hin


def test_windows_and_whole_walks_agree():
    model, hin = _toy_model()
    pos, neg = model.sample(torch.arange(40))
    assert tuple(pos.shape) == (80, 11) and tuple(neg.shape) == (240, 11) and bool((pos < 0).any())
    whole = model.loss(pos, neg)
    cut = model.loss(model.windows(pos), model.windows(neg))
    w = model.embedding.weight.detach().cpu().numpy()
    pw, nw = walk_ref.windows(pos.cpu().numpy(), 4), walk_ref.windows(neg.cpu().numpy(), 4)
    l32, _, _ = walk_ref.skipgram_loss(w, pw, nw, torch.float32)
    l64, _, _ = walk_ref.skipgram_loss(w, pw, nw, torch.float64)
    assert_fp32_close(np.array([whole.item()]), l32[:1], l64[:1], what='whole walks')
    assert_fp32_close(np.array([cut.item()]), l32[:1], l64[:1], what='windows')


def test_sparse_gradient_is_coalesced_and_equals_the_dense_rows():
    dense_model, _ = _toy_model(sparse=False)
    sparse_model, _ = _toy_model(sparse=True)
    pos, neg = dense_model.sample(torch.arange(40))
    dense, = torch.autograd.grad(dense_model.loss(pos, neg), dense_model.embedding.weight)
    sp, = torch.autograd.grad(sparse_model.loss(pos, neg), sparse_model.embedding.weight)
    assert sp.is_sparse and sp.is_coalesced() and not dense.is_sparse
    idx = sp._indices()[0]
    assert bool((idx[1:] > idx[:-1]).all())
    assert sp._values().cpu().numpy().tobytes() == dense[idx].cpu().numpy().tobytes()
    mask = torch.ones(dense.shape[0], dtype=torch.bool, device='cuda')
    mask[idx] = False
    assert not bool(dense[mask].any())
    sparse_model.loss(pos, neg).backward()                        # and through .grad, as the optimiser sees it
    g = sparse_model.embedding.weight.grad
    assert g.is_sparse and torch.equal(g.to_dense(), dense)
    torch.optim.SparseAdam(list(sparse_model.parameters()), lr=0.01).step()


def test_unsupported_shapes():
    from graph_recsys_benchmark_amd import _lib, engine
    lib = _lib.require_device()
    for d, t, c in ((6, 7, 7), (64, 6, 7), (64, 20, 17)):
        assert not engine.skipgram_supported(d, t, c)
        assert lib.pea_skipgram_workspace_bytes(2, 2, t, c, d) == 0
        w = torch.zeros((N_NODES, 8), device='cuda')
        rows = torch.zeros((2, 128), dtype=torch.int64, device='cuda')
        out = torch.zeros(4096, dtype=torch.float32, device='cuda')
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
        rc = lib.pea_skipgram_train(2, 2, t, c, d, _lib.ptr(w), 8, N_NODES, _lib.ptr(rows), 128, _lib.ptr(rows), 128, _lib.ptr(out),
                                    _lib.ptr(rows), _lib.ptr(out), _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(ws), ws.numel(),
                                    _lib.current_stream())
        assert rc == -1
    with pytest.raises(ValueError):
        engine.skipgram_train_raw(torch.zeros((N_NODES, 6), device='cuda'), torch.zeros((2, 7), dtype=torch.int64, device='cuda'),
                                  torch.zeros((2, 7), dtype=torch.int64, device='cuda'), 7)


def test_short_workspace_and_tape():
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.require_device()
    w = torch.zeros((N_NODES, 64), device='cuda')
    rows = torch.zeros((4, 11), dtype=torch.int64, device='cuda')
    loss, nv = torch.zeros(3, device='cuda'), torch.zeros(2, dtype=torch.int64, device='cuda')
    grad, touched = torch.zeros((N_NODES, 64), device='cuda'), torch.zeros(64, dtype=torch.int32, device='cuda')
    count = torch.zeros(1, dtype=torch.int32, device='cuda')
    flag = torch.ones(1, dtype=torch.int32, device='cuda')
    need = lib.pea_skipgram_workspace_bytes(4, 4, 11, 7, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')

    def call(ws_bytes):
        return lib.pea_skipgram_train(4, 4, 11, 7, 64, _lib.ptr(w), 64, N_NODES, _lib.ptr(rows), 11, _lib.ptr(rows), 11,
                                      _lib.ptr(loss), _lib.ptr(nv), _lib.ptr(grad), _lib.ptr(touched), _lib.ptr(count), _lib.ptr(flag),
                                      _lib.ptr(ws), ws_bytes, _lib.current_stream())
    assert need > 0 and call(need - 1) == -4 and call(need) == 0
    assert int(flag.item()) == 0                                   # cleared by the call
    tape = _lib.Tape()
    with tape.record():
        assert call(need) == -1
    assert len(tape) == 0


def test_queued_flag_owns_its_bytes_and_names_the_walks():
    """the flag a loss() call queues must not keep the step's workspace (the [rows * T, D] position gradients) alive, and a bad id
    surfaces as an IndexError that names the walks, at the model's forward() / eval()"""
    from graph_recsys_benchmark_amd import engine
    model, hin = _toy_model()
    engine.check_pending_errors()
    pos, neg = model.sample(torch.arange(40))
    model.loss(pos, neg).backward()
    flag = engine._pending_err[-1]
    assert flag.untyped_storage().nbytes() <= 64
    model('uid')                                                   # reads the flags: nothing raised
    assert not engine._pending_err
    bad = pos.clone()
    bad[0, 1] = hin['num_nodes'] + 5
    model.loss(bad, neg)
    with pytest.raises(IndexError, match='skip-gram walks'):
        model.eval()
    engine.check_pending_errors()                                  # consumed
