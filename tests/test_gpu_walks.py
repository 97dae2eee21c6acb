"""GPU: the device walks of csrc/walk.hip against their numpy restatement (tests/walk_ref.py), bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import walk_ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def _toy_plan():
    """(hin, GraphPlan over the flipped COOs of the toy metapath, its relation per step, the plan's own CSRs as numpy)"""
    if 'plan' not in _CACHE:
        from graph_recsys_benchmark_amd.engine import GraphPlan
        hin = walk_ref.toy_hin()
        flipped = [torch.from_numpy(np.ascontiguousarray(hin['edge_index_dict'][k][::-1])).cuda() for k in hin['metapath']]
        plan = GraphPlan(hin['num_nodes'], [flipped], self_loops=False)
        csrs = [tuple(t.cpu().numpy() for t in plan.export_csr(r)) for r in range(plan.num_relations)]
        _CACHE['plan'] = (hin, plan, list(plan.relation_of[0]), csrs)
    return _CACHE['plan']


@pytest.mark.parametrize('offset', [0, 7])
@pytest.mark.parametrize('seed', [walk_ref.WALK_SEED, 99])
@pytest.mark.parametrize('n_walks', [63, 273])
@pytest.mark.parametrize('walk_length', [10, 3])
def test_metapath_walks_match_the_restatement(walk_length, n_walks, seed, offset):
    from graph_recsys_benchmark_amd import engine
    hin, plan, rel, csrs = _toy_plan()
    starts = np.tile(np.arange(hin['num_nodes_dict']['uid']), 7)[:n_walks].astype(np.int64)
    starts[n_walks // 2] = hin['num_nodes'] + 3                          # one start outside the graph
    got, status = engine.metapath_walks(plan, rel, torch.from_numpy(starts).cuda(), walk_length, seed, offset, return_status=True)
    want, want_status = walk_ref.metapath_walks(csrs, rel, starts, walk_length, seed, offset, hin['num_nodes'])
    assert got.dtype == torch.int64 and tuple(got.shape) == (n_walks, walk_length + 1)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert status.cpu().tolist() == want_status and want_status[1] == 1
    if n_walks == 273:
        assert want_status[0] > 0 and (want[:, -1] >= 0).sum() > n_walks // 2
    with pytest.raises(IndexError):
        engine.metapath_walks(plan, rel, torch.from_numpy(starts).cuda(), walk_length, seed, offset, validate=True)


def test_plan_csr_is_the_csr_of_the_flipped_coo():
    """the adjacency the comparison above uses is the one a walk along the reference's direction needs"""
    hin, plan, rel, csrs = _toy_plan()
    for step, keys in enumerate(hin['metapath']):
        rowptr, col = walk_ref.csr_of(hin['edge_index_dict'][keys], hin['num_nodes'])
        np.testing.assert_array_equal(csrs[rel[step]][0], rowptr)
        np.testing.assert_array_equal(csrs[rel[step]][1], col)


@pytest.mark.parametrize('n_walks,walk_length', [(63, 10), (273, 3)])
def test_uniform_walks_match_the_restatement(n_walks, walk_length):
    from graph_recsys_benchmark_amd import engine
    lo, n = [40, 70, 40, 0], [30, 5, 30, 40]
    starts = (np.arange(n_walks) % 40).astype(np.int64)
    got = engine.uniform_walks(lo, n, torch.from_numpy(starts).cuda(), walk_length, walk_ref.WALK_SEED, 5).cpu().numpy()
    np.testing.assert_array_equal(got, walk_ref.uniform_walks(lo, n, starts, walk_length, walk_ref.WALK_SEED, 5))
    for t in range(1, walk_length + 1):
        s = (t - 1) % 4
        assert ((got[:, t] >= lo[s]) & (got[:, t] < lo[s] + n[s])).all()


def test_step_distribution_counts_multi_edges():
    """node 0 has 50 distinct neighbours and one of them twice: 51 slots, the doubled neighbour drawn twice as often"""
    from graph_recsys_benchmark_amd import engine
    from graph_recsys_benchmark_amd.engine import GraphPlan
    nbrs = np.arange(1, 51)
    coo = np.stack([np.concatenate([nbrs, [17]]), np.zeros(51, dtype=np.int64)]).astype(np.int64)    # source j -> target 0
    plan = GraphPlan(51, [[torch.from_numpy(coo).cuda()]], self_loops=False)
    n = 20000
    walks = engine.metapath_walks(plan, [0], torch.zeros(n, dtype=torch.int64, device='cuda'), 1, 1234, 0).cpu().numpy()
    counts = np.bincount(walks[:, 1], minlength=51)[1:]
    expect = np.full(50, n / 51.0)
    expect[16] *= 2
    assert (np.abs(counts - expect) < 6 * np.sqrt(expect)).all() and counts.sum() == n


def test_argument_errors():
    from graph_recsys_benchmark_amd import _lib, engine
    from graph_recsys_benchmark_amd.engine import GraphPlan
    hin, plan, rel, _ = _toy_plan()
    lib = _lib.require_device()
    starts = torch.zeros(4, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.PeaError):
        engine.metapath_walks(plan, [0, plan.num_relations], starts, 4, 1, 0)            # a relation outside the plan
    walks = torch.empty((4, 5), dtype=torch.int64, device='cuda')
    status = torch.zeros(2, dtype=torch.int32, device='cuda')
    one = (C.c_int * 1)(0)
    rc = lib.pea_metapath_walks(plan._h, 1, one, 5, 4, _lib.ptr(starts), 1, 0, _lib.ptr(walks), 5, _lib.ptr(status),
                                _lib.current_stream())
    assert rc == -1                                                                       # ld < walk_length + 1
    ei = torch.from_numpy(hin['edge_index_dict'][hin['metapath'][0]]).cuda()
    looped = GraphPlan(hin['num_nodes'], [[ei]], self_loops=True)
    with pytest.raises(_lib.PeaError):
        engine.metapath_walks(looped, [0], starts, 4, 1, 0)
    with pytest.raises(_lib.PeaError):
        engine.uniform_walks([0], [0], starts, 4, 1, 0)                                   # an empty block
