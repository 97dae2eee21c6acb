"""CPU: what tests/test_gpu_agg_bwd_matrix.py relies on, checked without a GPU.

1. The degree graph (helpers.degree_graph) really holds every listed degree as an in-degree and as an out-degree, with and
   without its self loops, duplicated edges, and sources of every row form that have no in-edge.
2. Headroom: the float32 form of the restatement (oracle/pyg_restatement.py under torch autograd), run on every case of the GPU
   matrix, stays within HALF of the gradient rule the GPU tests apply against float64 -- so a kernel that sums in another
   order has the other half, and a case that fails on the GPU is a finding about the kernel, not about the rule.  Worst
   measured fraction of the rule per kind: see the docstring of tests/test_gpu_agg_bwd_matrix.py."""
import numpy as np
import pytest
import torch

import helpers as H

LISTED = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 511, 512, 513)     # and one row of about 1100
HEADROOM = 0.5        # the share of the gradient rule the float32 restatement may use


def test_degree_graph_holds_every_listed_degree_on_both_sides():
    g = H.degree_graph()
    ei, n = g['edge_index'], g['n']
    assert ei.dtype == np.int64 and ei.shape[0] == 2 and 2000 <= n <= 3000 and n % 32 != 0
    assert ei.min() >= 0 and ei.max() < n
    loops = ei[0] == ei[1]
    assert loops.sum() >= 10                                                  # self loops in the input
    _, counts = np.unique(ei[:, ~loops], axis=1, return_counts=True)
    assert (counts > 1).sum() >= 50                                           # duplicated edges
    for drop in (True, False):                 # GAT / GCN plans drop the input's self loops, SAGE plans keep them
        deg_in, deg_out = H.kept_degrees(ei, n, drop)
        for side, deg in (('in', deg_in), ('out', deg_out)):
            for d in LISTED:
                assert (deg == d).any(), '%s-degree %d missing (self loops dropped: %s)' % (side, d, drop)
            assert deg.max() == 1100 and (deg == 1100).sum() == 2, side
        # rows of every form (short <= 32 < long <= 512 < hub) whose node has no edge at all on the other side: the S pass's
        # `lone` branch over the relation (no in-edge) and over its reverse (no out-edge)
        for mine, other in ((deg_out, deg_in), (deg_in, deg_out)):
            lone = mine[other == 0]
            assert ((lone >= 1) & (lone <= 32)).any() and ((lone > 32) & (lone <= 512)).any() and (lone > 512).any()
            for d in LISTED[1:] + (1100,):
                assert (lone == d).any() and (mine[other > 0] == d).any(), d
    # rows with a duplicated edge on both sides, in every row form
    deg_in, deg_out = H.kept_degrees(ei, n, True)
    pairs, counts = np.unique(ei[:, ~loops], axis=1, return_counts=True)
    for side, deg in ((1, deg_in), (0, deg_out)):
        d = deg[pairs[side][counts > 1]]
        assert (d <= 32).any() and ((d > 32) & (d <= 512)).any() and (d > 512).any()


def test_density_batches_produce_the_live_sets_they_name():
    g = H.degree_graph()
    n, hubs = g['n'], H.hub_nodes(g)
    assert hubs.size == 8                       # degrees 513 and 1100, lone and not, on either side
    live = {name: np.unique(H.density_batch(name, g)) for name in H.AGG_DENSITIES}
    assert live['one_triple'].size == 3
    assert live['two_percent'].size == n // 50
    assert np.array_equal(live['every_second'], np.arange(0, n, 2))
    assert np.array_equal(live['every_node'], np.arange(n))
    assert np.array_equal(live['hubs_only'], hubs)
    assert np.array_equal(live['all_but_hubs'], np.setdiff1d(np.arange(n), hubs))
    for name in H.AGG_DENSITIES:
        b = H.density_batch(name, g)
        assert b.dtype == np.int64 and b.ndim == 2 and b.shape[1] == 3 and 3 * b.shape[0] <= 16384


def test_the_conv_matrix_names_every_lane_width_and_head_class():
    ids = [c['id'] for c in H.AGG_CONV_CASES]
    assert len(set(ids)) == len(ids)
    seen = {(H.agg_lanes(c['heads'] * c['out']), H.agg_head_class(c['heads'], c['out'])) for c in H.AGG_CONV_CASES if c['kind'] == 'gat'}
    want = {(G, cls) for G in (4, 8, 16, 32, 64) for cls in ('full', 'four', 'generic')} - {(4, 'four')}     # at G = 4 'four' IS 'full'
    assert seen == want
    for G in (4, 8, 16, 32, 64):
        assert {c['slope'] for c in H.AGG_CONV_CASES if c['kind'] == 'gat' and H.agg_lanes(c['heads'] * c['out']) == G} == {0.0, 0.2, 1.0}
    assert {c['heads'] * c['out'] for c in H.AGG_CONV_CASES} >= {12, 20, 40, 96, 160}         # idle lanes in the last group
    assert {c['in_ch'] for c in H.AGG_CONV_CASES if c['kind'] != 'sage'} == {8, 36}
    for kind, width in (('gcn', 'out'), ('sage', 'in_ch')):           # the width each kind AGGREGATES at
        assert {H.agg_lanes(c[width]) for c in H.AGG_CONV_CASES if c['kind'] == kind} == {4, 8, 16, 32, 64}
    # the flagged last layer (repr_dim wide) at every lane width, on both routes of model.loss
    assert {H.agg_lanes(c[3]) for c in H.AGG_MODEL_CASES if c[0] == 'gat'} == {4, 8, 16, 32, 64}
    assert {H.agg_lanes(c[3]) for c in H.AGG_MODEL_CASES if c[0] == 'gcn'} == {4, 8, 16, 32, 64}
    assert len(set(H.AGG_MODEL_IDS)) == len(H.AGG_MODEL_IDS)


def test_the_gradient_rule_does_not_lose_a_nan():
    want = {k: np.ones(3) for k in ('x', 'w', 'b')}
    near = lambda: {k: v + 1e-5 for k, v in want.items()}
    frac, name = H.grad_rule_fraction(near(), want)
    assert 0.0 < frac <= 1.0 and name in want
    for bad in want:                             # first, middle, last tensor: the fraction must fail every `<=`
        for poison in (np.nan, np.inf):
            got = near()
            got[bad][0] = poison
            frac, name = H.grad_rule_fraction(got, want)
            assert name == bad and not frac <= 1.0 and not frac <= HEADROOM
    got = near()
    got['w'][1] += 1.0
    frac, name = H.grad_rule_fraction(got, want)
    assert name == 'w' and frac > 1000


def test_the_restated_loss_is_the_one_test_gpu_backward_uses():
    """helpers.restated_loss_and_grads restates f64_loss_and_grads with the dtype left open: in float64 they are the same numbers"""
    from test_gpu_backward import f64_loss_and_grads
    g = H.degree_graph()
    for kind, heads, channels in (('gat', 2, 2), ('gcn', 1, 1), ('sage', 1, 2)):
        _, sd = H.agg_model_state(kind, heads, 24, 12, channels, g)
        edges, batch = H.agg_model_edges(g, channels), H.density_batch('two_percent', g)
        l0, g0 = f64_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch)
        l1, g1 = H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch)
        assert l0 == l1 and set(g0) == set(g1)
        for k in g0:
            np.testing.assert_array_equal(g0[k], g1[k], err_msg=k)


_worst = {}


def _note(kind, frac, what):
    if frac > _worst.get(kind, (0.0, ''))[0]:
        _worst[kind] = (frac, what)
    print('float32 restatement uses %.3f of the rule (%s); worst so far per kind: %s' % (frac, what, _worst))


@pytest.mark.parametrize('case', H.AGG_CONV_CASES, ids=[c['id'] for c in H.AGG_CONV_CASES])
def test_float32_headroom_of_the_single_conv_cases(case):
    g = H.degree_graph()
    _, want = H.conv_reference(case, g, torch.float64)
    _, got = H.conv_reference(case, g, torch.float32)
    frac, name = H.grad_rule_fraction(got, want)
    _note(case['kind'], frac, name)
    assert frac <= HEADROOM, '%s: the float32 restatement already uses %.2f of the rule' % (name, frac)


@pytest.mark.parametrize('kind,heads,hidden,repr_dim,channels,density', H.AGG_MODEL_CASES, ids=H.AGG_MODEL_IDS)
def test_float32_headroom_of_the_row_flag_cases(kind, heads, hidden, repr_dim, channels, density):
    g = H.degree_graph()
    _, sd = H.agg_model_state(kind, heads, hidden, repr_dim, channels, g)
    edges, batch = H.agg_model_edges(g, channels), H.density_batch(density, g)
    l64, want = H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch)
    l32, got = H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch, dtype=torch.float32)
    frac, name = H.grad_rule_fraction(got, want)
    _note(kind + ' model', frac, name)
    assert abs(l32 - l64) <= 0.5 * 2e-5 * abs(l64)
    assert frac <= HEADROOM, '%s: the float32 restatement already uses %.2f of the rule' % (name, frac)


@pytest.mark.parametrize('case', H.AGG_COLSUM_CASES, ids=H.AGG_COLSUM_IDS)
def test_float32_headroom_of_the_colsum_cases(case):
    _, sd, n, edges, batch = H.colsum_case(*case)
    l64, want = H.restated_loss_and_grads(case[0], sd, edges, [2] * case[4], case[1], 'att', batch)
    l32, got = H.restated_loss_and_grads(case[0], sd, edges, [2] * case[4], case[1], 'att', batch, dtype=torch.float32)
    frac, name = H.grad_rule_fraction(got, want)
    _note('colsum', frac, name)
    assert abs(l32 - l64) <= 0.5 * 2e-5 * abs(l64)
    assert frac <= HEADROOM, '%s: the float32 restatement already uses %.2f of the rule' % (name, frac)
