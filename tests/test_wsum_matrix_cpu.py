"""CPU: what tests/test_gpu_wsum_matrix.py relies on, checked without a GPU.

1. The graph (helpers.wsum_graph: degree_graph without its self loops) still holds every listed degree as an in-degree and as
   an out-degree, so pea_weighted_aggregate's forward (relation 0) and backward (relation 1, the reverse) both meet every row form.
2. The width list reaches every cell of helpers.WSUM_CELLS: every lane width G alone with full and with idle lanes, 2, 3, 4 and 17
   column groups; taking a width away names the cell it leaves empty.
3. The comparison has room: the float32 form of the restatement (index_add_ in COO order), and a second float32 order (edges
   sorted by destination, np.add.reduceat), pass helpers.assert_fp32_close against float64 for every width and both directions.
4. The exact inputs are exact: float32 equals float64 bit for bit and no partial sum can reach 2^24.
5. The comparison notices: weights taken in CSR-slot order, and the last edge of a 1100-edge row left out, each fail the exact
   comparison and assert_fp32_close.  (No deliberately wrong kernel is ever run on a GPU; this is the evidence instead.)
6. The float32 form of the KGAT / KGCN / NGCF restatement uses at most half of the gradient rule the GPU test applies.

Measured here, largest row error against float64 in float32 ulps of the row's magnitude (helpers.row_ulps), forward / backward:

    width    index_add_ order    reduceat order          width    index_add_ order    reduceat order
    4        18.2 / 28.1         6.7 / 7.6               132      14.1 / 18.6         3.5 / 3.2
    12       14.3 / 12.9         3.1 / 3.2               160      25.0 / 12.2         23.5 / 3.9
    16       12.0 / 22.2         4.1 / 3.7               256      15.0 / 14.2         4.2 / 2.9
    20       18.7 / 18.0         3.9 / 4.0               260      16.9 / 15.2         3.7 / 3.3
    32       19.1 / 15.0         3.0 / 3.4               320      17.3 / 14.8         2.8 / 3.7
    36       12.1 / 15.2         9.5 / 4.0               512      26.9 / 17.8         2.8 / 3.8
    40       23.3 / 12.4         3.0 / 3.0               600      23.7 / 17.4         3.0 / 3.9
    64       19.7 / 14.1         3.2 / 3.9               772      16.4 / 19.1         3.5 / 3.1
    96       19.8 / 13.1         3.6 / 3.6               4100     23.7 / 21.1         4.3 / 4.3
    128      14.2 / 15.3         3.8 / 3.8

Over all widths the index_add_ order is at most 28.1 ulp off float64 and the reduceat order at most 23.5 (9.5 but for one row of
width 160).  Every case passes assert_fp32_close with `want` = `truth` = float64, so without any allowance for an oracle error, but
few on its first tier (helpers.fp32_tier): an element of a sum of 1100 terms that cancels to near nothing misses rtol 1e-5 of
itself in either order.  The reduceat order passes on the per-row tier (16 ulp of the row + atol) everywhere, the index_add_ order
needs the two-sided tier at the end of assert_fp32_close in 17 of the 38 comparisons (a few rows between 16 and 28 ulp).  With one
order as `want` and the other as the stand-in for the kernel every comparison passes as well, which is how the GPU tests compare.
KG convs, float32 restatement against float64: 0.002 to 0.005 of the gradient rule from run to run (the float32 sums of the dense
products depend on the thread count), outputs 8.5 to 11.3 ulp; the parameter scale 0.3 needed no shrinking."""
import numpy as np
import pytest
import torch

import helpers as H

HEADROOM = 0.5        # the share of the gradient rule the float32 restatement may use
ISSUE_WIDTHS = (4, 12, 16, 20, 32, 36, 40, 64, 96, 128, 132, 160, 256, 260, 320, 512, 772, 4100)
CASES = H.wsum_cases()
IDS = [i for _, i in CASES]


def test_wsum_graph_keeps_every_listed_degree_on_both_sides():
    g, full = H.wsum_graph(), H.degree_graph()
    ei, n = g['edge_index'], g['n']
    assert H.wsum_graph() is g                                              # cached
    assert n == 2076 and ei.shape == (2, 15856) and ei.dtype == np.int64 and ei.flags['C_CONTIGUOUS']
    assert full['edge_index'].shape[1] - ei.shape[1] == 40 and not (ei[0] == ei[1]).any()
    assert ei.min() >= 0 and ei.max() < n
    _, counts = np.unique(ei, axis=1, return_counts=True)
    assert int((counts - 1).sum()) == 230                                   # edges that repeat an earlier one
    deg_in, deg_out = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
    for side, deg in (('in', deg_in), ('out', deg_out)):
        for d in H.AGG_DEGREES:
            assert (deg == d).any(), '%s-degree %d missing' % (side, d)
        assert deg.max() == 1100 and (deg == 1100).sum() == 2, side
    # a duplicated edge in a short, a long and a hub row on both sides: a weight on the wrong copy shows in every row form
    pairs, counts = np.unique(ei, axis=1, return_counts=True)
    for side, deg in ((1, deg_in), (0, deg_out)):
        d = deg[pairs[side][counts > 1]]
        assert (d <= 32).any() and ((d > 32) & (d <= 512)).any() and (d > 512).any()


def test_the_width_list_reaches_every_cell():
    # 772 = 3 x 256 + 4 makes FOUR column groups (c = 0, 256, 512, 768), so 600 stands beside it for three
    assert tuple(w for w, _ in CASES) == H.WSUM_WIDTHS == tuple(sorted(ISSUE_WIDTHS + (600,)))
    assert len(set(IDS)) == len(IDS)
    H.check_wsum_cells()
    want_ids = {4: 'G4-groups1-w4', 20: 'G8-groups1-w20', 40: 'G16-groups1-w40', 96: 'G32-groups1-w96', 256: 'G64-groups1-w256',
                260: 'G64+4-groups2-w260', 320: 'G64+16-groups2-w320', 512: 'G64-groups2-w512', 600: 'G64+32-groups3-w600',
                772: 'G64+4-groups4-w772',
                4100: 'G64+4-groups17-w4100'}
    assert {w: i for w, i in CASES if w in want_ids} == want_ids
    assert {len(H.wsum_groups(w)) for w in H.WSUM_WIDTHS} == {1, 2, 3, 4, H.WSUM_MAX_GROUPS + 1}
    assert {H.agg_lanes(w) for w in H.WSUM_WIDTHS if w <= 256} == {4, 8, 16, 32, 64}
    for G in (8, 16, 32, 64):                                                # an idle-lane width per G >= 8
        assert any(H.agg_lanes(w) == G and w < 4 * G for w in H.WSUM_WIDTHS if w <= 256), G
    assert H.wsum_groups(260) == [256, 4] and H.wsum_groups(600) == [256, 256, 88] and H.wsum_groups(772) == [256, 256, 256, 4] and len(H.wsum_groups(4100)) == 17
    assert {H.agg_lanes(w) for w in H.WSUM_CHUNK64_WIDTHS if w <= 256} == {4, 8, 16, 32, 64} and 260 in H.WSUM_CHUNK64_WIDTHS
    # every width is needed, or shares its cell with one named neighbour that differs in the number of idle lanes
    shared = {4: 12, 12: 4, 36: 40, 40: 36, 132: 160, 160: 132}
    for w in H.WSUM_WIDTHS:
        rest = tuple(v for v in H.WSUM_WIDTHS if v != w)
        if w in shared:
            assert H.wsum_cells((w,)) == H.wsum_cells((shared[w],))
            H.check_wsum_cells(rest)
            with pytest.raises(AssertionError, match=r'\(G = %d, groups = 1\)' % H.agg_lanes(w)):
                H.check_wsum_cells(tuple(v for v in rest if v != shared[w]))
        else:
            G, groups = H.agg_lanes(H.wsum_groups(w)[-1]), len(H.wsum_groups(w))
            with pytest.raises(AssertionError, match=r'\(G = %d, groups = %d\)' % (G, groups)):
                H.check_wsum_cells(rest)


def _by_destination(width, reverse, wrong=None):
    """The same sum in float32 in another order: edges sorted by the row they are added to, np.add.reduceat over each row's run.
    wrong = 'slot': the weight of CSR slot s is w[s] instead of w[eid[s]]; wrong = 'last': the last slot of the first 1100-edge
    row is left out."""
    g = H.wsum_graph()
    x, w, gout = H.wsum_inputs(width)
    return _reduceat(g, gout if reverse else x, w, reverse, wrong)


def _reduceat(g, feat, w, reverse, wrong=None):
    ei, n = g['edge_index'], g['n']
    gather, scatter = (ei[1], ei[0]) if reverse else (ei[0], ei[1])
    eid = np.argsort(scatter, kind='stable')                                # CSR slot -> COO edge
    ws = w[eid] if wrong != 'slot' else w[:eid.size].copy()
    deg = np.bincount(scatter, minlength=n)
    starts = np.concatenate([[0], np.cumsum(deg)[:-1]])
    if wrong == 'last':
        row = int(np.flatnonzero(deg == 1100)[0])
        ws = ws.copy()
        ws[starts[row] + 1099] = 0.0
    msgs = feat[gather[eid]] * ws[:, None]
    out = np.zeros((n, feat.shape[1]), feat.dtype)
    rows = np.flatnonzero(deg > 0)
    out[rows] = np.add.reduceat(msgs, starts[rows], axis=0)
    return out


@pytest.mark.parametrize('width,case_id', CASES, ids=IDS)
def test_float32_in_two_orders_fits_the_rule(width, case_id):
    for reverse in (False, True):
        what = '%s %s' % (case_id, 'backward' if reverse else 'forward')
        r32 = H.wsum_reference(width, reverse, torch.float32)
        r64 = H.wsum_reference(width, reverse, torch.float64)
        p32 = _by_destination(width, reverse)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and p32.dtype == np.float32 and r32.shape == (2076, width)
        assert H.wsum_reference(width, reverse, torch.float32) is r32       # cached
        print('%s: index_add_ %.1f ulp %s, reduceat %.1f ulp %s' % (what, H.row_ulps(r32, r64), H.fp32_tier(r32, r64, r64),
                                                                    H.row_ulps(p32, r64), H.fp32_tier(p32, r64, r64)))
        # each order against float64 alone, then each as the kernel's stand-in against the other as the oracle
        H.assert_fp32_close(r32, r64, r64, what=what + ' index_add_')
        H.assert_fp32_close(p32, r64, r64, what=what + ' reduceat')
        H.assert_fp32_close(p32, r32, r64, what=what + ' reduceat against index_add_')
        H.assert_fp32_close(r32, p32, r64, what=what + ' index_add_ against reduceat')
        deg = np.bincount(H.wsum_graph()['edge_index'][0 if reverse else 1], minlength=2076)
        assert not r32[deg == 0].any() and not r64[deg == 0].any() and r64[deg > 0].any(axis=1).all()


@pytest.mark.parametrize('width,case_id', CASES, ids=IDS)
def test_exact_inputs_are_exact(width, case_id):
    g = H.wsum_graph()
    x, w, gout = H.wsum_inputs(width, exact=True)
    for a, top in ((x, 8), (gout, 8), (w, 4)):
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() == top
    assert (w != 0).all() and set(np.unique(w)) == {-4, -3, -2, -1, 1, 2, 3, 4}
    for reverse in (False, True):
        r32 = H.wsum_reference(width, reverse, torch.float32, exact=True)
        r64 = H.wsum_reference(width, reverse, torch.float64, exact=True)
        assert np.array_equal(r32, r64) and np.array_equal(r64, np.round(r64))
        assert np.array_equal(_reduceat(g, gout if reverse else x, w, reverse), r64)
        # no order of additions can leave the integers float32 holds exactly: the sum of the magnitudes bounds every partial sum
        feat, (gather, scatter) = (gout if reverse else x), ((1, 0) if reverse else (0, 1))
        bound = np.zeros(g['n'])
        np.add.at(bound, g['edge_index'][scatter], np.abs(w).astype(np.float64) * np.abs(feat).max(axis=1)[g['edge_index'][gather]])
        assert bound.max() <= 1100 * 32 < 2 ** 24 and np.abs(r64).max() <= bound.max()


@pytest.mark.parametrize('wrong', ['slot', 'last'], ids=['weights_in_slot_order', 'last_edge_of_1100_dropped'])
@pytest.mark.parametrize('width', [12, 260])
def test_the_comparisons_notice_a_wrong_sum(width, wrong):
    g = H.wsum_graph()
    for reverse in (False, True):
        r32, r64 = H.wsum_reference(width, reverse, torch.float32), H.wsum_reference(width, reverse, torch.float64)
        H.assert_fp32_close(_by_destination(width, reverse), r32, r64)                      # the same code without the fault passes
        bad = _by_destination(width, reverse, wrong)
        rows = np.flatnonzero((bad != _by_destination(width, reverse)).any(axis=1))
        assert rows.size == 1 if wrong == 'last' else rows.size > 1000
        with pytest.raises(AssertionError):
            H.assert_fp32_close(bad, r32, r64)
        x, w, gout = H.wsum_inputs(width, exact=True)
        e64 = H.wsum_reference(width, reverse, torch.float64, exact=True)
        assert np.array_equal(_reduceat(g, gout if reverse else x, w, reverse), e64)
        assert not np.array_equal(_reduceat(g, gout if reverse else x, w, reverse, wrong), e64)


@pytest.mark.parametrize('kind', sorted(H.KG_CONV_PARAMS))
def test_float32_headroom_of_the_kg_convs(kind):
    out64, want = H.kg_conv_reference(kind, torch.float64)
    out32, got = H.kg_conv_reference(kind, torch.float32)
    assert set(want) == {'x'} | set(H.KG_CONV_PARAMS[kind]) and out64.shape == (2076, H.KG_CONV_OUT)
    x, params, att, gout = H.kg_conv_tensors(kind)
    seg = np.zeros(2076)
    np.add.at(seg, H.wsum_graph()['edge_index'][1], att.numpy().astype(np.float64))
    assert np.abs(seg[seg > 0] - 1.0).max() < 1e-6 and (att.numpy() > 0).all()          # att_map is a softmax per destination
    frac, name = H.grad_rule_fraction(got, want)
    print('%s: the float32 restatement uses %.3f of the gradient rule (%s); out %.1f ulp' % (kind, frac, name, H.row_ulps(out32, out64)))
    H.assert_fp32_close(out32, out64, out64, what=kind + ' out')
    assert frac <= HEADROOM, '%s: the float32 restatement already uses %.2f of the rule' % (name, frac)
