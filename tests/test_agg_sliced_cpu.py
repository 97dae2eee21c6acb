"""CPU: what tests/test_gpu_agg_sliced_matrix.py relies on, checked without a GPU.

1. Slice counts: helpers.slice_count, the hand restatement of build_relation's slice decision (csrc/plan.hip), gives the S
   every shape of helpers.AGG_SLICED_SHAPES names under the shape's knobs -- for the relation and its reverse, self loops
   dropped and kept -- and 1 with the knobs unset.
2. Cell coverage: helpers.AGG_SLICED_CASES holds every (kind, lane width) cell and the two extra GAT head classes.
3. Layouts: which degrees each shape cuts per slice, the plain hub row inside the sliced `s32` plan, the record counts that give
   the merges a second trip, a shape that pads and one that does not, and helpers.es_sliced_bins unchanged.
4. Headroom: the float32 restatement with the edges visited in (destination, slice) order uses at most HALF of the gradient rule
   and passes assert_fp32_close, on every case and shape: a failure on the GPU is then the kernel's, not float32's.
5. The integer recipe of test_sliced_equals_unsliced_on_integers is exact: float32 equals float64, in plain and in sliced edge
   order, and every chunk record of every cut row of the reverse relation gathers a row that carries a gradient.
6. Two wrong restatements -- the last chunk record of the 1100-edge row left out; one slice's segment of that row added to the
   neighbouring hub row -- fail the integer comparison, the gradient rule and assert_fp32_close."""
import numpy as np
import pytest
import torch

import helpers as H

HEADROOM = 0.5        # the share of the gradient rule the float32 restatement may use
SHAPES = list(H.AGG_SLICED_SHAPES)
CASE_IDS = [c['id'] for c in H.AGG_SLICED_CASES]
SAGE_CASES = [c for c in H.AGG_SLICED_CASES if c['kind'] == 'sage']
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sides(graph):
    """(self loops dropped, reverse, kept edges) of the four relations a shape plans"""
    return [(drop, rev, H.kept_edges(graph['edge_index'], drop, rev)) for drop in (True, False) for rev in (False, True)]


def _bins(shape):
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    return _cached(('bins', shape), lambda: [H.sliced_plan_bins(k, g['n'], sh['chunk'], 32, sh['slices']) for _, _, k in _sides(g)])


@pytest.mark.parametrize('shape', SHAPES)
def test_slice_count_gives_the_shapes_slices(shape):
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    assert sh['env']['PEA_SLICE_MIN_EDGES'] == '1' and set(sh['env']) <= set(H.AGG_SLICED_KNOBS)
    assert int(sh['env'].get('PEA_CHUNK', 512)) == sh['chunk']
    for drop, rev, kept in _sides(g):
        span = int(kept[0].max()) - int(kept[0].min()) + 1
        got = H.slice_count(span, H.CONV_ROW_BYTES, kept.shape[1], int(sh['env']['PEA_SLICE_MIN_EDGES']), float(sh['env']['PEA_SLICE_BYTES']))
        assert got == sh['slices'], (drop, rev, span)
        assert H.slice_count(span, H.CONV_ROW_BYTES, kept.shape[1]) == 1                  # the knobs unset: a small graph is never sliced
        assert H.slice_count(span, 0, kept.shape[1], 1, float(sh['env']['PEA_SLICE_BYTES'])) == 1      # no row size, no slices


def test_slice_count_thresholds():
    sb = 1000.0
    assert H.slice_count(6, 250, 10, 10, sb) == 1 and H.slice_count(7, 250, 10, 10, sb) == 8          # 1.5 slices' worth, strictly more
    assert H.slice_count(7, 250, 9, 10, sb) == 1                                                    # too few edges
    assert [H.slice_count(s, 250, 10, 10, sb) for s in (32, 33, 64, 65, 224, 225, 100000)] == [8, 16, 16, 24, 56, 64, 64]
    assert H.slice_count(2 * 10 ** 6, 256, 24800000) == 64 and H.slice_count(40000, 256, 24800000) == 8      # the defaults (6 MB slices)
    assert H.slice_count(30000, 256, 24800000) == 1 and H.slice_count(40000, 256, 1999999) == 1


def test_sliced_cases_hold_every_cell():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    cells = {(c['kind'], H.agg_case_lanes(c)) for c in H.AGG_SLICED_CASES}
    missing = {(k, G) for k in ('gat', 'gcn', 'sage') for G in (4, 8, 16, 32, 64)} - cells
    assert not missing, 'no case for %s' % sorted(missing)
    gat16 = {H.agg_head_class(c['heads'], c['out']) for c in H.AGG_SLICED_CASES if c['kind'] == 'gat' and H.agg_case_lanes(c) >= 16}
    assert gat16 == {'full', 'four', 'generic'}
    assert set(c['id'] for c in H.AGG_CHUNK64_CASES) <= set(CASE_IDS)
    assert {c['deg'] for c in H.AGG_SLICED_CASES if c['kind'] == 'gcn'} == {'row', 'col'}
    assert len(SAGE_CASES) == 5


@pytest.mark.parametrize('shape', SHAPES)
def test_layout_of_the_shape(shape):
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    n = g['n']
    for (drop, rev, kept), b in zip(_sides(g), _bins(shape)):
        deg = np.bincount(kept[1], minlength=n)
        # a degree of AGG_DEGREES sits on two rows of either side (one of them `lone`), the big graph's own degrees on one
        assert b['sliced_degrees'] == sorted(d for d in sh['cut'] for _ in range(2 if d in H.AGG_DEGREES else 1))
        cut, records = H.sliced_plan_items(kept, n, sh['chunk'], 32, sh['slices'])
        plain = sorted({int(deg[r]) for r in records if not cut[r]})
        assert plain == sorted(sh['hub']), plain
        assert b['hub_rows'] == len(records) and b['hub_slots'] == sum(len(r) for r in records.values())
        for row, recs in records.items():           # the records tile the row, in order, none longer than the chunk size or empty
            assert [f for _, f, _ in recs] == list(np.cumsum([0] + [ln for _, _, ln in recs])[:-1])
            assert sum(ln for _, _, ln in recs) == deg[row] and all(0 < ln <= sh['chunk'] for _, _, ln in recs)
            if cut[row]:
                assert [s for s, _, _ in recs] == sorted(s for s, _, _ in recs) and len({s for s, _, _ in recs}) > 1
        # the head of the item list: whole rounds of 8 slices x 4 items per phase
        head = b['pad_items'] + sum(len(records[r]) for r in records if cut[r])
        assert head % 32 == 0 and head >= 32 * (sh['slices'] // 8) and b['pad_items'] >= 0
        unsliced = H.es_plan_bins(deg, sh['chunk'])
        assert b['long_items'] == unsliced['long_items'] - sum(len(unsliced['chunks'][int(deg[r])]) for r in records if cut[r]) + head
        assert {k: b[k] for k in ('edges', 'max_degree', 'short_rows')} == {k: unsliced[k] for k in ('edges', 'max_degree', 'short_rows')}


def test_layouts_reach_what_the_table_names():
    bins = {shape: _bins(shape) for shape in SHAPES}
    # s8 fills its one round exactly (4 rows x 8 slices), s32 / s64_big / the small-chunk shapes leave padding items
    assert all(b['pad_items'] == 0 for b in bins['s8']) and all(b['pad_items'] == 0 for b in bins['s16'])
    assert all(b['pad_items'] > 0 for shape in ('s32', 's8_chunk64', 's8_chunk8', 's64_big') for b in bins[shape])
    assert all(b['hub_records'] == 8 for b in bins['s8']) and all(b['hub_records'] == 16 for b in bins['s16'])
    # s32: the 513-edge rows stay plain two-chunk hub rows inside a plan of 32 slices
    assert H.AGG_SLICED_SHAPES['s32']['hub'] == (513,) and all(b['hub_rows'] == 4 and len(b['sliced_degrees']) == 2 for b in bins['s32'])
    # chunk records of the busiest row against the merges' trips: agg_bwd.hip folds 8 records per trip, agg.hip 8 x 64 / G.
    # chunks of 64 edges give the 1100-edge row 23 records (8 slices x 3, one segment of 2): a second trip of every backward
    # merge and of the forward merge at G = 32 and 64; chunks of 8 give it 141: a second forward trip at every G
    assert all(b['hub_records'] == 23 for b in bins['s8_chunk64'])
    assert all(b['hub_records'] > 8 * 64 // 4 for b in bins['s8_chunk8'])
    assert all(b['hub_records'] == 64 for b in bins['s64_big'])                 # 4200 edges, one chunk in each of 64 slices
    # s64_big: eight phases, 2047 edges stay below 64 x 32
    assert H.AGG_SLICED_SHAPES['s64_big']['slices'] == 64 and 2047 in H.AGG_SLICED_SHAPES['s64_big']['hub']
    g = H.agg_big_graph()
    assert 6400 <= g['n'] <= 6600
    for drop in (True, False):
        deg_in, deg_out = H.kept_degrees(g['edge_index'], g['n'], drop)
        for deg in (deg_in, deg_out):
            assert all((deg == d).sum() == 1 for d in (2047, 2048, 2049, 4200)) and deg.max() == 4200
            assert all((deg == d).sum() == 2 for d in (513, 1100))


def test_one_phase_bins_are_the_edge_softmax_matrix_bins():
    ei, n = H.es_graph()['edge_index'], H.es_graph()['n']
    for chunk in (512, 256):
        a, b = H.es_sliced_bins(ei, n, chunk=chunk), H.sliced_plan_bins(ei, n, chunk, 32, 8)
        assert a == b
    # the numbers tests/test_es_matrix_cpu.py and tests/test_gpu_es_matrix.py pin
    assert {k: H.es_sliced_bins(ei, n)[k] for k in ('long_items', 'hub_rows', 'hub_slots', 'pad_items')} == dict(
        long_items=55, hub_rows=4, hub_slots=32, pad_items=0)
    assert {k: H.es_sliced_bins(ei, n, chunk=256)[k] for k in ('long_items', 'hub_rows', 'hub_slots', 'pad_items')} == dict(
        long_items=114, hub_rows=9, hub_slots=72, pad_items=24)
    deg = np.bincount(ei[1], minlength=n)
    plain = H.es_plan_bins(deg)
    one = H.sliced_plan_bins(ei, n, 512, 32, 1)
    assert {k: one[k] for k in plain if k != 'chunks'} == {k: plain[k] for k in plain if k != 'chunks'} and one['pad_items'] == 0


def test_sliced_csr_is_a_stable_sort_by_destination_and_slice():
    g = H.degree_graph()
    kept = H.kept_edges(g['edge_index'], True)
    rowptr, col, order = H.sliced_csr(kept, g['n'], 8)
    sl = H.edge_slices(kept[0], 8)
    assert sl.min() == 0 and sl.max() == 7
    key = kept[1][order] * 8 + sl[order]
    assert (np.diff(key) >= 0).all() and all((np.diff(order[key == k]) > 0).all() for k in np.unique(key)[:200])
    assert rowptr[-1] == kept.shape[1] and np.array_equal(np.diff(rowptr), np.bincount(kept[1], minlength=g['n']))
    p1, c1, o1 = H.sliced_csr(kept, g['n'], 1)
    assert np.array_equal(o1, np.argsort(kept[1], kind='stable')) and np.array_equal(p1, rowptr) and not np.array_equal(c1, col)


# ---------------------------------------------------------------------------------------------------------------------
# headroom
# ---------------------------------------------------------------------------------------------------------------------
_worst = {}


def _truth(case, graph):
    return _cached(('f64', case['id'], graph['n']), lambda: H.conv_reference(case, graph, torch.float64))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', H.AGG_SLICED_CASES, ids=CASE_IDS)
def test_float32_headroom_in_sliced_edge_order(case, shape):
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    out64, want = _truth(case, g)
    out_plain = _cached(('f32', case['id'], g['n']), lambda: H.conv_reference(case, g, torch.float32))[0]
    ordered = H.slice_ordered_graph(g, sh['slices'], case['kind'] != 'sage')
    out32, got = H.conv_reference(case, ordered, torch.float32)
    frac, name = H.grad_rule_fraction(got, want)
    if frac > _worst.get(case['kind'], (0.0,))[0]:
        _worst[case['kind']] = (frac, name, case['id'], shape)
    print('float32 in sliced order uses %.3f of the rule (%s); worst so far per kind: %s' % (frac, name, _worst))
    assert np.isfinite(out32).all()
    H.assert_fp32_close(out32, out_plain, out64, what='%s %s out' % (case['id'], shape))
    assert frac <= HEADROOM, '%s: the float32 restatement already uses %.2f of the rule' % (name, frac)


# ---------------------------------------------------------------------------------------------------------------------
# the integer recipe
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', SAGE_CASES, ids=[c['id'] for c in SAGE_CASES])
def test_integer_recipe_is_exact_in_float32(case, shape):
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    x, params, gout = H.sage_integer_tensors(case, g)
    assert float(x.abs().max()) == 8 and all(torch.equal(t, t.round()) for t in [x, gout] + list(params.values()))
    kept = H.kept_edges(g['edge_index'], False)
    deg = np.bincount(kept[1], minlength=g['n'])
    plain = H.sage_by_edges(x, params, gout, kept[0], kept[1], deg, torch.float32)
    truth = H.sage_by_edges(x, params, gout, kept[0], kept[1], deg, torch.float64)
    src, dst, deg2 = H.sliced_edge_list(g, shape)
    assert np.array_equal(deg, deg2)
    sliced = H.sage_by_edges(x, params, gout, src, dst, deg, torch.float32)
    # x.grad is exact: float32 equals float64 bitwise, in either edge order.  `out`: a row's neighbour sum is exact, its mean is
    # one rounding of it (exact on rows whose degree is a power of two: there float32 equals float64), and the dense product
    # that follows sees the same mean in either edge order -- so the two float32 orders agree bitwise on every row
    assert np.array_equal(plain[1]['x'], sliced[1]['x']) and np.array_equal(plain[1]['x'], truth[1]['x'])
    assert np.abs(truth[1]['x']).max() > 0
    assert np.array_equal(plain[0], sliced[0])
    exact = H.pow2_rows(deg)
    assert np.array_equal(plain[0][exact], truth[0][exact]) and exact.sum() > g['n'] // 4
    # every chunk record of every hub row of the REVERSE relation gathers at least one row that carries a gradient, so a
    # dropped or misattributed record shows in x.grad.  (`out` covers every edge of the relation itself, and the degree graph
    # prescribes the same degrees on both sides.)
    live = H.pow2_rows(deg) & (np.abs(gout.numpy()).sum(axis=1) > 0)
    rk = H.kept_edges(g['edge_index'], False, True)
    rowptr, col, _ = H.sliced_csr(rk, g['n'], sh['slices'])
    cut, records = H.sliced_plan_items(rk, g['n'], sh['chunk'], 32, sh['slices'])
    assert cut.any()
    short = [(int(row), f, ln) for row, recs in records.items() for _, f, ln in recs if not live[col[rowptr[row] + f:rowptr[row] + f + ln]].any()]
    total = sum(len(r) for r in records.values())
    # (records of 8 edges: about 0.7^8 = 6 % of them gather no such row -- three gathered rows in ten carry a gradient)
    assert (not short) if sh['chunk'] >= 64 else len(short) <= 0.1 * total, (len(short), total, short[:5])


def test_integer_restatement_is_the_conv_restatement():
    """helpers.sage_by_edges restates oracle/pyg_restatement.py's SAGEConv: in float64, on the conv cases' own tensors, the same
    output and gradients (to the rounding of two summation orders)"""
    g = H.degree_graph()
    kept = H.kept_edges(g['edge_index'], False)
    deg = np.bincount(kept[1], minlength=g['n'])
    for case in SAGE_CASES[:2]:
        x, params, gout = H.conv_case_tensors(case, g['n'])
        out, grads = H.sage_by_edges(x, params, gout, kept[0], kept[1], deg, torch.float64)
        out64, want = _truth(case, g)
        np.testing.assert_allclose(out, out64, rtol=1e-12, atol=1e-12)
        assert set(grads) == set(want)
        for k in want:
            np.testing.assert_allclose(grads[k], want[k], rtol=1e-10, atol=1e-12, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# wrong restatements
# ---------------------------------------------------------------------------------------------------------------------
def _sage_dx(params, gout, rows, gathered, deg_in, dtype):
    """x.grad of L = sum(SAGEConv(x) * gout) the way the backward forms it: the root term, and over the REVERSED relation (row j
    gathers every i with an edge j -> i, in the listed order) the sum of (gout_i lin_rel) / deg_i"""
    w_rel, w_root, go = params['lin_rel.weight'].to(dtype), params['lin_root.weight'].to(dtype), gout.to(dtype)
    scaled = (go @ w_rel) / torch.from_numpy(np.maximum(deg_in, 1)).to(dtype)[:, None]
    dx = (go @ w_root).index_add(0, torch.from_numpy(np.ascontiguousarray(rows)), scaled[torch.from_numpy(np.ascontiguousarray(gathered))])
    return dx.numpy().astype(np.float64)


@pytest.mark.parametrize('wrong', ['drop_last_chunk', 'neighbour_row'])
@pytest.mark.parametrize('shape', SHAPES)
def test_wrong_restatements_fail_every_check(shape, wrong):
    g = H.agg_sliced_graph(shape)
    case = SAGE_CASES[1]
    fwd_right, fwd_wrong = H.sliced_edge_list(g, shape), H.sliced_edge_list(g, shape, wrong)
    bwd_right, bwd_wrong = H.sliced_edge_list(g, shape, reverse=True), H.sliced_edge_list(g, shape, wrong, reverse=True)
    for right, bad in ((fwd_right, fwd_wrong), (bwd_right, bwd_wrong)):
        assert (bad[0].size < right[0].size) == (wrong == 'drop_last_chunk') and bad[0].size <= right[0].size
        assert not (np.array_equal(right[0], bad[0]) and np.array_equal(right[1], bad[1]))
    deg_in = fwd_right[2]
    # --- the integer comparison: `out` shows a wrong forward list, x.grad a wrong list of the reversed relation
    x, params, gout = H.sage_integer_tensors(case, g)
    right = H.sage_by_edges(x, params, gout, *fwd_right, torch.float32)
    assert not np.array_equal(right[0], H.sage_by_edges(x, params, gout, *fwd_wrong, torch.float32)[0])
    dx = _sage_dx(params, gout, bwd_right[1], bwd_right[0], deg_in, torch.float32)
    assert np.array_equal(dx, right[1]['x'])                          # the reversed walk IS autograd's x.grad, bit for bit
    assert not np.array_equal(dx, _sage_dx(params, gout, bwd_wrong[1], bwd_wrong[0], deg_in, torch.float32))
    # --- the gradient rule and the forward criterion, on the conv case's own tensors
    x, params, gout = H.conv_case_tensors(case, g['n'])
    out64, want = _truth(case, g)
    out_r, got_r = H.sage_by_edges(x, params, gout, *fwd_right, torch.float32)
    assert H.grad_rule_fraction(got_r, want)[0] <= HEADROOM
    H.assert_fp32_close(out_r, out64.astype(np.float32), out64, what='right')
    good = dict(got_r, x=_sage_dx(params, gout, bwd_right[1], bwd_right[0], deg_in, torch.float32))
    assert H.grad_rule_fraction(good, want)[0] <= HEADROOM
    out_w, got_w = H.sage_by_edges(x, params, gout, *fwd_wrong, torch.float32)
    f_fwd, name = H.grad_rule_fraction(got_w, want)
    f_bwd, _ = H.grad_rule_fraction(dict(got_r, x=_sage_dx(params, gout, bwd_wrong[1], bwd_wrong[0], deg_in, torch.float32)), want)
    print('%s %s: forward list %.1f (%s), reversed list %.1f times the rule' % (shape, wrong, f_fwd, name, f_bwd))
    # the rule is relative to a tensor's largest element: the few rows of `out` a wrong FORWARD list changes move the weight
    # gradients (sums over all rows) by less than it at some shapes (measured 0.9 to 40 times the rule); they fail the forward
    # criterion below.  A wrong list of the REVERSED relation changes rows of x.grad themselves: hundreds of times the rule
    assert f_bwd > 1.0
    with pytest.raises(AssertionError):
        H.assert_fp32_close(out_w, out64.astype(np.float32), out64, what='wrong')
