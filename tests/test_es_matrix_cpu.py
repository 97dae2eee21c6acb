"""CPU: what tests/test_gpu_es_matrix.py relies on, checked without a GPU.

1. The graph (helpers.es_graph = degree_graph(degrees=ES_DEGREES): 2082 nodes, 17,444 edges) holds every degree of ES_DEGREES as
   an in-degree and as an out-degree, with its self loops and duplicated edges; the copies of a duplicated edge carry different
   logits and different types; both type tables hold negative types, type 0 and +-(T-1).  The default degree_graph() is bit for bit what it
   was (a digest of its edge list).
2. The width lists reach every (mode, G, full / idle) cell; taking a width away names the cell it leaves empty.
3. The comparison has room: the float32 torch restatement of every GPU case stays within half of the per-edge rule
   |got - f64| <= 2e-5 |f64| + 1e-9 (backward: 2e-5 |g64| + 1e-6 y max|g| + 1e-9).
4. The masked-edge inputs never mask a whole row, and mask whole 64-edge chunks of the rows of 200 edges and more.
5. The comparison notices: types in CSR-slot order, the last edge of the 1100-edge row left out of its sum, and -r[0] on the
   type-0 edges of the edge list's second half each miss the rule.  (No deliberately wrong kernel is ever run on a GPU.)
6. helpers.es_plan_bins / es_sliced_bins, the hand restatement of the plan the GPU tests hold pea_plan_relation_info to, give the
   equalised chunk lengths (513 -> 257 + 256, 1100 -> 367 + 367 + 366; PEA_CHUNK=16: 69 records for 1100 edges).

Measured here, the float32 restatement against float64 as the largest used fraction of the rule: KGAT maps 0.049 to 0.100, KGCN
maps 0.043 to 0.136 with T = 37 (worst: emb 160) and 0.003 with T = 1 (one score per row); softmax forward 0.008 to 0.050 over
the four logit ranges and with masked edges; softmax backward 0.021 to 0.190 of its bound (worst: masked edges, index =
destination)."""
import hashlib

import numpy as np
import pytest
import torch

import helpers as H

HEADROOM = 0.5
KG_CASES = [(mode, emb, nt) for mode in H.ES_MODES for emb in H.ES_FULL_WIDTHS + H.ES_IDLE_WIDTHS for nt in (H.ES_T, 1)]
KG_IDS = [H.es_case_id(*c) for c in KG_CASES]
SOFTMAX_CASES = [(name, side) for side in ('dst', 'src') for name in tuple(H.ES_LOGITS) + ('masked',)]


def test_default_degree_graph_is_unchanged():
    g = H.degree_graph()
    assert g is H.degree_graph(degrees=H.AGG_DEGREES) and g is not H.es_graph()
    ei = g['edge_index']
    assert g['n'] == 2076 and ei.shape == (2, 15896) and ei.dtype == np.int64 and ei.flags['C_CONTIGUOUS']
    assert hashlib.sha256(ei.tobytes()).hexdigest() == '8998632f5cbce270f3d7215a927f271e4502e3697930e2d05800579a773bf48b'
    assert g['degrees'] == [d for d in H.AGG_DEGREES if d > 0]
    assert all(len(g['blocks'][k]) == 18 for k in ('dst_lone', 'dst', 'src_lone', 'src'))


def test_es_graph_holds_every_degree_on_both_sides():
    assert H.ES_DEGREES == H.AGG_DEGREES + (255, 256, 257)
    g = H.es_graph()
    ei, n = g['edge_index'], g['n']
    assert H.es_graph() is g and n == 2082 and ei.shape == (2, 17444) and ei.min() >= 0 and ei.max() < n
    deg_in, deg_out = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
    for side, deg in (('in', deg_in), ('out', deg_out)):
        for d in H.ES_DEGREES:
            assert (deg == d).any(), '%s-degree %d missing' % (side, d)
        assert deg.max() == 1100
    assert int((ei[0] == ei[1]).sum()) == 40                                   # the self loops take part
    pairs, counts = np.unique(ei, axis=1, return_counts=True)
    assert int((counts - 1).sum()) > 200
    for side, deg in ((1, deg_in), (0, deg_out)):                              # a duplicated edge in a short, a long and a hub row
        d = deg[pairs[side][counts > 1]]
        assert (d <= 32).any() and ((d > 32) & (d <= 512)).any() and (d > 512).any()
    # the copies of a duplicated edge differ in type and in every logit set
    t = H.es_types(H.ES_T)
    order = np.lexsort((ei[1], ei[0]))
    same = np.flatnonzero((ei[:, order][:, 1:] == ei[:, order][:, :-1]).all(axis=0))
    assert same.size > 200
    groups = {}
    for e in range(ei.shape[1]):
        groups.setdefault((int(ei[0, e]), int(ei[1, e])), []).append(e)
    dups = [ids for ids in groups.values() if len(ids) > 1]
    assert len(dups) > 200
    for ids in dups:
        assert len({int(t[e]) for e in ids}) == len(ids)
        for name in H.ES_LOGITS:
            assert len({float(H.es_logits(name)[e]) for e in ids}) == len(ids)


def test_type_tables():
    t = H.es_types(H.ES_T)
    assert t.dtype == np.int64 and t.shape == (17444,) and t.min() == -(H.ES_T - 1) and t.max() == H.ES_T - 1
    assert set(np.unique(t)) == set(range(-(H.ES_T - 1), H.ES_T))              # every type, negative ones, 0 and +-(T-1)
    assert (t == 0).sum() > 100 and (t < 0).sum() > 5000
    half = t.size // 2
    assert (t[half:] == 0).sum() > 50                                          # what the 'rev0' restatement gets wrong
    t1 = H.es_types(1)
    assert t1.shape == t.shape and not t1.any()
    # in CSR-slot order the table is another one for nearly every edge
    order = H.es_csr_order(H.es_graph()['edge_index'][1])
    assert (t[order] != t).mean() > 0.9


def test_the_width_lists_reach_every_cell():
    assert len(set(KG_IDS)) == len(KG_IDS) == 2 * 14 * 2
    assert set(H.ES_KNOB_WIDTHS) <= set(H.ES_FULL_WIDTHS + H.ES_IDLE_WIDTHS)
    assert sorted(H.agg_lanes(w) for w in H.ES_KNOB_WIDTHS) == [4, 8, 16, 32, 64]
    H.check_es_cells()
    assert H.es_case_id('kgat', 20, 37) == 'kgat-G8-idle-emb20-T37' and H.es_case_id('kgcn', 256, 1) == 'kgcn-G64-full-emb256-T1'
    shared = {4: (12,), 12: (4,), 20: (24,), 24: (20,), 36: (40,), 40: (36,), 132: (160,), 160: (132,)}      # same cell
    for w in H.ES_FULL_WIDTHS + H.ES_IDLE_WIDTHS:
        full = tuple(v for v in H.ES_FULL_WIDTHS if v != w and v not in shared.get(w, ()))
        idle = tuple(v for v in H.ES_IDLE_WIDTHS if v != w and v not in shared.get(w, ()))
        G, lanes = H.es_cell('kgat', w)[1:]
        with pytest.raises(AssertionError, match=r'\(kgat, G = %d\) with %s lanes' % (G, lanes)):
            H.check_es_cells(full, idle)
        if w in shared:                                                         # one of the pair is enough
            H.check_es_cells(tuple(v for v in H.ES_FULL_WIDTHS if v != w), tuple(v for v in H.ES_IDLE_WIDTHS if v != w))
    with pytest.raises(AssertionError, match='width 16 has no idle lane'):
        H.check_es_cells(H.ES_FULL_WIDTHS, H.ES_IDLE_WIDTHS + (16,))


@pytest.mark.parametrize('mode,emb,nt', KG_CASES, ids=KG_IDS)
def test_float32_restatement_of_the_kg_maps_fits_half_the_rule(mode, emb, nt):
    r64 = H.es_kg_reference(mode, emb, nt)
    r32 = H.es_kg_reference(mode, emb, nt, dtype=torch.float32)
    assert r64.dtype == np.float64 and r64.shape == (17444,) and H.es_kg_reference(mode, emb, nt) is r64
    frac = H.es_rule_fraction(r32, r64)
    print('%s: the float32 restatement uses %.3f of the rule' % (H.es_case_id(mode, emb, nt), frac))
    assert frac <= HEADROOM
    sums = np.zeros(2082)
    np.add.at(sums, H.es_graph()['edge_index'][1], r64)
    has = np.bincount(H.es_graph()['edge_index'][1], minlength=2082) > 0
    assert np.abs(sums[has] - 1).max() < 1e-12 and (r64 > 0).all()
    # the attention is not flat: a wrong score moves it
    deg = np.bincount(H.es_graph()['edge_index'][1], minlength=2082)
    of_row = r64[H.es_graph()['edge_index'][1] == int(np.flatnonzero(deg == 1100)[0])]
    assert of_row.max() > 1.5 * of_row.min() or (mode, nt) == ('kgcn', 1)       # x_i . r[0] is one score for the whole row


@pytest.mark.parametrize('name,side', SOFTMAX_CASES, ids=['%s-index_%s' % c for c in SOFTMAX_CASES])
def test_float32_restatement_of_the_softmax_fits_half_the_rule(name, side):
    y64, g64 = H.es_softmax_case(name, side)
    y32, g32 = H.es_softmax_case(name, side, torch.float32)
    f_fwd = H.es_rule_fraction(y32, y64)
    f_bwd = H.es_bwd_fraction(g32, g64, y64, float(np.abs(H.es_grad_out()).max()))
    print('softmax %s over %s: the float32 restatement uses %.3f of the rule, its backward %.3f' % (name, side, f_fwd, f_bwd))
    assert f_fwd <= HEADROOM and f_bwd <= HEADROOM
    if name == 'masked':
        m = H.es_mask(side)
        assert not y64[m].any() and not g64[m].any() and (y64[~m] > 0).all()
    else:
        assert (y64 > 0).all()
    sums = np.zeros(2082)
    np.add.at(sums, H.es_index(side), y64)
    assert np.abs(sums[np.bincount(H.es_index(side), minlength=2082) > 0] - 1).max() < 1e-12


@pytest.mark.parametrize('side', ['dst', 'src'])
def test_masked_inputs_never_mask_a_whole_row(side):
    index, m = H.es_index(side), H.es_mask(side)
    deg = np.bincount(index, minlength=2082)
    masked = np.bincount(index[m], minlength=2082)
    assert (masked[deg < 3] == 0).all() and (masked[deg >= 3] > 0).all() and (masked < np.maximum(deg, 1)).all()
    big = deg >= 3
    assert ((masked[big] >= deg[big] // 3) & (masked[big] <= (deg[big] + 2) // 3)).all()       # a third of every row
    a = H.es_masked_logits(side)
    assert np.isneginf(a[m]).all() and np.isfinite(a[~m]).all()
    # the first edge of every row of 3 edges and more is masked (the row state starts from a -inf score), and the 1100-edge rows
    # lose their first 366 edges: at PEA_CHUNK=64 (18 chunks of 62 edges) that is five whole chunks
    order = H.es_csr_order(index)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    assert m[order[start[big]]].all()
    row = int(np.flatnonzero(deg == 1100)[0])
    assert m[order[start[row]:start[row] + 366]].all() and not m[order[start[row] + 366:start[row] + 1100]].any()


@pytest.mark.parametrize('wrong', ['slot', 'last', 'rev0'], ids=['types_in_slot_order', 'last_edge_of_1100_dropped', 'minus_r0_on_reversed_type0'])
@pytest.mark.parametrize('mode', H.ES_MODES)
def test_the_rule_notices_a_wrong_map(mode, wrong):
    for emb in (12, 40):
        r64 = H.es_kg_reference(mode, emb, H.ES_T)
        bad = H.es_kg_reference(mode, emb, H.ES_T, wrong=wrong)
        assert H.es_rule_fraction(H.es_kg_reference(mode, emb, H.ES_T, dtype=torch.float32), r64) <= HEADROOM      # the same code without the fault
        frac = H.es_rule_fraction(bad, r64)
        off = np.abs(bad - r64) > H.ES_RTOL * np.abs(r64) + H.ES_ATOL
        print('%s emb %d %s: %.1f times the rule, %d edges off' % (mode, emb, wrong, frac, int(off.sum())))
        assert frac > 10.0
        if wrong == 'last':                                                     # edges of that row only (its smallest weights move by less than the 1e-9)
            deg = np.bincount(H.es_graph()['edge_index'][1], minlength=2082)
            row = int(np.flatnonzero(deg == 1100)[0])
            assert 1000 <= off.sum() <= 1100 and not off[H.es_graph()['edge_index'][1] != row].any()
        else:
            assert off.sum() > 1000
        # the float32 restatement of the wrong map misses it as well: the miss is no rounding matter
        assert H.es_rule_fraction(H.es_kg_reference(mode, emb, H.ES_T, dtype=torch.float32, wrong=wrong), r64) > 10.0


def test_plan_restatement_gives_the_chunk_lengths():
    ei, n = H.es_graph()['edge_index'], H.es_graph()['n']
    for index in (ei[1], ei[0]):
        deg = np.bincount(index, minlength=n)
        b = H.es_plan_bins(deg)
        assert b['chunks'] == {513: [257, 256], 1100: [367, 367, 366]} and b['hub_rows'] == 4 and b['hub_slots'] == 10
        assert b['edges'] == 17444 and b['max_degree'] == 1100
        b64 = H.es_plan_bins(deg, chunk=64)
        assert [len(b64['chunks'][d]) for d in (65, 127, 128, 129, 200, 255, 256, 257, 511, 512, 513, 1100)] == [2, 2, 2, 3, 4, 4, 4, 5, 8, 8, 9, 18]
        assert b64['chunks'][1100] == [62] * 17 + [46] and b64['chunks'][257] == [52, 52, 52, 52, 49]
        b16 = H.es_plan_bins(deg, chunk=16)
        assert len(b16['chunks'][1100]) == 69 and b16['chunks'][33] == [11, 11, 11] and b16['long_items'] == b16['hub_slots']
        assert b16['short_rows'] == b['short_rows']                             # rows of 17 .. 32 edges stay short rows
        b1024 = H.es_plan_bins(deg, chunk=1024)
        assert b1024['chunks'] == {1100: [550, 550]} and b1024['hub_rows'] == 2
        s64 = H.es_plan_bins(deg, short_deg=64)
        assert s64['short_rows'] - b['short_rows'] == int(((deg > 32) & (deg <= 64)).sum()) > 0 and s64['hub_slots'] == 10
    # a knob the library ignored would leave the default plan, and no knob case expects the default plan's numbers
    fields = ('short_rows', 'long_items', 'hub_rows', 'hub_slots')
    deg = np.bincount(ei[1], minlength=n)
    default = [H.es_plan_bins(deg)[k] for k in fields]
    others = [H.es_plan_bins(deg, chunk=c) for c in (64, 16, 1024, 2048, 256)] + [H.es_plan_bins(deg, short_deg=64)]
    others += [H.es_sliced_bins(ei, n, chunk=c) for c in (512, 256)]
    assert all([o[k] for k in fields] != default for o in others)
    assert H.es_sliced_bins(ei, n, chunk=256)['hub_slots'] != H.es_plan_bins(deg, chunk=256)['hub_slots']      # the slices, not the chunk size
    assert H.es_sliced_bins(ei, n)['pad_items'] == 0 and H.es_sliced_bins(ei, n, chunk=256)['pad_items'] == 24
    for chunk, cut in ((512, [513, 513, 1100, 1100]), (256, [257, 511, 511, 512, 512, 513, 513, 1100, 1100])):
        s = H.es_sliced_bins(ei, n, chunk=chunk)
        assert s['sliced_degrees'] == cut and s['hub_rows'] == len(cut) and s['pad_items'] >= 0
        assert s['hub_slots'] >= 8 * len([d for d in cut if d >= 511])           # every slice holds a segment of the big rows
        assert s['short_rows'] == H.es_plan_bins(np.bincount(ei[1], minlength=n))['short_rows']
