"""CPU: what tests/test_gpu_bpr_head_matrix.py relies on, checked without a GPU (tests/bpr_head_ref.py holds the restatements).

1. HEAD_CELLS reaches every (R4, mode) instantiation of bpr_train_kernel, P = 1 / 3 / 4 / 9 at each, the three limit shapes and
   the route's cap of 5461 triples; every batch size meets both modes and an odd R4; every cell is one pea_bpr_train_supported
   accepts, and the hand-written predicate agrees with the library's on a grid around its boundary.
2. The comparison has room: for every cell the float32 restatement passes helpers.assert_fp32_close at its defaults against the
   float64 one (as `want` and as `truth`, so with no allowance for an oracle error) for the loss, every raw output and every
   gradient; the relu-gate exclusion (gate_margin) stays within its cap, keeps at least one triple, and no cell holds a
   pre-activation within HEAD_NEAR_ULPS of the gate.
3. The comparison notices: each planted defect of head_reference fails it against the correct float64 truth.
4. The constructed id vectors of the scatter hold the run lengths NB - 1, NB, NB + 1, 2 NB, 2 NB + 1 of both width classes,
   interleaved, three ids in one LDS bucket, the table's last row and the three kinds of skipped id; n % 4 takes 1, 2, 3.
5. The scatter's comparisons notice a position left out (bit-exact and float64) and two rows added in swapped order (bit-exact
   only: float32 addition is not associative on the chosen rows, which is asserted).

test_largest_used_headroom_over_the_matrix computes, prints (-s) and bounds the maxima over the 72 cells.  When it was written:
every raw output, the loss and d picked pass on the elementwise tier of assert_fp32_close (largest used share of atol + rtol
|float64|: zx 0.70), the parameter gradients on it or on the per-row tier (12 of 288 comparisons), none on the two-sided tier;
the parameter gradients use at most 0.007 of the gradient rule (the float32 sums of torch depend on the thread count);
gate_margin excludes one triple of 257 in R4_4-no_pad-att, 2 of 5461 in either route_cap cell, none elsewhere."""
import numpy as np
import pytest
import torch

import bpr_head_ref as H
import helpers
from graph_recsys_benchmark_amd import _lib

GRAD_KEYS = tuple('d_' + k for k in H.KEYS)
DEFECT_CELLS = [next(c for c in H.HEAD_IDS if c.startswith(name)) for name in ('R4_3-one_pad-att', 'R4_5-headline-att', 'limit_P64xR16_cols1024-att')]


def test_cells_reach_every_instantiation_and_limit():
    cells = H.HEAD_CELLS
    assert len(cells) == 8 * 4 * 2 + 3 * 2 + 2 and len(set(H.HEAD_IDS)) == len(cells)
    shapes = {(r // 4, mode, p) for _, b, p, r, mode, _ in cells}
    for r4 in range(1, 9):
        for mode in H.MODES:
            for p in (1, 3, 4, 9):
                assert (r4, mode, p) in shapes, (r4, mode, p)
    for p, r in ((64, 16), (32, 32), (64, 4)):
        assert {mode for _, b, pp, rr, mode, _ in cells if (pp, rr) == (p, r)} == set(H.MODES), (p, r)
    assert {b for _, b, *_ in cells} == {1, 63, 64, 65, 257, 5461}
    for b in (1, 63, 64, 65, 257):
        assert {mode for _, bb, p, r, mode, _ in cells if bb == b} == set(H.MODES), b
        assert any((r // 4) % 2 == 1 for _, bb, p, r, mode, _ in cells if bb == b), 'B = %d meets no odd R4' % b
    assert [(b, p, r, mode) for _, b, p, r, mode, _ in cells if b == 5461] == [(5461, 9, 16, 'att'), (5461, 9, 16, 'mean')]
    assert {(r // 4, mode) for _, b, p, r, mode, _ in H.FUSE_CELLS} == {(r4, m) for r4 in range(1, 9) for m in H.MODES}
    assert len(H.FUSE_CELLS) == 16 + 6
    lib = _lib.load()
    for cid, b, p, r, mode, _ in cells:
        assert H.head_supported(p, r) and lib.pea_bpr_train_supported(p, r) == 1, cid
        assert 3 * b <= H.SCATTER_MAX, cid


def test_supported_predicate_is_the_librarys():
    lib = _lib.load()
    for p in (-1, 0, 1, 2, 9, 31, 32, 33, 63, 64, 65, 256, 257):
        for r in (-4, 0, 1, 2, 4, 6, 8, 12, 16, 20, 24, 28, 30, 32, 36, 64):
            assert bool(lib.pea_bpr_train_supported(p, r)) == bool(H.head_supported(p, r)), (p, r)
    for p, r in ((64, 16), (32, 32), (1, 4)):
        assert H.head_supported(p, r)
    for p, r in ((65, 4), (33, 32), (9, 36), (9, 6), (0, 16)):
        assert not H.head_supported(p, r)


@pytest.mark.parametrize('cid', H.HEAD_IDS)
def test_float32_restatement_fits_the_rule(cid):
    inp, r32, r64, flagged = H.head_case(cid)
    b = flagged.size
    assert flagged.sum() <= H.exclusion_cap(b), '%s: %d of %d triples excluded' % (cid, flagged.sum(), b)
    assert (~flagged).any(), cid + ': no triple kept'
    near = H.gate_margin(*[inp[k] for k in H.KEYS], ulps=H.HEAD_NEAR_ULPS)
    assert not near.any(), '%s: triple %s within %g ulps of a relu gate' % (cid, np.flatnonzero(near), H.HEAD_NEAR_ULPS)
    report = {}
    H.assert_head_close(r32, r64, r64, flagged, what=cid, keys=H.RAW + ('loss',) + GRAD_KEYS, report=report)
    assert (r64['dsc'] is None) == (inp['att'] is None) == (r64['d_att'] is None)
    grads = {k: r64[k] for k in GRAD_KEYS if r64.get(k) is not None}
    frac, name = helpers.grad_rule_fraction({k: r32[k] for k in grads}, grads)
    assert frac <= 0.5, (cid, name, frac)
    print('%s: excluded %d of %d (%.2f %%); float32 against float64 in row ulps: %s; %.4f of the gradient rule (%s)'
          % (cid, flagged.sum(), b, 100.0 * flagged.sum() / b, ', '.join('%s %.1f %s' % ((k,) + v) for k, v in report.items()), frac, name))
    # the layout: the pad columns hold what bpr_train.hip documents, in both precisions
    p, r = inp['picked'].shape[1:]
    for ref in (r32, r64):
        assert not ref['dhx'][:, r + 1:].any() and not ref['zx'][:, 3 * r + 1:].any() and (ref['zx'][:, 3 * r] == 1).all()
        if ref['dsc'] is not None:
            assert ref['dsc'].shape == (3 * b, H.ceil4(p)) and not ref['dsc'][:, p:].any()
        assert np.array_equal(ref['dhx'][0::2, r], -ref['dhx'][1::2, r])
        assert ref['grad_rows'].shape == (3 * b, p * r)
    # the hand-written backward is autograd's
    np.testing.assert_allclose(r64['grad_rows'].reshape(r64['d_picked'].shape), r64['d_picked'], rtol=1e-11, atol=1e-14)


def test_largest_used_headroom_over_the_matrix():
    """The maxima over all cells, computed here rather than quoted: per output the largest share the float32 restatement uses of
    assert_fp32_close's elementwise allowance atol + rtol |float64| (above 1: the per-row tier decides), the deciding tiers, the
    largest share of the gradient rule and the largest excluded share.  No comparison may need the two-sided tier, no raw
    output or loss the per-row one, no cell more than half of the gradient rule."""
    keys = H.RAW + ('loss',) + GRAD_KEYS
    used, tiers, worst_frac, worst_share = dict.fromkeys(keys, 0.0), {}, (0.0, ''), (0.0, '')
    for cid in H.HEAD_IDS:
        inp, r32, r64, flagged = H.head_case(cid)
        for k in keys:
            if r64[k] is None:
                continue
            g, t = np.asarray(r32[k], np.float64), np.asarray(r64[k], np.float64)
            if k in H.PER_TRIPLE:
                keep = H.kept_rows(flagged, H.PER_TRIPLE[k])
                g, t = g[keep], t[keep]
            width = t.shape[-1] if t.ndim > 1 else t.size
            g, t = g.reshape(-1, width), t.reshape(-1, width)
            used[k] = max(used[k], float((np.abs(g - t) / (1e-6 + 1e-5 * np.abs(t))).max()))
            tier = helpers.fp32_tier(g, t, t)
            tiers[(k, tier)] = tiers.get((k, tier), 0) + 1
            assert tier != 'two-sided', (cid, k)
        grads = {k: r64[k] for k in GRAD_KEYS if r64[k] is not None}
        frac, name = helpers.grad_rule_fraction({k: r32[k] for k in grads}, grads)
        worst_frac = max(worst_frac, (frac, '%s %s' % (cid, name)))
        worst_share = max(worst_share, (float(flagged.mean()) if flagged.size >= 200 else 0.0, cid))
    print('largest used share of atol + rtol |float64| by the float32 restatement over %d cells: %s'
          % (len(H.HEAD_IDS), ', '.join('%s %.2f' % kv for kv in used.items())))
    print('deciding tiers: %s' % ', '.join('%s %s x%d' % (k + (n,)) for k, n in sorted(tiers.items())))
    print('largest share of the gradient rule: %.4f (%s); largest excluded share at B >= 200: %.2f %% (%s)'
          % (worst_frac + (100.0 * worst_share[0], worst_share[1])))
    assert worst_frac[0] <= 0.5 and worst_share[0] <= H.EXCLUDE_SHARE
    assert max(used[k] for k in H.RAW + ('loss', 'd_picked')) <= 1.0, used


def test_raw_outputs_are_the_operands_of_the_parameter_gradients():
    """dhx^T zx and sum_rows dsc[row, p] S[row, p] of the restatement are autograd's parameter gradients (float64): the layout
    head_reference writes down is the one engine.bpr_train_raw reduces"""
    inp, _, t, _ = H.head_case(DEFECT_CELLS[0])
    assert inp['picked'].shape[1:] == (3, 12)
    r = 12
    g = t['dhx'].T @ t['zx']
    np.testing.assert_allclose(g[:r, :2 * r], t['d_fc1_w'], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g[:r, 3 * r], t['d_fc1_b'], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g[r, 2 * r:3 * r], t['d_fc2_w'][0], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g[r, 3 * r], t['d_fc2_b'][0], rtol=1e-12, atol=1e-14)
    d_att = np.einsum('np,npr->pr', t['dsc'][:, :3], inp['picked'].double().numpy())
    np.testing.assert_allclose(d_att, t['d_att'][0], rtol=1e-12, atol=1e-14)


DEFECTS = {'ds_sign': ('dhx', 'grad_rows'), 'dsc_no_sum': ('dsc',), 'dsc_rotated': ('dsc',), 'zx_swapped': ('zx',), 'dhx_pad': ('dhx',)}


@pytest.mark.parametrize('cid', DEFECT_CELLS)
@pytest.mark.parametrize('wrong', sorted(DEFECTS))
def test_the_comparison_notices_a_wrong_head(wrong, cid):
    inp, r32, r64, flagged = H.head_case(cid)
    bad = H.head_reference(*[inp[k] for k in H.KEYS], torch.float32, wrong=wrong)
    for key in H.RAW:
        if key in DEFECTS[wrong]:
            with pytest.raises(AssertionError):
                H.assert_head_close(bad, r32, r64, flagged, what=wrong, keys=(key,))
            with pytest.raises(AssertionError):                    # with no float32 peer at all
                H.assert_head_close(bad, r64, r64, flagged, what=wrong, keys=(key,))
        elif wrong != 'ds_sign':                                   # ds_sign moves everything downstream of ds_1 as well
            assert np.array_equal(bad[key], r32[key]), (wrong, key)
    assert np.array_equal(bad['loss'], r32['loss']) and np.array_equal(bad['d_picked'], r32['d_picked'])


def test_gate_margin_flags_a_triple_on_the_gate():
    inp = H.head_inputs(65, 3, 12, 'att', 5)
    args = [inp[k] for k in H.KEYS]
    assert not H.gate_margin(*args).any()
    inp['fc1_w'][7] = 0.0
    inp['fc1_b'][7] = 0.0                                          # hidden unit 7 is exactly 0 for every triple
    assert H.gate_margin(*[inp[k] for k in H.KEYS]).all()
    assert H.exclusion_cap(1) == 1 and H.exclusion_cap(199) == 1 and H.exclusion_cap(200) == 1 and H.exclusion_cap(5461) == 27
    assert H.kept_rows(np.array([False, True, False]), 2).tolist() == [True, True, False, False, True, True]


# ------------------------------------------------------------------------------------------------ pea_rows_scatter_sum
def test_scatter_cases_hold_both_width_classes_and_the_boundary_widths():
    widths = [p * r for p, r, _ in H.SCATTER_CASES]
    assert {4, 256, 260, 1024} <= set(widths) and widths == [4, 256, 260, 768, 1024]
    assert [H.scatter_width_class(w) for w in widths] == [1, 1, 4, 4, 4]
    assert {m for _, _, m in H.SCATTER_CASES} == {1, 2, 3}
    for p, r, _ in H.SCATTER_CASES:
        assert p <= 64 and r % 4 == 0 and p * r <= 1024


@pytest.mark.parametrize('p,r,n_mod4', H.SCATTER_CASES, ids=H.SCATTER_IDS)
def test_scatter_ids_are_what_they_claim(p, r, n_mod4):
    ids, nodes, src, cols, dst0 = H.scatter_case(p, r, n_mod4)
    v = H.scatter_width_class(p * r)
    nb = 32 // v
    assert sorted(nodes) == sorted(H.SCATTER_RUNS[v]) and {nb - 1, nb, nb + 1, 2 * nb, 2 * nb + 1, 1} <= set(nodes)
    assert ids.dtype == np.int64 and ids.size % 4 == n_mod4 and ids.size <= H.SCATTER_MAX
    for length, node in nodes.items():
        pos = np.flatnonzero(ids == node)
        assert pos.size == length
        if length >= 7:
            assert (np.diff(pos) > 1).any(), 'the run of node %d is contiguous' % node
    inside = ids[(ids >= 0) & (ids < H.SCATTER_ROWS)]
    assert set(inside) == set(nodes.values())
    buckets = np.array(sorted(nodes.values())) % H.SCATTER_BUCKETS
    assert (np.bincount(buckets, minlength=H.SCATTER_BUCKETS) == 3).sum() == 1
    assert H.SCATTER_ROWS - 1 in nodes.values()
    assert {-1, H.SCATTER_ROWS, 2 ** 40} <= set(ids.tolist())
    assert sorted(cols) == [q * r for q in range(p)] and (p == 1 or cols != sorted(cols))
    assert not src.flags['C_CONTIGUOUS'] or p * r == src.base.shape[1]
    want, want64 = H.scatter_reference(ids, src, p, r, cols, dst0)
    assert want.dtype == np.float32 and want.shape == (H.SCATTER_ROWS, p * r + 4)
    written = np.zeros(H.SCATTER_ROWS, bool)
    written[list(nodes.values())] = True
    assert (want[~written] == 7.0).all() and (want[:, p * r:] == 7.0).all() and (want[written, :p * r] != 7.0).all()
    assert np.abs(want - want64).max() <= H.scatter_f64_bound(want64)
    # a one-position run is a copy, channel c of the source at column cols[c]
    row = src[np.flatnonzero(ids == nodes[1])[0]]
    for c in range(p):
        assert np.array_equal(want[nodes[1], cols[c]:cols[c] + r], row[c * r:(c + 1) * r])


@pytest.mark.parametrize('p,r,n_mod4', H.SCATTER_CASES, ids=H.SCATTER_IDS)
def test_the_scatter_comparisons_notice_a_dropped_and_a_swapped_row(p, r, n_mod4):
    ids, nodes, src, cols, dst0 = H.scatter_case(p, r, n_mod4)
    nb = 32 // H.scatter_width_class(p * r)
    node = nodes[nb + 1]                                             # the 33-long (V = 4: 9-long) run: its last row is a trip of its own
    want, want64 = H.scatter_reference(ids, src, p, r, cols, dst0)
    dropped, _ = H.scatter_reference(ids, src, p, r, cols, dst0, wrong=('drop_last', node))
    assert not np.array_equal(dropped, want) and np.flatnonzero((dropped != want).any(axis=1)).tolist() == [node]
    assert np.abs(dropped - want64).max() > H.scatter_f64_bound(want64)
    # two rows in swapped order: ... (s + a) + b ... against ... (s + b) + a ...  The first pair of the run for which the float32
    # sum of the whole run comes out with other bits: float32 addition is not associative, here shown on the test's own rows
    pos = np.flatnonzero(ids == node)

    def run_sum(order):
        acc = src[order[0]].copy()
        for q in order[1:]:
            acc = acc + src[q]
        return acc

    found = next((j for j in range(1, pos.size - 1)
                  if not np.array_equal(run_sum(np.concatenate([pos[:j], pos[[j + 1, j]], pos[j + 2:]])), run_sum(pos))), None)
    assert found is not None, 'float32 addition order does not matter on any pair of this run'
    swapped, swapped64 = H.scatter_reference(ids, src, p, r, cols, dst0, wrong=('swap', node, found))
    assert not np.array_equal(swapped, want) and np.flatnonzero((swapped != want).any(axis=1)).tolist() == [node]
    assert np.abs(swapped - want64).max() <= H.scatter_f64_bound(want64)        # invisible to the float64 bound
    assert np.array_equal(swapped64, want64)


@pytest.mark.parametrize('kind', ['one_node', 'distinct', 'skipped'])
def test_scatter_limit_cases(kind):
    ids, src, num_rows = H.scatter_limit_case(kind)
    assert ids.size == H.SCATTER_MAX == 16384
    dst0 = np.full((num_rows, 20), 7.0, np.float32)
    want, want64 = H.scatter_reference(ids, src, 1, 16, [0], dst0)
    assert np.abs(want - want64).max() <= H.scatter_f64_bound(want64)
    if kind == 'one_node':
        assert set(ids) == {2} and (want[:2] == 7.0).all() and not np.array_equal(want[2, :16], want64[2, :16].astype(np.float32))
    elif kind == 'distinct':
        assert (np.bincount(ids % H.SCATTER_BUCKETS) == 8).all() and np.array_equal(np.sort(ids), np.arange(16384))
        assert np.array_equal(want[ids, :16], src)
    else:
        assert np.array_equal(want, dst0) and not ((ids >= 0) & (ids < num_rows)).any()
