"""GPU: the conv gathers, forward and backward, on SOURCE-SLICED plans (csrc/plan.hip: build_relation's XCD-affine layout).

A relation whose gather table overflows an XCD's L2 gets its edges regrouped by source slice inside every row, its rows of at
least S x 32 edges cut into per-slice chunks, those chunks laid out four per workgroup and slice ahead of every other long item,
and each round padded with `slot == -2` items.  The benchmark's user -> item relation is planned that way; the other matrices
(test_gpu_agg_bwd_matrix.py, test_gpu_wsum_matrix.py, test_gpu_two_step_matrix.py) build plans of one slice.  Here the knobs
PEA_SLICE_MIN_EDGES / PEA_SLICE_BYTES (and PEA_CHUNK) shape the plans of the 2076-node degree graph, the sizes derived from
helpers.slice_count -- the slice decision written down by hand -- and held against what the plan reports:

  shape        slices  what the plan holds (relation and reverse alike; helpers.AGG_SLICED_SHAPES)
  s8           8       rows of 513 and 1100 edges cut per slice: 32 records, one round of 8 x 4 filled exactly, no padding item
  s16          16      two phases; 512-edge rows stay direct items, 513 and 1100 are cut: 64 records, no padding item
  s32          32      four phases; only 1100 reaches 32 x 32 edges: 62 records and 66 padding items; the 513-edge rows are
                       plain two-chunk hub rows INSIDE a sliced plan
  s8_chunk64   8       PEA_CHUNK=64: 511, 512, 513, 1100 cut per slice into chunks of at most 64 (23 records on the 1100-edge
                       row: a second trip of every backward merge, and of the forward merge at G = 32 and 64), rows of 65 to 200
                       edges plain hub rows, 39 / 44 padding items
  s8_chunk8    8       PEA_CHUNK=8: 141 records on the 1100-edge row, more than the 8 x 64 / G = 128 a 4-lane forward merge folds
                       per trip: the second trip at every lane width
  s64_big      64      the degree graph with rows of 2047, 2048, 2049 and 4200 edges more (6484 nodes): eight phases, the most;
                       2048, 2049 and 4200 are cut (64 records on the 4200-edge row), 2047 is not

  test_plan_is_the_sliced_layout                     relation_info field for field, the slice count, and the exported CSR bit for
                                                     bit (numpy's stable sort by destination and slice), both self-loop settings
  test_single_conv_matches_float64_on_sliced_plans   helpers.AGG_SLICED_CASES (every kind x lane width, GAT `four` and `generic`
                                                     at G = 16 too) x every shape through test_gpu_agg_bwd_matrix._check_single_conv:
                                                     out, dx, every parameter gradient, the launches by name
  test_sliced_equals_unsliced_on_integers            SAGE on integers: out and x.grad torch.equal to the one-slice plan's, x.grad
                                                     equal to float64 -- the edge bookkeeping without a tolerance
  test_row_flag_models_on_sliced_plans               model.loss(batch) level-wise: the last layer's SP kernels (survivor queue)
                                                     walk sliced reverse rows, three densities
  test_two_step_schedule_on_a_sliced_first_layer     the two-step forward and training schedules over a sliced first layer
  test_hot_and_fat_kernels_on_a_sliced_plan          agg_long_hot_kernel's virtual-workgroup walk and agg_long_fat_kernel on the
                                                     4-per-workgroup layout, without (`s8`) and with (`s32`) padding items:
                                                     bitwise / 2e-6 against the plain kernel

No tolerance of its own: helpers.assert_fp32_close, the gradient rule (helpers.grad_rule_fraction), torch.equal, and the 2e-6
thin / fat rule of test_gpu_edge_cases.py.  tests/test_agg_sliced_cpu.py checks the table, the layouts and the float32 headroom
(at most half of the rule with the edges summed in sliced order) without a GPU, and holds two wrong restatements -- a dropped
chunk record, a slice segment added to the neighbouring hub row -- that fail these checks.

Not covered: sharded ranks with sliced plans; AGG_WSUM, which is never sliced (gather_row_bytes = 0)."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import oracle as orc
from test_gpu_agg_bwd_matrix import _cached, _check_single_conv, _conv_module, _grads, _kernel_names, _stack_step
from test_gpu_backward import _assert_sparse_equals_dense
from test_gpu_edge_cases import _kernel_names_of_one_forward

pytestmark = pytest.mark.gpu

SHAPES = list(H.AGG_SLICED_SHAPES)
INFO = ('edges', 'max_degree', 'short_rows', 'long_items', 'hub_rows', 'hub_chunks')       # engine.py: GraphPlan.relation_info
HOT_FAT_KNOBS = ('PEA_HOT', 'PEA_HOT_MIN_EDGES', 'PEA_HOT_MIN_FRACTION', 'PEA_FAT')


def _np(t):
    return t.detach().cpu().numpy()


def _set_knobs(monkeypatch, env):
    """the plan knobs of one test: exactly `env`, whatever the process had"""
    for knob in H.AGG_SLICED_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for knob, value in env.items():
        monkeypatch.setenv(knob, str(value))


def _shape(shape, monkeypatch):
    """(graph, device edge tensor) of a shape, its knobs set.  nn.conv caches its plans per edge tensor and the knobs are read when a
    plan is made: every shape owns a device copy of its graph's edges, and every test sets the knobs before its first use."""
    _set_knobs(monkeypatch, H.AGG_SLICED_SHAPES[shape]['env'])
    g = H.agg_sliced_graph(shape)
    return g, _cached(('sliced ei', shape), lambda: torch.from_numpy(g['edge_index']).cuda())


def _want_info(bins):
    return dict(zip(INFO, [bins[k] for k in ('edges', 'max_degree', 'short_rows', 'long_items', 'hub_rows', 'hub_slots')]))


@pytest.mark.parametrize('self_loops', [True, False], ids=['loops_dropped', 'loops_kept'])
@pytest.mark.parametrize('shape', SHAPES)
def test_plan_is_the_sliced_layout(shape, self_loops, monkeypatch):
    from graph_recsys_benchmark_amd.nn import conv
    sh = H.AGG_SLICED_SHAPES[shape]
    g, ei = _shape(shape, monkeypatch)
    plan = conv._train_plan_for(ei, g['n'], self_loops)
    r = plan.relation_of[0][0]
    assert plan.reverse_of[r] != r and plan.reverse_of[plan.reverse_of[r]] == r
    for rel, reverse in ((r, False), (plan.reverse_of[r], True)):
        kept = H.kept_edges(g['edge_index'], self_loops, reverse)
        bins = H.sliced_plan_bins(kept, g['n'], sh['chunk'], 32, sh['slices'])
        info = plan.relation_info(rel)
        print(shape, 'reverse' if reverse else 'relation', info, 'padding items', bins['pad_items'], 'records of the busiest row', bins['hub_records'])
        assert info['slices'] == sh['slices']
        assert {k: info[k] for k in INFO} == _want_info(bins)
        assert bins['sliced_degrees'] == sorted(d for d in sh['cut'] for _ in range(2 if d in H.AGG_DEGREES else 1))
        # the padding items are part of long_items: a shape whose rounds fill exactly has none, the others do
        assert (bins['pad_items'] == 0) == (shape in ('s8', 's16'))
        rowptr, col = plan.export_csr(rel)
        want_rowptr, want_col, _ = H.sliced_csr(kept, g['n'], sh['slices'])
        assert rowptr.dtype == torch.int32 and col.dtype == torch.int32
        np.testing.assert_array_equal(_np(rowptr), want_rowptr)
        np.testing.assert_array_equal(_np(col), want_col)
        assert not np.array_equal(want_col, H.sliced_csr(kept, g['n'], 1)[1])          # and that is not the plain destination sort


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', H.AGG_SLICED_CASES, ids=[c['id'] for c in H.AGG_SLICED_CASES])
def test_single_conv_matches_float64_on_sliced_plans(case, shape, monkeypatch):
    from graph_recsys_benchmark_amd.nn import conv
    sh = H.AGG_SLICED_SHAPES[shape]
    g, ei = _shape(shape, monkeypatch)
    _check_single_conv(case, sh['chunk'], graph=g if sh['big'] else None, ei=ei)
    plan = conv._train_plan_for(ei, g['n'], case['kind'] != 'sage')           # the plan that conv just used
    r = plan.relation_of[0][0]
    assert plan.relation_info(r)['slices'] == plan.relation_info(plan.reverse_of[r])['slices'] == sh['slices']


# ---------------------------------------------------------------------------------------------------------------------
# SAGE on integers
# ---------------------------------------------------------------------------------------------------------------------
_SAGE_CASES = [c for c in H.AGG_SLICED_CASES if c['kind'] == 'sage']


def _integer_step(case, g, ei):
    x, params, gout = H.sage_integer_tensors(case, g)
    conv = _conv_module(case)
    conv.load_state_dict(params, strict=True)
    conv = conv.cuda().train()
    xg = x.cuda().requires_grad_(True)
    out = conv(xg, ei)
    (out * gout.cuda()).sum().backward()
    return out.detach().clone(), xg.grad.detach().clone()


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', _SAGE_CASES, ids=[c['id'] for c in _SAGE_CASES])
def test_sliced_equals_unsliced_on_integers(case, shape, monkeypatch):
    """helpers.sage_integer_tensors: every neighbour sum of the forward is an integer below 2^24 divided once by the row's degree,
    every term of the backward's sums a dyadic fraction -- both exact in float32 in any order (tests/test_agg_sliced_cpu.py
    asserts float32 == float64 for the recipe).  So the sliced plan must give the one-slice plan's `out` and x.grad bit for bit:
    a dropped, duplicated or misattributed edge of any chunk shows, and no tolerance can hide it."""
    from graph_recsys_benchmark_amd.nn import conv
    sh, g = H.AGG_SLICED_SHAPES[shape], H.agg_sliced_graph(shape)
    n = g['n']
    _set_knobs(monkeypatch, {})                                    # the one-slice plan (chunks of 512) of the same graph

    def plain():
        ei1 = _cached(('plain ei', n), lambda: torch.from_numpy(g['edge_index']).cuda())
        res = _integer_step(case, g, ei1)
        assert conv._train_plan_for(ei1, n, False).relation_info(0)['slices'] == 1
        return res

    out1, dx1 = _cached(('integer', case['id'], n), plain)
    g, ei = _shape(shape, monkeypatch)
    out, dx = _integer_step(case, g, ei)
    plan = conv._train_plan_for(ei, n, False)
    assert [plan.relation_info(r)['slices'] for r in range(plan.num_relations)] == [sh['slices']] * 2
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    print('%s %s: out differs in %d elements, x.grad in %d' % (case['id'], shape, int((out != out1).sum()), int((dx != dx1).sum())))
    assert torch.equal(out, out1)
    assert torch.equal(dx, dx1)
    kept = H.kept_edges(g['edge_index'], False)
    x, params, gout = H.sage_integer_tensors(case, g)
    truth = _cached(('integer f64', case['id'], n),
                    lambda: H.sage_by_edges(x, params, gout, kept[0], kept[1], np.bincount(kept[1], minlength=n), torch.float64))
    assert np.array_equal(_np(dx).astype(np.float64), truth[1]['x'])
    exact = H.pow2_rows(np.bincount(kept[1], minlength=n))         # rows whose mean is exact: `out` equals float64 there
    assert np.array_equal(_np(out).astype(np.float64)[exact], truth[0][exact])


# ---------------------------------------------------------------------------------------------------------------------
# models: the level-wise schedule's flagged last layer, the two-step schedules, the hot and fat kernels
# ---------------------------------------------------------------------------------------------------------------------
def _model_knobs(g, row_bytes, slices, **more):
    """the shape's knobs for a model whose plan passes gather_row_bytes = 4 x hidden x heads"""
    return dict({'PEA_SLICE_MIN_EDGES': 1, 'PEA_SLICE_BYTES': H.slice_bytes_for(g['edge_index'], row_bytes, slices)}, **more)


def _assert_model_plan(model, g, slices, chunk):
    """every relation of the model's plan (the degree graph and its reverse) is the sliced layout the shape names"""
    plan = model._plan
    drop = model.kind in ('gat', 'gcn')
    assert plan.num_relations == 2
    for rel in range(plan.num_relations):
        reverse = not torch.equal(plan._uniq[rel].cpu(), torch.from_numpy(g['edge_index']))
        bins = H.sliced_plan_bins(H.kept_edges(g['edge_index'], drop, reverse), g['n'], chunk, 32, slices)
        info = plan.relation_info(rel)
        assert info['slices'] == slices and {k: info[k] for k in INFO} == _want_info(bins), (rel, info, bins)
        assert bins['sliced_degrees'] and info['hub_chunks'] > info['hub_rows']


_ROW_FLAG_MODELS = [('gat', 2, 24, 12, 2), ('gcn', 1, 96, 16, 2), ('sage', 1, 24, 12, 2)]         # of helpers.AGG_MODELS, one per kind
assert set(_ROW_FLAG_MODELS) <= set(H.AGG_MODELS)


@pytest.mark.parametrize('density', ['two_percent', 'every_node', 'hubs_only'])
@pytest.mark.parametrize('shape', ['s8', 's8_chunk64'])
@pytest.mark.parametrize('kind,heads,hidden,repr_dim,channels', _ROW_FLAG_MODELS, ids=['%s-h%d-hid%d-r%d-P%d' % m for m in _ROW_FLAG_MODELS])
def test_row_flag_models_on_sliced_plans(kind, heads, hidden, repr_dim, channels, shape, density, monkeypatch):
    from graph_recsys_benchmark_amd.autograd import _Layout
    sh, g = H.AGG_SLICED_SHAPES[shape], H.degree_graph()
    more = {'PEA_CHUNK': sh['chunk']} if sh['chunk'] != 512 else {}
    _set_knobs(monkeypatch, _model_knobs(g, 4 * hidden * (heads if kind == 'gat' else 1), sh['slices'], **more))
    monkeypatch.setenv('PEA_FUSED2_TRAIN', '0')
    model, sd = H.agg_model_state(kind, heads, hidden, repr_dim, channels, g, device='cuda')
    batch = H.density_batch(density, g)
    bt = torch.from_numpy(batch).cuda()
    model.train()
    model.zero_grad()

    def step():
        loss = model.loss(bt)
        loss.backward()
        return loss

    loss, names = _kernel_names(step)
    assert not _Layout(model._train_engine).two_step_train
    _assert_model_plan(model, g, sh['slices'], sh['chunk'])
    G = H.agg_lanes(repr_dim)
    if kind == 'gat':                   # the last layer ran the flagged (SP) instantiations over sliced reverse rows
        assert {'gat_bwd_dst_g%d_batch' % G, 'gat_bwd_src_g%d_batch' % G, 'gat_bwd_dst_merge', 'gat_bwd_src_merge'} <= names, sorted(names)
        assert 'gat_bwd_src_g%d' % H.agg_lanes(heads * hidden) in names, sorted(names)
    elif kind == 'gcn':
        assert {'sum_bwd_src_g%d_batch' % G, 'sum_bwd_src_merge'} <= names, sorted(names)
    else:                               # level-wise SAGE sets no row flags: the plain weighted sums, hidden and emb wide
        assert {'agg_rows_g%d_gcn' % H.agg_lanes(hidden), 'agg_rows_g%d_gcn' % H.agg_lanes(H.AGG_EMB)} <= names, sorted(names)
        assert not any(nm.startswith(('gat_bwd', 'sum_bwd')) for nm in names), sorted(names)
    edges = H.agg_model_edges(g, channels)
    want_loss, want = _cached(('model', kind, heads, hidden, repr_dim, channels, density),
                              lambda: H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch))
    got = {k: _np(v) for k, v in _grads(model).items()}
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('%s %s %s: loss %.8g want %.8g; gradients use %.3f of the rule (%s)' % (kind, shape, density, float(loss.detach()), want_loss, frac, worst))
    assert np.isfinite(float(loss.detach()))
    np.testing.assert_allclose(float(loss.detach()), want_loss, rtol=2e-5)
    assert frac <= 1.0, 'gradient of %s is off by %.2f times the rule' % (worst, frac)
    if density in ('two_percent', 'hubs_only'):
        # the same step with the mask absent: skipped rows contribute exact zeros, only the summation order may differ
        l1, g1 = _stack_step(model, bt, True)
        l0, g0 = _stack_step(model, bt, False)
        np.testing.assert_allclose(l1, want_loss, rtol=2e-5)
        _assert_sparse_equals_dense(l1, g1, l0, g0)


def _forward_against_oracle(model, kind, edges, steps, what):
    """fused table and channel stack of one forward against the C oracle and float64 (test_gpu_edge_cases._check's comparison)"""
    with torch.no_grad():
        fused, stack = model.forward(return_stack=True)
    assert bool(torch.isfinite(stack).all()) and bool(torch.isfinite(fused).all())
    sd, cps, hls = H.oracle_params(model, steps, kind)
    want, wstack = orc.pea_forward(kind, sd['x'], edges, cps, hls, att=sd.get('att'), return_stack=True)
    t_fused, t_stack = H.f64_forward(kind, sd, edges, steps, 1, 'att')
    H.assert_fp32_close(_np(stack), wstack, t_stack, what=what + ' stack')
    H.assert_fused_close(_np(fused), _np(stack), want, t_fused, sd.get('att'), truth_stack=t_stack, what=what + ' fused')
    return fused, stack


TWO_STEP_WIDTH = 64         # emb = hidden: gather_row_bytes = 256, the conv plans' own, so the shapes' knobs apply as they are


@pytest.mark.parametrize('shape', ['s8', 's16'])
@pytest.mark.parametrize('kind', ['gat', 'gcn', 'sage'])
def test_two_step_schedule_on_a_sliced_first_layer(kind, shape, monkeypatch):
    from graph_recsys_benchmark_amd.autograd import _Layout
    sh, g = H.AGG_SLICED_SHAPES[shape], H.degree_graph()
    assert 4 * TWO_STEP_WIDTH == H.CONV_ROW_BYTES
    _set_knobs(monkeypatch, sh['env'])
    monkeypatch.delenv('PEA_FUSED2', raising=False)
    monkeypatch.delenv('PEA_FUSED2_TRAIN', raising=False)
    channels, steps = 2, [2, 2]
    edges = H.agg_model_edges(g, channels)
    model, sd = H.agg_model_state(kind, 1, TWO_STEP_WIDTH, 16, channels, g, emb=TWO_STEP_WIDTH, device='cuda')
    # forward: the first-layer gather of the two-step schedule walks the sliced layout, mlp2 chains both transforms
    model.eval()
    assert 'mlp2_fused' in _kernel_names_of_one_forward(model)
    _assert_model_plan(model, g, sh['slices'], sh['chunk'])
    assert model._plan.relation_info(model._plan.relation_of[0][0])['slices'] == sh['slices']
    _forward_against_oracle(model, kind, edges, steps, '%s %s' % (kind, shape))
    # one training step on the two-step training schedule
    batch = H.density_batch('two_percent', g)
    bt = torch.from_numpy(batch).cuda()
    model.train()
    model.zero_grad()
    loss = model.loss(bt)
    loss.backward()
    assert _Layout(model._train_engine).two_step_train
    want_loss, want = _cached(('two-step', kind), lambda: H.restated_loss_and_grads(kind, sd, edges, steps, 1, 'att', batch))
    got = {k: _np(v) for k, v in _grads(model).items()}
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('%s %s: loss %.8g want %.8g; gradients use %.3f of the rule (%s)' % (kind, shape, float(loss.detach()), want_loss, frac, worst))
    np.testing.assert_allclose(float(loss.detach()), want_loss, rtol=2e-5)
    assert frac <= 1.0, 'gradient of %s is off by %.2f times the rule' % (worst, frac)


@pytest.mark.parametrize('shape', ['s8', 's32'])
@pytest.mark.parametrize('kind', ['gat', 'gcn', 'sage'])
def test_hot_and_fat_kernels_on_a_sliced_plan(kind, shape, monkeypatch):
    """agg_long_hot_kernel is persistent: its 16 waves per workgroup replay the plain kernel's 4-items-per-workgroup order through
    virtual workgroups -- besides agg_rows_kernel the only consumer of the sliced item layout, padding items included -- and must
    give the plain kernel's result BITWISE.  agg_long_fat_kernel walks the same items with 16 columns per lane: within the
    2e-6 x max|stack| of test_gpu_edge_cases.py.  Hidden 64: one head of 64 columns takes the fat lanes.  `s8` has no padding
    item (its round fills exactly); `s32` has 66, which both kernels must pass over."""
    sh, g = H.AGG_SLICED_SHAPES[shape], H.degree_graph()
    _set_knobs(monkeypatch, sh['env'])
    for knob in HOT_FAT_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv('PEA_HOT_MIN_EDGES', '1000')
    channels, steps = 2, [2, 2]
    edges = H.agg_model_edges(g, channels)
    model, _ = H.agg_model_state(kind, 1, TWO_STEP_WIDTH, 16, channels, g, emb=TWO_STEP_WIDTH, device='cuda')
    model.eval()

    def forward(hot, fat):
        monkeypatch.setenv('PEA_HOT', hot)
        monkeypatch.setenv('PEA_FAT', fat)
        names = _kernel_names_of_one_forward(model)
        assert any(nm.startswith('agg_longhot_') for nm in names) == (hot == '1'), sorted(names)
        assert any(nm.startswith('agg_long_fat_') for nm in names) == (fat == '1'), sorted(names)
        return _forward_against_oracle(model, kind, edges, steps, '%s %s hot %s fat %s' % (kind, shape, hot, fat))

    fused, stack = forward('0', '0')
    _assert_model_plan(model, g, sh['slices'], sh['chunk'])
    hot_fused, hot_stack = forward('1', '0')
    assert torch.equal(hot_stack, stack) and torch.equal(hot_fused, fused)
    fat_fused, fat_stack = forward('0', '1')
    scale = float(stack.abs().max())
    diff = float((fat_stack - stack).abs().max())
    print('%s %s: fat against thin %.3e, bound %.3e' % (kind, shape, diff, 2e-6 * scale))
    assert diff <= 2e-6 * scale
