"""GPU: the aggregation backward (csrc/agg_bwd.hip, wired by csrc/model_bwd.hip) at every lane width, head class, row form and
live-row density, each cell against torch autograd on the float64 restatement (oracle/pyg_restatement.py).

The graph (helpers.degree_graph, 2076 nodes) prescribes in- AND out-degrees, so a relation and its reverse both hold rows of
0, 1, 3, 4, 5 (short rows take 4 edges per step), 31, 32, 33 (32 = the longest short row), 63, 64, 65, 127, 128, 129, 200 (long
rows take 64 edges per batch), 511, 512, 513 (512 = the longest unchunked row) and 1100 edges, with duplicated edges, self loops
in the input, and sources of every row form that have no in-edge (the `lone` branch of the S pass).  PEA_CHUNK=64 cuts the same
rows into hub rows of 2, 3, 4, 8, 8, 9 and 18 chunks (the merge kernels read 8 records per step).

  test_plan_holds_every_row_form       the plan nn.conv caches: short rows, long items, hub rows and hub chunks of the relation and
                                       of its reverse, exactly as the degrees say, at both chunk sizes
  test_single_conv_matches_float64     nn.GATConv / GCNConv / SAGEConv under a dense random output gradient: out, dx and every
                                       parameter gradient; every (G, head class) pair launch_bwd_mode can form, widths with idle
                                       lanes, in_channels 8 / 36, negative_slope 0 / 0.2 / 1; the ids name G and the class
  test_single_conv_with_chunks_of_64   one width per G and kind again, hub rows of up to 18 chunks
  test_row_flags_match_float64_and_the_unflagged_step
                                       model.loss(batch) of 2-step level-wise models (PEA_FUSED2_TRAIN=0): the last layer runs
                                       the SP kernels (row flags, per-wave survivor queue) over the batch's rows.  That layer is
                                       repr_dim wide: 16 and 12 (G = 4) at all six densities; 32, 64, 128, 256 (G = 8 ... 64, GAT
                                       class `full`, and past 32 the PEAStackFunction route) at two_percent and every_node.  SP with
                                       several heads or a `four` / `generic` class beyond G = 4 stays uncovered: a last layer has
                                       one head.  Level-wise SAGE sets no row flags (its launches are asserted to be the plain ones)
  test_colsum_beyond_one_column_block_and_per_head
                                       a level 1152 columns wide (colsum_stage1's column-block loop) and 3 heads x 4 columns

Which (degree of the walked row, density of live gathered rows) drives which branch of bwd_long_item's survivor queue (a wave
walks a row of the REVERSED relation in batches of 64 edges and queues the live ones; the queue holds 64):

    collect and continue                         two_percent, every_second: any degree > 64
    mid-row flush (queue + batch > 64)           every_node, degree >= 129 (the second batch, 64 queued + 64 live, is not the last)
    last batch without a flush                   every_node, degree 64 (one batch); any sparse batch
    last batch WITH a flush and the second pass  every_node, degrees 65 to 128 (64 queued + 1..64 more: the old queue is
                                                 processed, then what the last batch left behind)
    nothing live (queue stays empty)             one_triple, hubs_only on most rows; all_but_hubs removes the hubs' own flags
                                                 (D pass: row_on false on a hub row; S pass: the hub rows' gradients are not fetched)

Tolerances: the project's gradient rule (test_gpu_backward.py), err <= 2e-4 max|want| + 1e-6 (largest gradient of the case) +
1e-9, rtol 2e-5 on the loss, helpers.assert_fp32_close on forward outputs.  tests/test_agg_bwd_matrix_cpu.py runs the float32
form of the same restatement on every case here and asserts it uses at most half of the rule; worst measured fractions:
single conv GAT 0.15 to 0.21 from run to run (att_i; the float32 sums depend on the thread count), GCN 0.004, SAGE 0.006; row-flag models GAT 0.21 (last layer's bias), GCN 0.03, SAGE 0.014; colsum
cases 0.08.  (Batches whose positives and negatives are drawn alike do NOT fit: the scorer's gradients cancel to nothing and
float32 itself used 0.9 to 45 times the rule; helpers.density_batch therefore takes its negatives from a few fixed nodes.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_backward import _assert_sparse_equals_dense

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _edge_tensor(chunk):
    """One device copy of the graph per chunk size: nn.conv caches its plans by edge tensor, so the cases of a chunk size share
    two plans (self loops dropped and kept); PEA_CHUNK is read when a plan is made, so the caller sets it before the first use."""
    return _cached(('ei', chunk), lambda: torch.from_numpy(H.degree_graph()['edge_index']).cuda())


def _kernel_names(step):
    """profile names (csrc/prof.hip) of the launches `step` makes"""
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    lib.pea_profile_enable(1)
    try:
        out = step()
        torch.cuda.synchronize()
    finally:
        lib.pea_profile_enable(0)
    cap = 4096
    names, cnt = C.create_string_buffer(cap * 32), C.c_int()
    lib.pea_profile_read(cap, names, None, None, C.byref(cnt))
    return out, {names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode() for i in range(cnt.value)}


def _bins(deg, chunk):
    """what csrc/plan.hip makes of these degrees: short rows (the edge-less ones included) hold at most 32 edges, a row of more
    than `chunk` edges is cut into ceil(deg / chunk) chunks, and every chunk is a long item like every row in between"""
    hub = deg > chunk
    chunks = int((-(-deg[hub] // chunk)).sum())
    return dict(max_degree=int(deg.max()), short_rows=int((deg <= 32).sum()), hub_rows=int(hub.sum()), hub_chunks=chunks,
                long_items=int(((deg > 32) & (deg <= chunk)).sum()) + chunks)


@pytest.mark.parametrize('self_loops', [True, False], ids=['loops_dropped', 'loops_kept'])
@pytest.mark.parametrize('chunk', [512, 64], ids=['chunk512', 'chunk64'])
def test_plan_holds_every_row_form(chunk, self_loops, monkeypatch):
    from graph_recsys_benchmark_amd.nn import conv
    g = H.degree_graph()
    if chunk != 512:
        monkeypatch.setenv('PEA_CHUNK', str(chunk))
    plan = conv._train_plan_for(_edge_tensor(chunk), g['n'], self_loops)
    deg_in, deg_out = H.kept_degrees(g['edge_index'], g['n'], self_loops)
    r = plan.relation_of[0][0]
    assert plan.reverse_of[r] != r and plan.reverse_of[plan.reverse_of[r]] == r
    for rel, deg in ((r, deg_in), (plan.reverse_of[r], deg_out)):
        info = plan.relation_info(rel)
        print(rel, info)
        assert min(info[k] for k in ('short_rows', 'long_items', 'hub_rows', 'hub_chunks')) > 0
        assert info['max_degree'] == 1100 and info['edges'] == int(deg.sum())
        assert {k: info[k] for k in _bins(deg, chunk)} == _bins(deg, chunk)
        per_row = -(-deg[deg > chunk] // chunk)
        if chunk == 512:
            assert sorted(per_row) == [2, 2, 3, 3] and info['hub_chunks'] == 10
        else:           # 65, 127, 128 -> 2; 129 -> 3; 200 -> 4; 511, 512 -> 8; 513 -> 9; 1100 -> 18: each on two rows
            assert sorted(per_row) == sorted(2 * [2, 2, 2, 3, 4, 8, 8, 9, 18]) and info['hub_chunks'] == 2 * 56


def _conv_module(case):
    from graph_recsys_benchmark_amd import nn
    if case['kind'] == 'gat':
        return nn.GATConv(case['in_ch'], case['out'], heads=case['heads'], negative_slope=case['slope'])
    if case['kind'] == 'gcn':
        return nn.GCNConv(case['in_ch'], case['out'], gcn_deg_from=case['deg'])
    return nn.SAGEConv(case['in_ch'], case['out'])


def _conv_reference(case, g=None, tag=None):
    g = g or H.degree_graph()
    key = ('conv', case['id']) if tag is None else ('conv', case['id'], tag)
    return _cached(key, lambda: (H.conv_reference(case, g, torch.float32)[0],) + H.conv_reference(case, g, torch.float64))


def _check_single_conv(case, chunk, graph=None, ei=None):
    """graph, ei: another graph (a dict of helpers.degree_graph) and a device copy of its edges whose plans the caller has shaped
    (tests/test_gpu_agg_sliced_matrix.py); default: the degree graph and the edge tensor of `chunk`"""
    g = graph or H.degree_graph()
    x, params, gout = H.conv_case_tensors(case, g['n'])
    conv = _conv_module(case)
    conv.load_state_dict(params, strict=True)
    conv = conv.cuda().train()
    xg = x.cuda().requires_grad_(True)
    ei = _edge_tensor(chunk) if ei is None else ei

    out = conv(xg, ei)
    _, names = _kernel_names(lambda: (out * gout.cuda()).sum().backward())       # the launches of the backward alone
    # the lane width the id names, and the hub rows' merges, really ran in the backward
    if case['kind'] == 'gat':
        G = H.agg_lanes(case['heads'] * case['out'])
        assert {'gat_bwd_dst_g%d' % G, 'gat_bwd_src_g%d' % G, 'gat_bwd_dst_merge', 'gat_bwd_src_merge', 'colsum'} <= names, sorted(names)
    else:       # a linear aggregation's backward is the weighted sum over the reversed relation: GCN at the output width,
        G = H.agg_lanes(case['out'] if case['kind'] == 'gcn' else case['in_ch'])           # SAGE at the input width
        assert {'agg_rows_g%d_gcn' % G, 'agg_merge_g%d_gcn' % G, 'colsum'} <= names, sorted(names)
    out32, out64, want = _conv_reference(case, g, None if graph is None else g['n'])      # the graphs in use differ in size
    got = {'x': xg.grad.cpu().numpy()}
    for name, p in conv.named_parameters():
        assert p.grad is not None, name
        got[name] = p.grad.cpu().numpy()
    assert set(got) == set(want) == {'x'} | set(H.CONV_PARAM_NAMES[case['kind']])
    frac, worst = H.grad_rule_fraction(got, want)
    print('%s chunk %d: gradients use %.3f of the rule (%s)' % (case['id'], chunk, frac, worst))
    assert bool(torch.isfinite(out).all()), case['id']         # (a NaN compares false with every bound; the rule has its own check)
    H.assert_fp32_close(out.detach().cpu().numpy(), out32, out64, what=case['id'] + ' out')
    assert frac <= 1.0, '%s: gradient of %s is off by %.2f times the rule' % (case['id'], worst, frac)


@pytest.mark.parametrize('case', H.AGG_CONV_CASES, ids=[c['id'] for c in H.AGG_CONV_CASES])
def test_single_conv_matches_float64(case):
    _check_single_conv(case, 512)


_CHUNK64_CASES = H.AGG_CHUNK64_CASES


@pytest.mark.parametrize('case', _CHUNK64_CASES, ids=[c['id'] for c in _CHUNK64_CASES])
def test_single_conv_with_chunks_of_64(case, monkeypatch):
    monkeypatch.setenv('PEA_CHUNK', '64')
    _check_single_conv(case, 64)


def _grads(model):
    out = {}
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        out[name] = p.grad.detach().clone()
    return out


def _stack_step(model, bt, flagged):
    """One training step through PEAStackFunction with the scorer in torch ops; flagged: the batch's rows are named (read_ids: row
    flags, SP kernels), else the backward gets the same dense d_stack, zero outside those rows, and walks every row."""
    from graph_recsys_benchmark_amd.autograd import PEAStackFunction, StackOptions
    eng = model._get_engine(train=True)
    flat = [t for lp in model._layer_params() for t in lp]
    ids = bt[:, :3].reshape(-1)
    model.zero_grad()
    stack = PEAStackFunction.apply(eng, model.x, eng.slots, StackOptions(read_ids=ids) if flagged else None, *flat)
    rows = model._fuse_torch(stack[ids]).view(bt.shape[0], 3, -1)
    score = lambda i: model.fc2(torch.relu(model.fc1(torch.cat([rows[:, 0], rows[:, i]], dim=-1))))
    loss = -(score(1) - score(2)).sigmoid().log().sum()
    loss.backward()
    return float(loss.detach()), _grads(model)


@pytest.mark.parametrize('kind,heads,hidden,repr_dim,channels,density', H.AGG_MODEL_CASES, ids=H.AGG_MODEL_IDS)
def test_row_flags_match_float64_and_the_unflagged_step(kind, heads, hidden, repr_dim, channels, density, monkeypatch):
    from graph_recsys_benchmark_amd.autograd import _Layout
    monkeypatch.setenv('PEA_FUSED2_TRAIN', '0')
    g = H.degree_graph()
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
    info = model._plan.relation_info(model._plan.relation_of[0][1])
    assert min(info[k] for k in ('short_rows', 'long_items', 'hub_rows')) > 0
    from graph_recsys_benchmark_amd import engine as _engine
    one_node = _engine.bpr_train_supported(channels, repr_dim)      # PEALossFunction; else PEAStackFunction with read_ids
    assert one_node == (repr_dim <= 32)
    G = H.agg_lanes(repr_dim)           # the last layer: one group per channel (each ends on another relation), repr_dim wide
    if kind == 'gat':                   # the last layer ran the flagged (SP) instantiations, the first the dense ones
        assert {'gat_bwd_dst_g%d_batch' % G, 'gat_bwd_src_g%d_batch' % G, 'gat_bwd_dst_merge', 'gat_bwd_src_merge'} <= names, sorted(names)
        assert 'gat_bwd_src_g%d' % H.agg_lanes(heads * hidden) in names, sorted(names)
    elif kind == 'gcn':
        assert {'sum_bwd_src_g%d_batch' % G, 'sum_bwd_src_merge'} <= names, sorted(names)
    else:                               # level-wise SAGE aggregates the layer's INPUT gradient, unflagged: hidden wide at the last layer
        assert {'agg_rows_g%d_gcn' % H.agg_lanes(hidden), 'agg_rows_g%d_gcn' % H.agg_lanes(H.AGG_EMB)} <= names, sorted(names)
        assert not any(nm.startswith(('gat_bwd', 'sum_bwd')) for nm in names), sorted(names)
    edges = H.agg_model_edges(g, channels)
    want_loss, want = _cached(('model', kind, heads, hidden, repr_dim, channels, density),
                              lambda: H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch))
    got = {k: v.cpu().numpy() for k, v in _grads(model).items()}
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('loss %.8g want %.8g; gradients use %.3f of the rule (%s)' % (float(loss.detach()), want_loss, frac, worst))
    np.testing.assert_allclose(float(loss.detach()), want_loss, rtol=2e-5)
    assert frac <= 1.0, 'gradient of %s is off by %.2f times the rule' % (worst, frac)
    if density in ('two_percent', 'every_second', 'every_node'):
        # the same step with the mask absent: skipped rows contribute exact zeros, only the summation order may differ
        l1, g1 = _stack_step(model, bt, True)
        l0, g0 = _stack_step(model, bt, False)
        np.testing.assert_allclose(l1, want_loss, rtol=2e-5)
        _assert_sparse_equals_dense(l1, g1, l0, g0)


@pytest.mark.parametrize('case', H.AGG_COLSUM_CASES, ids=H.AGG_COLSUM_IDS)
def test_colsum_beyond_one_column_block_and_per_head(case, monkeypatch):
    from graph_recsys_benchmark_amd.autograd import _Layout, layout_of
    monkeypatch.setenv('PEA_FUSED2_TRAIN', '0')
    kind, heads, hidden, repr_dim, channels = case
    model, sd, n, edges, batch = H.colsum_case(*case, device='cuda')
    bt = torch.from_numpy(batch).cuda()
    model.train()
    model.zero_grad()

    def step():
        loss = model.loss(bt)
        loss.backward()
        return loss

    loss, names = _kernel_names(step)
    assert 'colsum' in names
    lay = layout_of(model._train_engine)
    assert not _Layout(model._train_engine).two_step_train
    level0 = lay.levels[0]['units']
    assert sum(u['HF'] for u in level0) == channels * heads * hidden and {u['F'] for u in level0} == {hidden}
    if channels == 9:
        assert channels * heads * hidden == 1152 > 1024           # one reduction over the level: more than one column block
    want_loss, want = H.restated_loss_and_grads(kind, sd, edges, [2] * channels, heads, 'att', batch)
    got = {k: v.cpu().numpy() for k, v in _grads(model).items()}
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('loss %.8g want %.8g; gradients use %.3f of the rule (%s)' % (float(loss.detach()), want_loss, frac, worst))
    np.testing.assert_allclose(float(loss.detach()), want_loss, rtol=2e-5)
    assert frac <= 1.0, 'gradient of %s is off by %.2f times the rule' % (worst, frac)
    small = [k for k in want if k.endswith(('att_i', 'att_j', 'bias'))]
    assert len(small) == 2 * channels * 3 + 2        # per layer att_i, att_j, bias; fc1.bias and fc2.bias
    f2, w2 = H.grad_rule_fraction({k: got[k] for k in small}, {k: want[k] for k in small})
    assert f2 <= 1.0, 'gradient of %s is off by %.2f times the rule' % (w2, f2)
