"""GPU parity: the HIP path (through the C ABI / the drop-in modules) against
  (a) the golden vectors written by the reference's own models/base.py (tests/golden), and
  (b) the C oracle (oracle/pea_oracle.c) on seeded random HINs with hub rows, multi-edges, self loops.
Tolerance fp32: rtol 1e-5 / atol 1e-6 elementwise (config 2).  On the hub-row cases the
oracle itself sums ~10^3-10^4 fp32 terms sequentially; where an element misses the elementwise bound the test
falls back to a float64 evaluation and requires the HIP error to be no larger than twice the fp32 oracle's own
error (recorded reason: two different, equally valid fp32 summation orders)."""
import numpy as np
import pytest
import torch

from helpers import (GoldenCase, agg_lanes, assert_fp32_close, build_model, f64_forward, golden_cases, model_from_golden,
                     random_hin, random_state_dict)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('name', golden_cases())
def test_model_matches_reference_golden(name):
    g = GoldenCase(name)
    model = model_from_golden(g)
    model.eval()
    with torch.no_grad():
        fused, stack = model.forward(return_stack=True)
    for p in range(g.P):
        np.testing.assert_allclose(_np(stack[:, p]), g.out['channel/%d' % p], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(_np(fused), g.out['repr'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(_np(model.cached_repr), g.out['repr'], rtol=RTOL, atol=ATOL)
    model.eval(1)                                   # ablation: channel 1 zeroed before fusion
    np.testing.assert_allclose(_np(model.cached_repr), g.out['repr_mask1'], rtol=RTOL, atol=ATOL)
    model.eval()
    bt = torch.from_numpy(g.batch).cuda()
    np.testing.assert_allclose(_np(model.predict(bt[:, 0], bt[:, 1])).reshape(-1), g.out['pos'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(_np(model.predict(bt[:, 0], bt[:, 2])).reshape(-1), g.out['neg'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(float(model.loss(bt)), g.out['loss_eval'], rtol=RTOL)
    model.train()
    with torch.no_grad():
        if g.batch9 is None:
            np.testing.assert_allclose(float(model.loss(bt)), g.out['loss_train'], rtol=RTOL)
        else:
            b9 = torch.from_numpy(g.batch9).cuda()
            np.testing.assert_allclose(float(model.loss(b9)), g.out['loss_train'], rtol=RTOL)
    if g.batch9 is not None:
        # the same entity-aware loss under autograd (training step of --entity_aware=true): same value, and x receives
        # the regulariser's gradient on top of the conv stack's
        model.zero_grad()
        b9 = torch.from_numpy(g.batch9).cuda()
        loss = model.loss(b9)
        np.testing.assert_allclose(float(loss), g.out['loss_train'], rtol=RTOL)
        loss.backward()
        assert model.x.grad is not None and bool(torch.isfinite(model.x.grad).all()) and float(model.x.grad.abs().max()) > 0


@pytest.mark.parametrize('name', ['pea_gat_p3deep_h2_att', 'pea_gcn_p5s2_att', 'pea_sage_p5s2_att'])
def test_single_conv_modules_match_oracle(name):
    """The per-layer drop-in modules (pea_{gat,gcn,sage}_conv) on their own, including the fused relu."""
    g = GoldenCase(name)
    model = model_from_golden(g)
    x = model.x.detach()
    hl = g.heads_lists()
    with torch.no_grad():
        for p in range(g.P):
            xin = g.state_dict['x']
            h = x
            for s in range(g.steps[p]):
                layer = model.pea_channels[p].gnn_layers[s]
                ei = model.meta_path_edge_index_list[p][s]
                want = orc.conv(g.kind, xin, g.edges[p][s], g.layer_params(p, s), hl[p][s])
                last = s == g.steps[p] - 1
                got = layer(h, ei, relu=not last)
                if not last:
                    want = orc.relu_(want)
                np.testing.assert_allclose(_np(got), want, rtol=RTOL, atol=ATOL)
                xin, h = want, got
            np.testing.assert_allclose(_np(model.pea_channels[p](x, model.meta_path_edge_index_list[p])),
                                       g.out['channel/%d' % p], rtol=RTOL, atol=ATOL)


def _oracle_model(kind, model, edges, steps, heads):
    sd = {k: _np(v) for k, v in model.state_dict().items()}
    cps, hls = [], []
    for p, S in enumerate(steps):
        cps.append([{k[len('pea_channels.%d.gnn_layers.%d.' % (p, s)):]: v for k, v in sd.items()
                     if k.startswith('pea_channels.%d.gnn_layers.%d.' % (p, s))} for s in range(S)])
        hls.append([1] * S if kind != 'gat' else ([heads] * (S - 1) + [1] if S > 1 else [heads]))
    return sd, cps, hls


@pytest.mark.parametrize('kind,heads,aggr', [('gat', 1, 'att'), ('gat', 2, 'att'), ('gcn', 1, 'att'),
                                              ('sage', 1, 'att'), ('gat', 1, 'mean')])
def test_hub_rows_multi_edges_vs_oracle(kind, heads, aggr):
    """4k users all rating one item -> a 4k-edge hub row (8 chunks) under user->item; rows of every bin."""
    n, blocks, rel = random_hin(11, n_user=4000, n_item=600, n_attr=40, e_u2i=60000, e_attr=3000)
    u2i, a2i = rel['u2i'], rel['a2i']
    flip = lambda e: np.ascontiguousarray(e[::-1])
    edges = [[u2i, flip(u2i)], [flip(u2i), u2i], [a2i, flip(u2i)], [flip(a2i), a2i, flip(u2i)]]
    steps = [2, 2, 2, 3]
    model = build_model(kind, n, edges, steps, 64, 32, 16, heads=heads, channel_aggr=aggr)
    model.load_state_dict(random_state_dict(model, 5))
    model.eval()
    with torch.no_grad():
        fused, stack = model.forward(return_stack=True)
    sd, cps, hls = _oracle_model(kind, model, edges, steps, heads)
    want, wstack = orc.pea_forward(kind, sd['x'], edges, cps, hls, att=sd.get('att'), channel_aggr=aggr,
                                   return_stack=True)
    t_fused, t_stack = f64_forward(kind, sd, edges, steps, heads, aggr)
    assert_fp32_close(_np(stack), wstack, t_stack, what='stack')
    assert_fp32_close(_np(fused), want, t_fused, what='fused')
    info = model._engine.plan.relation_info(model._engine.plan.relation_of[0][0])
    assert info['hub_rows'] >= 1 and info['hub_chunks'] >= 8 and info['short_rows'] > 0 and info['long_items'] > 8
    # scoring on top
    rng = np.random.default_rng(3)
    batch = np.stack([rng.integers(*blocks['u'], size=1000), rng.integers(*blocks['i'], size=1000),
                      rng.integers(*blocks['i'], size=1000)], axis=1).astype(np.int64)
    loss = float(model.loss(torch.from_numpy(batch).cuda()))
    wl, _, _ = orc.pea_loss(want, batch, sd['fc1.weight'], sd['fc1.bias'], sd['fc2.weight'], sd['fc2.bias'])
    np.testing.assert_allclose(loss, wl, rtol=2e-5)


def test_plan_csr_is_stable_destination_sort():
    from graph_recsys_benchmark_amd.engine import GraphPlan
    rng = np.random.default_rng(0)
    n, e = 500, 20000
    ei = np.stack([rng.integers(0, n, size=e), rng.integers(0, n, size=e)]).astype(np.int64)
    ei[:, :50] = ei[0, :50]                          # 50 self loops
    t = torch.from_numpy(ei).cuda()
    for drop in (True, False):
        plan = GraphPlan(n, [[t, torch.flip(t, dims=[0]), t.clone()]], self_loops=drop)
        assert plan.num_relations == 2 and plan.relation_of == [[0, 1, 0]]      # dedupe by content
        rowptr, col = plan.export_csr(0)
        keep = ei[0] != ei[1] if drop else np.ones(e, bool)
        src, dst = ei[0][keep], ei[1][keep]
        order = np.argsort(dst, kind='stable')
        np.testing.assert_array_equal(_np(col), src[order].astype(np.int32))
        np.testing.assert_array_equal(_np(rowptr), np.searchsorted(dst[order], np.arange(n + 1)).astype(np.int32))


def test_error_behaviour():
    from graph_recsys_benchmark_amd import _lib
    from graph_recsys_benchmark_amd.engine import GraphPlan
    bad = torch.tensor([[0, 7], [1, 2]], dtype=torch.int64).cuda()
    with pytest.raises(_lib.PeaError) as ei:
        GraphPlan(5, [[bad]], True)
    assert ei.value.code == -2
    g = GoldenCase('pea_gat_p5s2_h1_att')
    model = model_from_golden(g)
    model.eval()
    with pytest.raises(IndexError):
        model.predict(torch.tensor([0]).cuda(), torch.tensor([10 ** 6]).cuda())
    with pytest.raises(NotImplementedError):
        build_model('gat', g.meta['num_nodes'], g.edges, g.steps, 32, 24, 16, channel_aggr='concat').eval()


def test_source_sliced_hub_rows_match_oracle(monkeypatch):
    """Large relations get their hub rows cut per source slice (XCD-affine layout, csrc/plan.hip); shrink the
    thresholds so a small graph takes that path, and check results and plan shape."""
    monkeypatch.setenv('PEA_SLICE_MIN_EDGES', '1000')
    monkeypatch.setenv('PEA_SLICE_BYTES', '20000')
    n, blocks, rel = random_hin(31, n_user=5000, n_item=400, n_attr=30, e_u2i=90000, e_attr=2000)
    u2i, a2i = rel['u2i'], rel['a2i']
    flip = lambda e: np.ascontiguousarray(e[::-1])
    edges = [[u2i, flip(u2i)], [a2i, flip(u2i)], [flip(u2i), u2i]]
    steps = [2, 2, 2]
    for kind in ('gat', 'gcn', 'sage'):
        model = build_model(kind, n, edges, steps, 64, 64, 16)
        model.load_state_dict(random_state_dict(model, 6))
        model.eval()
        with torch.no_grad():
            fused, stack = model.forward(return_stack=True)
        plan = model._engine.plan
        info = plan.relation_info(plan.relation_of[0][0])          # user -> item: hub items, 5000 source users
        assert info['slices'] >= 8 and info['hub_chunks'] > info['hub_rows'] >= 1
        sd, cps, hls = _oracle_model(kind, model, edges, steps, 1)
        want, wstack = orc.pea_forward(kind, sd['x'], edges, cps, hls, att=sd.get('att'), return_stack=True)
        t_fused, t_stack = f64_forward(kind, sd, edges, steps, 1, 'att')
        assert_fp32_close(_np(stack), wstack, t_stack, what=kind + ' stack')
        assert_fp32_close(_np(fused), want, t_fused, what=kind + ' fused')


def test_entity_aware_kernel_value_and_gradient():
    """A11 as one HIP launch (csrc/entity.hip) on the batch of the reference-generated fixture pea_gat_p5s2_h1_att_ea:
    value against the C oracle and the reference's formula in float64 (models/base.py:50-73), gradient with respect to x
    against float64 autograd of that formula; a batch row with masks 0 contributes log(1/2) twice and no gradient."""
    from graph_recsys_benchmark_amd import engine, scoring
    g = GoldenCase('pea_gat_p5s2_h1_att_ea')
    assert g.batch9 is not None and g.batch9.shape[1] == 9
    x = torch.from_numpy(g.state_dict['x']).cuda().requires_grad_(True)
    t = torch.from_numpy(g.batch9).cuda()
    reg = engine.entity_reg(x, t)
    reg.backward()
    xd = torch.from_numpy(g.state_dict['x']).double().requires_grad_(True)
    td = torch.from_numpy(g.batch9)

    def sq(a, b):
        d = xd[td[:, a]] - xd[td[:, b]]
        return (d * d).sum(-1)

    want = -(((sq(1, 3) - sq(1, 4)) * td[:, 5]).sigmoid().log().sum()) - (((sq(0, 6) - sq(0, 7)) * td[:, 8]).sigmoid().log().sum())
    want.backward()
    np.testing.assert_allclose(float(reg), float(want), rtol=1e-5)
    np.testing.assert_allclose(float(reg), orc.entity_reg(g.state_dict['x'], g.batch9), rtol=1e-5)
    gw = xd.grad.numpy()
    np.testing.assert_allclose(_np(x.grad), gw, rtol=1e-4, atol=1e-6 * float(np.abs(gw).max()))
    b = g.batch9
    assert (b[:, 5] == 0).any() and (b[:, 8] == 0).any()
    # a batch row with both masks 0: six gradient rows of exact zeros out of the launch itself, and 2 log 2 in the value
    dead = (b[:, 5] == 0) & (b[:, 8] == 0)
    live = (b[:, 5] == 1) & (b[:, 8] == 1)
    assert dead.any() and live.any()
    with torch.no_grad():
        _, rows = scoring._entity_launch(x.detach(), t, want_grad=True)
        rows = _np(rows).reshape(b.shape[0], 6, -1)
        assert (rows[dead] == 0).all() and np.isfinite(rows).all()
        assert (np.abs(rows[live]).max(axis=(1, 2)) > 0).all()
        k_dead, k_live = int(np.flatnonzero(dead)[0]), int(np.flatnonzero(live)[0])
        alone = float(engine.entity_reg(x.detach(), t[[k_live]]))
        pair = float(engine.entity_reg(x.detach(), t[[k_dead, k_live]]))
        np.testing.assert_allclose(pair - alone, 2.0 * np.log(2.0), rtol=1e-5)
        np.testing.assert_allclose(float(engine.entity_reg(x.detach(), t[[k_dead]])), 2.0 * np.log(2.0), rtol=1e-6)
    with torch.no_grad():                                   # no-grad path: same value, no gradient rows
        np.testing.assert_allclose(float(engine.entity_reg(x.detach(), t)), float(reg), rtol=0, atol=0)
    bad = t.clone()
    bad[0, 3] = 10 ** 7
    with torch.no_grad():
        assert bool(torch.isnan(engine.entity_reg(x.detach(), bad)))
    with pytest.raises(IndexError):
        engine.check_pending_errors()


@pytest.mark.parametrize('emb', [4, 16, 20, 128, 256])
def test_entity_aware_kernel_at_every_lane_group(emb):
    """csrc/entity.hip has five lane-group instantiations; the fixtures run G = 8 (emb 32) and G = 16 (emb 64).  Here emb 4 and
    16 (G = 4, one and four active lanes), 20 (G = 8 with idle lanes), 128 (G = 32) and 256 (G = 64) on random rows, B = 67 so
    that the last workgroup is partial at every rows-per-workgroup (64 ... 4): value and gradient against the float64 formula
    (reference models/base.py:50-73) and float64 autograd, at the tolerances of the test above."""
    from graph_recsys_benchmark_amd import engine
    rng = np.random.default_rng(100 + emb)
    n, B = 50, 67
    xs = (rng.normal(size=(n, emb)) * 0.5 / np.sqrt(emb)).astype(np.float32)       # squared distances of about 0.5
    ids, masks = rng.integers(0, n, size=(B, 7)), rng.integers(0, 2, size=(B, 2))
    b9 = np.concatenate([ids[:, :5], masks[:, :1], ids[:, 5:], masks[:, 1:]], axis=1).astype(np.int64)
    assert all(set(np.unique(b9[:, c])) == {0, 1} for c in (5, 8)) and B % (256 // agg_lanes(emb)) != 0
    x = torch.from_numpy(xs).cuda().requires_grad_(True)
    reg = engine.entity_reg(x, torch.from_numpy(b9).cuda())
    reg.backward()
    engine.check_pending_errors()
    xd = torch.from_numpy(xs).double().requires_grad_(True)
    td = torch.from_numpy(b9)

    def sq(a, b):
        d = xd[td[:, a]] - xd[td[:, b]]
        return (d * d).sum(-1)

    want = -(((sq(1, 3) - sq(1, 4)) * td[:, 5]).sigmoid().log().sum()) - (((sq(0, 6) - sq(0, 7)) * td[:, 8]).sigmoid().log().sum())
    want.backward()
    np.testing.assert_allclose(float(reg), float(want), rtol=1e-5)
    gw = xd.grad.numpy()
    assert np.abs(gw).max() > 0
    np.testing.assert_allclose(_np(x.grad), gw, rtol=1e-4, atol=1e-6 * float(np.abs(gw).max()))
