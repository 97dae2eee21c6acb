"""Training-step head in HIP (csrc/bpr_train.hip: channel fusion + fc1/fc2 scorer + BPR loss, forward and backward in one
launch) against float64 torch autograd of the reference's formulas (models/base.py:193-203, :208-214, :46-48)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _reference(picked, att, fc1_w, fc1_b, fc2_w, fc2_b):
    x = picked
    if att is None:
        fused = x.mean(dim=1)
    else:
        a = torch.softmax(torch.sum(x * att, dim=-1), dim=-1).unsqueeze(-1)
        fused = torch.sum(x * a, dim=1)
    rows = fused.view(-1, 3, fused.shape[-1])

    def score(i):
        z = torch.cat([rows[:, 0], rows[:, i]], dim=-1)
        return torch.relu(z @ fc1_w.t() + fc1_b) @ fc2_w.t() + fc2_b

    return -(score(1) - score(2)).sigmoid().log().sum()


@pytest.mark.parametrize('b,p,r,mode', [(257, 9, 16, 'att'), (64, 5, 8, 'mean'), (130, 3, 12, 'att'), (33, 13, 32, 'att'),
                                        (1, 9, 16, 'att'), (100, 1, 4, 'att'),
                                        (130, 4, 20, 'att'), (64, 3, 24, 'mean'), (33, 2, 28, 'att')])      # bpr_train_kernel<5>, <6>, <7>
def test_bpr_train_matches_float64_autograd(b, p, r, mode):
    from graph_recsys_benchmark_amd import engine
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(1000 * b + 10 * p + r)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s)
    tensors = dict(picked=mk(3 * b, p, r, s=0.7), att=mk(1, p, r, s=0.5) if mode == 'att' else None, fc1_w=mk(r, 2 * r, s=0.4),
                   fc1_b=mk(r, s=0.1), fc2_w=mk(1, r, s=0.5), fc2_b=mk(1, s=0.1))
    ref_in = {k: (v.double().requires_grad_(True) if v is not None else None) for k, v in tensors.items()}
    ref = _reference(**ref_in)
    ref.backward()
    hip_in = {k: (v.to(dev).requires_grad_(True) if v is not None else None) for k, v in tensors.items()}
    assert engine.bpr_train_supported(p, r)
    loss = engine.bpr_train_loss(hip_in['picked'], hip_in['att'], hip_in['fc1_w'], hip_in['fc1_b'], hip_in['fc2_w'],
                                 hip_in['fc2_b'])
    (2.0 * loss).backward()      # a non-unit upstream gradient must scale every gradient
    assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref)) + 1e-6 * b
    for k, v in hip_in.items():
        if v is None:
            continue
        want = 2.0 * ref_in[k].grad
        got = v.grad.double().cpu()
        assert got.shape == want.shape, k
        err = float((got - want).abs().max())
        assert err <= 2e-5 * float(want.abs().max()) + 1e-7, (k, err, float(want.abs().max()))


@pytest.mark.parametrize('aggr', ['att', 'mean'])
def test_training_loss_of_a_model_uses_the_hip_head_and_matches_the_torch_head(aggr):
    """model.loss(batch) under autograd: the HIP head against the torch-op head it replaced (same stack rows); the
    float64 check of the whole step is tests/test_gpu_backward.py."""
    import numpy as np
    from graph_recsys_benchmark_amd import engine
    from helpers import build_model, random_hin, random_state_dict
    n, blocks, rel = random_hin(47, n_user=900, n_item=300, n_attr=20, e_u2i=9000, e_attr=800)
    u2i, a2i = rel['u2i'], rel['a2i']
    flip = lambda e: np.ascontiguousarray(e[::-1])
    edges = [[u2i, flip(u2i)], [flip(u2i), u2i], [a2i, flip(u2i)]]
    model = build_model('gat', n, edges, [2, 2, 2], 32, 32, 16, channel_aggr=aggr)
    model.load_state_dict(random_state_dict(model, 9, scale=0.25))
    rng = np.random.default_rng(3)
    batch = torch.from_numpy(np.stack([rng.integers(*blocks['u'], size=200), rng.integers(*blocks['i'], size=200),
                                       rng.integers(*blocks['i'], size=200)], axis=1).astype(np.int64)).cuda()
    model.train()
    calls = []
    orig_raw = engine.bpr_train_raw
    engine.bpr_train_raw = lambda *a: (calls.append(1), orig_raw(*a))[1]
    try:
        model.zero_grad()
        loss = model.loss(batch)
        loss.backward()
    finally:
        engine.bpr_train_raw = orig_raw
    assert calls, 'the training loss did not go through csrc/bpr_train.hip'
    got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    model.zero_grad()
    (0.5 * model.loss(batch)).backward()        # a non-unit upstream gradient scales every gradient (exactly: a power of two)
    for k, v in model.named_parameters():
        if v.grad is not None:
            assert torch.equal(v.grad, 0.5 * got[k]), k
    orig = engine.bpr_train_supported
    engine.bpr_train_supported = lambda *_: False     # the torch-op head (kept for repr_dim > 32)
    try:
        model.zero_grad()
        loss2 = model.loss(batch)
        loss2.backward()
    finally:
        engine.bpr_train_supported = orig
    assert abs(float(loss) - float(loss2)) <= 1e-5 * abs(float(loss2))
    for k, v in model.named_parameters():
        assert (v.grad is None) == (k not in got), k
        if v.grad is None:
            continue
        scale = float(v.grad.abs().max())
        assert float((got[k] - v.grad).abs().max()) <= 2e-4 * scale + 1e-7, k


def test_rows_scatter_sum_accumulates_duplicates_in_position_order():
    """pea_rows_scatter_sum against a sequential float32 accumulation in position order: bit-exact (the same additions in
    the same order), with heavy duplication, skipped (negative) ids and a channel -> column permutation; and against a
    float64 sum within fp32 rounding."""
    import numpy as np
    from graph_recsys_benchmark_amd import engine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(5)
    for n, p, r, nodes in ((1000, 9, 16, 50), (4099, 3, 8, 4000), (1, 1, 4, 3), (12288, 9, 16, 6000), (700, 20, 16, 9), (16384, 2, 4, 100)):
        ids = rng.integers(0, nodes, size=n).astype(np.int64)
        ids[rng.random(n) < 0.1] = -1
        ids[rng.random(n) < 0.03] = nodes + 3                 # outside the table: skipped like the negative ones
        if n > 10:
            ids[:7] = ids[7]                                     # a run of duplicates at the front
        src = rng.standard_normal((n, p * r)).astype(np.float32)
        perm = rng.permutation(p)
        cols = [int(perm[q]) * r for q in range(p)]
        ld = p * r + 4
        want = np.full((nodes, ld), 7.0, dtype=np.float32)      # rows / columns nobody writes keep their value
        want64 = want.astype(np.float64)
        for i in np.unique(ids[(ids >= 0) & (ids < nodes)]):
            pos = np.nonzero(ids == i)[0]
            acc = src[pos[0]].copy()
            for q in pos[1:]:
                acc = acc + src[q]
            tot = src[pos].astype(np.float64).sum(axis=0)
            for c in range(p):
                want[i, cols[c]:cols[c] + r] = acc[c * r:(c + 1) * r]
                want64[i, cols[c]:cols[c] + r] = tot[c * r:(c + 1) * r]
        dst = torch.full((nodes, ld), 7.0, dtype=torch.float32, device=dev)
        engine.rows_scatter_sum(torch.from_numpy(ids).to(dev), torch.from_numpy(src).to(dev), p, r, cols, dst)
        got = dst.cpu().numpy()
        assert np.array_equal(got, want), (n, p, r, float(np.abs(got - want).max()))
        assert np.abs(got - want64).max() <= 1e-5 * max(1.0, np.abs(want64).max())


def test_training_loss_is_continuous_across_the_hip_head_batch_limit():
    """models/base.py (mirror) `_loss_autograd`: batches of up to ROWS_SCATTER_MAX / 3 = 5461 triples take the one-node HIP head
    (csrc/bpr_train.hip + pea_rows_scatter_sum), larger ones the torch-op route over the same HIP conv stack.  The BPR loss is
    a SUM over triples (reference models/base.py:48), so  loss(5462 triples) - loss(first 5461) = loss(the last one alone),
    and the same for every gradient: checked across the limit, and both routes on the SAME 5461 triples agree."""
    import numpy as np
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from helpers import build_model, random_hin, random_state_dict
    from graph_recsys_benchmark_amd import engine
    n, blocks, rel = random_hin(31, n_user=900, n_item=300, n_attr=20, e_u2i=9000, e_attr=700)
    u2i, a2i = rel['u2i'], rel['a2i']
    flip = lambda e: np.ascontiguousarray(e[::-1])
    edges = [[u2i, flip(u2i)], [a2i, flip(u2i)], [flip(u2i), u2i]]
    model = build_model('gat', n, edges, [2, 2, 2], 32, 32, 16)
    model.load_state_dict(random_state_dict(model, 3, scale=0.2))
    model.train()
    limit = engine.ROWS_SCATTER_MAX // 3
    assert limit == 5461
    rng = np.random.default_rng(9)
    big = np.stack([rng.integers(*blocks['u'], size=limit + 1), rng.integers(*blocks['i'], size=limit + 1),
                    rng.integers(*blocks['i'], size=limit + 1)], axis=1).astype(np.int64)
    bt = torch.from_numpy(big).cuda()

    def run(batch, force_torch=False):
        saved = engine.ROWS_SCATTER_MAX
        if force_torch:
            engine.ROWS_SCATTER_MAX = 0
        try:
            model.zero_grad()
            loss = model.loss(batch)
            loss.backward()
        finally:
            engine.ROWS_SCATTER_MAX = saved
        return float(loss), {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()}

    l_hip, g_hip = run(bt[:limit])                       # HIP head
    l_tor, g_tor = run(bt[:limit], force_torch=True)     # torch-op route on the same triples
    l_big, g_big = run(bt)                               # one triple past the limit: torch-op route
    l_one, g_one = run(bt[limit:])                       # the last triple alone: HIP head
    assert abs(l_hip - l_tor) <= 2e-6 * abs(l_hip)
    assert abs(l_big - (l_hip + l_one)) <= 4e-6 * abs(l_big)
    g_max = max(float(v.abs().max()) for v in g_big.values())
    for k in g_big:
        scale = float(g_big[k].abs().max())
        # two fp32 routes against each other (different summation orders over 5461 triples), not against float64: 1e-3
        assert float((g_hip[k] - g_tor[k]).abs().max()) <= 1e-3 * scale + 1e-6 * g_max, k
        assert float((g_big[k] - (g_hip[k] + g_one[k])).abs().max()) <= 1e-3 * scale + 1e-6 * g_max, k
