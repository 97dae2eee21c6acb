"""CPU: the headline fixtures (tests/golden/headline_*.npz and .grad.npz, written by `python oracle/make_golden.py headline`
from the reference's own models/base.py at its default widths: emb == hidden in {64, 128}, repr 16, one head, the nine 2-step
metapaths of the Movielens latest-small branch) against the project's two yardsticks, without a GPU.

1. Fixture identity: widths, metapaths (every edge list is the relation, or its flip, that graph_input_tables.json names), masks.
2. The C oracle (oracle/pea_oracle.c) against the reference's float32 forward outputs, under the rule of the GPU parity tests
   (rtol 1e-5 / atol 1e-6 through helpers.assert_fp32_close / assert_fused_close, helpers.f64_forward as truth).
3. The float64 restatement (helpers.restated_loss_and_grads, the truth of every gradient test here) against the gradients of the
   reference's own loss.backward(), run in float64 and stored as float32.  Two float64 evaluations of one expression, apart only
   by the storage rounding (2^-24 per element, 3e-4 of a rule whose relative term is 2e-4): at most 1e-2 of the gradient rule.
4. The float32 restatement against the same gradients: at most half of the rule (the convention of test_agg_bwd_matrix_cpu.py),
   and so was the reference's own float32 run when the fixture was written (meta of the .grad.npz).
5. The entity-aware term in float64 (reference models/base.py:50-73) against loss64_ea - loss64 and grad_ea/x - grad/x.

Measured fractions of the gradient rule (helpers.grad_rule_fraction), worst tensor in brackets:

    case                    reference float32 run     restatement float64      restatement float32
    headline_gat_att        0.0123 (fc2.weight)       2.9e-4 (a layer bias)    0.0123 (fc2.weight)
    headline_gcn_att        0.0469 (att)              2.6e-4 (fc2.weight)      0.0470 (att)
    headline_sage_att       0.0068 (lin_rel.bias)     2.4e-4 (lin_rel.bias)    0.0067 (lin_rel.bias)
    headline_gcn_att_w128   0.0264 (a layer bias)     2.3e-4 (a layer weight)  0.0264 (a layer bias)
    entity term, headline_gat_att: x gradient 2.5e-4 of the rule
"""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
from oracle import oracle as orc

CASES = {'headline_gat_att': ('gat', 64, (1, 2, 3, 4, 5, 6, 7, 8, 9)), 'headline_gcn_att': ('gcn', 64, (1, 2, 3, 4, 5, 6, 7, 8, 9)),
         'headline_sage_att': ('sage', 64, (1, 2, 3, 8, 9)), 'headline_gcn_att_w128': ('gcn', 128, (1, 2, 9))}
STORAGE = 1e-2          # share of the gradient rule that rounding the stored gradients to float32 may use (see 3. above)
HEADROOM = 0.5          # share of the rule a float32 evaluation on the CPU may use
SIZE_CAP = 406774       # bytes of tests/golden/checkpoints/PEASage_ea0.pt, the largest file the repository carried before
_CACHE = {}


def headline(name):
    """(GoldenCase, arrays of the .grad.npz, its meta), loaded once"""
    if name not in _CACHE:
        z = np.load(os.path.join(H.GOLDEN, name + '.grad.npz'))
        _CACHE[name] = (H.GoldenCase(name), {k: z[k] for k in z.files if k != 'meta'}, json.loads(bytes(z['meta']).decode()))
    return _CACHE[name]


def stored_grads(arrays, prefix='grad/'):
    return {k[len(prefix):]: v.astype(np.float64) for k, v in arrays.items() if k.startswith(prefix)}


def f64_truth(g):
    """float64 tables of the fixture's model: stack, fused, fused with channel 1 / 6 zeroed, pos, neg, loss"""
    key = g.name + '/truth'
    if key not in _CACHE:
        sd = g.state_dict
        fused, stack = H.f64_forward(g.kind, sd, g.edges, g.steps, 1, 'att')
        att = sd['att'].astype(np.float64).reshape(g.P, -1)

        def fuse(masked):
            x = stack.copy()
            x[:, masked] = 0
            logit = (x * att).sum(-1)
            w = np.exp(logit - logit.max(-1, keepdims=True))
            return (x * (w / w.sum(-1, keepdims=True))[..., None]).sum(1)

        def pred(u, i):
            hdn = np.maximum(np.concatenate([fused[u], fused[i]], -1) @ sd['fc1.weight'].astype(np.float64).T + sd['fc1.bias'], 0)
            return (hdn @ sd['fc2.weight'].astype(np.float64).T + sd['fc2.bias']).reshape(-1)

        b = g.batch
        pos, neg = pred(b[:, 0], b[:, 1]), pred(b[:, 0], b[:, 2])
        _CACHE[key] = dict(stack=stack, fused=fused, masked={m: fuse(m) for m in (1, 6) if m < g.P}, pos=pos, neg=neg,
                           loss=float(np.log1p(np.exp(-(pos - neg))).sum()))
    return _CACHE[key]


def entity_term_f64(x, batch9):
    """(value, gradient with respect to x) of the reference's entity-aware term (models/base.py:50-73) in float64"""
    xd = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    td = torch.from_numpy(batch9)

    def sq(a, b):
        d = xd[td[:, a]] - xd[td[:, b]]
        return (d * d).sum(-1)

    reg = -(((sq(1, 3) - sq(1, 4)) * td[:, 5]).sigmoid().log().sum()) - (((sq(0, 6) - sq(0, 7)) * td[:, 8]).sigmoid().log().sum())
    reg.backward()
    return float(reg.detach()), xd.grad.numpy()


def test_the_headline_names_stay_out_of_the_pea_glob():
    assert not [c for c in H.golden_cases() if 'headline' in c] and all(not c.startswith('pea_') for c in CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture_identity(name):
    g, grads, gmeta = headline(name)
    kind, width, picked = CASES[name]
    m = g.meta
    assert (m['kind'], m['emb_dim'], m['hidden_size'], m['repr_dim'], m['heads'], m['channel_aggr']) == (kind, width, width, 16, 1, 'att')
    assert tuple(m['metapaths']) == picked and g.steps == [2] * len(picked) and not m['entity_aware']
    for suffix in ('.npz', '.grad.npz'):
        assert os.path.getsize(os.path.join(H.GOLDEN, name + suffix)) <= SIZE_CAP
    # the metapaths are the reference's own: relation and direction per (metapath, step) as recorded from update_pea_graph_input
    with open(os.path.join(H.GOLDEN, 'graph_input_tables.json')) as f:
        table = json.load(f)['Movielens/latest-small']
    z = np.load(os.path.join(H.GOLDEN, name + '.npz'))
    rel = {k[len('rel/'):]: z[k] for k in z.files if k.startswith('rel/')}
    assert len(table) == 9 and len(rel) == 8
    for p, q in enumerate(picked):
        for s, (rname, flipped) in enumerate(table[q - 1]):
            want = rel[rname][::-1] if flipped else rel[rname]
            assert g.edges[p][s].dtype == np.int64 and np.array_equal(g.edges[p][s], want), (q, s, rname, flipped)
    if len(picked) == 9:
        assert sum(table[q - 1][1] == ['user2item', 1] for q in picked) == 7 and sum(table[q - 1][1] == ['user2item', 0] for q in picked) == 2
    # the relations connect the node blocks they name; the graph has what the kernels' row forms need
    n, blocks = m['num_nodes'], {k: tuple(v) for k, v in m['blocks'].items()}
    assert n == 136 and blocks['user'] == (0, 40) and blocks['item'] == (40, 96) and max(b[1] for b in blocks.values()) == n - 3
    inside = lambda ids, b: bool(((ids >= b[0]) & (ids < b[1])).all())
    for rname, e in rel.items():
        src, dst = rname.split('2')
        loops = e[0] == e[1]
        assert inside(e[0][~loops], blocks[src]) and inside(e[1][~loops], blocks[dst]), rname
        assert loops.sum() == (7 if rname == 'tag2user' else 0)
    u2i = rel['user2item']
    deg = np.bincount(u2i[1], minlength=n)
    assert 1400 <= u2i.shape[1] <= 1500 and 300 < deg.max() <= 512 and (deg == 0).sum() > n // 2
    assert (np.bincount(u2i[0][u2i[1] == blocks['item'][0]], minlength=40)[:40] >= 1).all()        # every user -> item 0
    assert np.unique(u2i, axis=1).shape[1] < u2i.shape[1]                                          # multi-edges
    assert np.unique(rel['tag2item'], axis=1).shape[1] <= rel['tag2item'].shape[1] - 20            # repeated pairs
    for k in ('year', 'actor', 'director', 'writer', 'genre'):
        assert rel[k + '2item'].shape[1] == 70
    # the batch: 96 triples, six fixed negatives
    b = g.batch
    assert b.shape == (96, 3) and inside(b[:, 0], blocks['user']) and inside(b[:, 1:], blocks['item']) and np.unique(b[:, 2]).size == 6
    assert ('repr_mask1' in g.out) and (('repr_mask6' in g.out) == (g.P > 6))
    if name == 'headline_gat_att':
        b9 = g.batch9
        assert b9.shape == (96, 9) and np.array_equal(b9[:, :3], b) and b9[:, [3, 4, 6, 7]].min() >= 0 and b9[:, [3, 4, 6, 7]].max() < n
        for c in (5, 8):
            assert set(np.unique(b9[:, c])) == {0, 1}
        assert ((b9[:, 5] == 0) & (b9[:, 8] == 0)).any()
        assert 'loss_train_ea' in g.out and 'grad_ea/x' in grads and 'loss64_ea' in grads
    else:
        assert g.batch9 is None and 'grad_ea/x' not in grads
    # one gradient per parameter, stored as float32
    assert set(stored_grads(grads)) == set(g.state_dict)
    assert all(v.dtype == np.float32 and v.shape == g.state_dict[k[5:]].shape for k, v in grads.items() if k.startswith('grad/'))
    assert grads['loss64'].dtype == np.float64 and 0 < gmeta['ref_fp32_rule_fraction'] <= HEADROOM


@pytest.mark.parametrize('name', sorted(CASES))
def test_c_oracle_matches_the_reference_forward(name):
    g, grads, _ = headline(name)
    sd, t = g.state_dict, f64_truth(g)
    att = sd['att']
    fused, stack = orc.pea_forward(g.kind, sd['x'], g.edges, g.channel_params(), g.heads_lists(), att=att, channel_aggr='att',
                                   return_stack=True)
    want_stack = np.stack([g.out['channel/%d' % p] for p in range(g.P)], axis=1)
    H.assert_fp32_close(stack, want_stack, t['stack'], what='stack')
    H.assert_fused_close(fused, stack, g.out['repr'], t['fused'], att, truth_stack=t['stack'], what='repr')
    for masked, truth in t['masked'].items():
        zeroed, t_zeroed = stack.copy(), t['stack'].copy()
        zeroed[:, masked] = 0
        t_zeroed[:, masked] = 0
        H.assert_fused_close(orc.fuse(stack, att, masked=masked), zeroed, g.out['repr_mask%d' % masked], truth, att,
                             truth_stack=t_zeroed, what='repr_mask%d' % masked)
    loss, pos, neg = orc.pea_loss(fused, g.batch, sd['fc1.weight'], sd['fc1.bias'], sd['fc2.weight'], sd['fc2.bias'])
    H.assert_fp32_close(pos, g.out['pos'], t['pos'], what='pos')
    H.assert_fp32_close(neg, g.out['neg'], t['neg'], what='neg')
    np.testing.assert_allclose(loss, g.out['loss_eval'], rtol=1e-5)
    np.testing.assert_allclose(loss, g.out['loss_train'], rtol=1e-5)
    np.testing.assert_allclose(g.out['loss_train'], float(grads['loss64']), rtol=1e-5)
    np.testing.assert_allclose(t['loss'], float(grads['loss64']), rtol=1e-9)
    if g.batch9 is not None:
        np.testing.assert_allclose(loss + 0.1 * orc.entity_reg(sd['x'], g.batch9), g.out['loss_train_ea'], rtol=1e-5)


@pytest.mark.parametrize('name', sorted(CASES))
def test_float64_restatement_matches_the_reference_autograd(name):
    """The restatement is the yardstick of every gradient test of this project; here it meets the reference's own autograd."""
    g, grads, _ = headline(name)
    loss, got = H.restated_loss_and_grads(g.kind, g.state_dict, g.edges, g.steps, 1, 'att', g.batch, dtype=torch.float64)
    np.testing.assert_allclose(loss, float(grads['loss64']), rtol=1e-9)
    want = stored_grads(grads)
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('%s: float64 restatement against the stored reference gradients: %.3e of the rule (%s)' % (name, frac, worst))
    assert frac <= STORAGE, (frac, worst)


@pytest.mark.parametrize('name', sorted(CASES))
def test_float32_restatement_keeps_half_of_the_rule(name):
    g, grads, gmeta = headline(name)
    loss, got = H.restated_loss_and_grads(g.kind, g.state_dict, g.edges, g.steps, 1, 'att', g.batch, dtype=torch.float32)
    np.testing.assert_allclose(loss, float(grads['loss64']), rtol=2e-5)
    frac, worst = H.grad_rule_fraction(got, stored_grads(grads))
    print('%s: float32 restatement %.4f of the rule (%s); the reference\'s float32 run used %.4f (%s)'
          % (name, frac, worst, gmeta['ref_fp32_rule_fraction'], gmeta['ref_fp32_rule_tensor']))
    assert frac <= HEADROOM, (frac, worst)
    assert gmeta['ref_fp32_rule_fraction'] <= HEADROOM
    np.testing.assert_allclose(gmeta['loss32'], g.out['loss_train'], rtol=1e-7)


def test_entity_term_matches_the_reference_autograd():
    g, grads, _ = headline('headline_gat_att')
    reg, dreg = entity_term_f64(g.state_dict['x'], g.batch9)
    coff = 0.1
    np.testing.assert_allclose((float(grads['loss64_ea']) - float(grads['loss64'])) / coff, reg, rtol=1e-9)
    plain, with_term = grads['grad/x'].astype(np.float64), grads['grad_ea/x'].astype(np.float64)
    frac, _ = H.grad_rule_fraction({'x': plain + coff * dreg}, {'x': with_term})
    print('entity term: x gradient %.3e of the rule' % frac)
    assert frac <= STORAGE, frac
    assert np.abs(with_term - plain).max() > 1e-3 * np.abs(plain).max()         # the term is not lost in the plain gradient
    np.testing.assert_allclose(g.out['loss_train_ea'], float(grads['loss64_ea']), rtol=1e-5)
    np.testing.assert_allclose(orc.entity_reg(g.state_dict['x'], g.batch9), reg, rtol=1e-5)
