"""GPU: the schedules the benchmark times -- the two-step inference schedule (csrc/mlp2.hip, pea_model::fused2) and the two-step
training schedule (csrc/mlp2_bwd.hip, pea_model::fused2_train) -- against fixtures written by the reference's own models/base.py
at its default widths (tests/golden/headline_*.npz: emb == hidden in {64, 128}, repr 16, one head, the nine 2-step metapaths of
the Movielens latest-small branch; tests/test_headline_golden_cpu.py holds the fixtures against the oracle and the restatement).

Forward: stack, fused table, both ablation tables, scores and losses under the rule of the parity tests (rtol 1e-5 / atol 1e-6
through helpers.assert_fp32_close / assert_fused_close with float64 as truth), on the default schedule, on the level-wise one
(PEA_FUSED2=0) and with PEA_CHUNK=64 (item 1 of user2item, about 350 in-edges, becomes a hub row of several chunks); the launch
log says which schedule ran.  Training step: the loss against the reference's float64 loss and every parameter gradient against
the gradients of the reference's own loss.backward() (float64 run), under the gradient rule of tests/test_gpu_backward.py
(helpers.grad_rule_fraction <= 1), on the default schedule and on the level-wise one (PEA_FUSED2_TRAIN=0);
_Layout.two_step_train says which ran.  The entity-aware step runs entity_kernel<16> with gradient rows.  Two negative controls
show that the comparisons can fail: GCN normalised from the other degree side, and fc1.weight scaled by 1.002.

Measured fractions of the gradient rule on an MI355X (worst tensor in brackets); the reference's own float32 run uses 0.0123 /
0.0469 / 0.0068 / 0.0264 of it on the four cases:

    case                    two-step schedule                       level-wise schedule
    headline_gat_att        0.0035 (a last layer's att_i)           0.0092 (a last layer's att_i)
    headline_gcn_att        0.0164 (att)                            0.0068 (att)
    headline_sage_att       0.0082 (a last layer's lin_rel.bias)    0.0093 (a last layer's lin_rel.bias)
    headline_gcn_att_w128   0.0116 (a last layer's weight)          0.0121 (a last layer's weight)
    headline_gat_att, entity-aware step (two-step schedule): 0.0035 (a last layer's att_i)
    negative control, fc1.weight x 1.002: 19.9 times the rule (att)
"""
import numpy as np
import pytest
import torch

import helpers as H
from test_gpu_edge_cases import _kernel_names_of_one_forward
from test_headline_golden_cpu import CASES, f64_truth, headline, stored_grads

pytestmark = pytest.mark.gpu
KNOBS = ('PEA_FUSED2', 'PEA_FUSED2_TRAIN', 'PEA_CHUNK')


def _np(t):
    return t.detach().cpu().numpy()


def _set_env(monkeypatch, **env):
    """every knob is read when a plan or an engine is made: set them before the model is built"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _model(g, state_dict=None, **kw):
    m = g.meta
    return H.build_model(g.kind, m['num_nodes'], g.edges, g.steps, m['emb_dim'], m['hidden_size'], m['repr_dim'], heads=1,
                         channel_aggr='att', state_dict=state_dict or g.state_dict, **kw)


def _assert_forward_matches_the_fixture(model, g):
    t, att = f64_truth(g), g.state_dict['att']
    model.eval()
    with torch.no_grad():
        fused, stack = model.forward(return_stack=True)
    fused, stack = _np(fused), _np(stack)
    want_stack = np.stack([g.out['channel/%d' % p] for p in range(g.P)], axis=1)
    H.assert_fp32_close(stack, want_stack, t['stack'], what='stack')
    H.assert_fused_close(fused, stack, g.out['repr'], t['fused'], att, truth_stack=t['stack'], what='fused')
    H.assert_fused_close(_np(model.cached_repr), stack, g.out['repr'], t['fused'], att, truth_stack=t['stack'], what='cached_repr')
    for masked, truth in t['masked'].items():
        model.eval(masked)
        zeroed, t_zeroed = stack.copy(), t['stack'].copy()
        zeroed[:, masked] = 0
        t_zeroed[:, masked] = 0
        H.assert_fused_close(_np(model.cached_repr), zeroed, g.out['repr_mask%d' % masked], truth, att, truth_stack=t_zeroed,
                             what='eval(%d)' % masked)
    model.eval()
    bt = torch.from_numpy(g.batch).cuda()
    H.assert_fp32_close(_np(model.predict(bt[:, 0], bt[:, 1])).reshape(-1), g.out['pos'], t['pos'], what='pos')
    H.assert_fp32_close(_np(model.predict(bt[:, 0], bt[:, 2])).reshape(-1), g.out['neg'], t['neg'], what='neg')
    np.testing.assert_allclose(float(model.loss(bt)), g.out['loss_eval'], rtol=1e-5)
    model.train()
    with torch.no_grad():
        np.testing.assert_allclose(float(model.loss(bt)), g.out['loss_train'], rtol=1e-5)


FORWARD_RUNS = ([(name, sched) for name in sorted(CASES) for sched in ('two_step', 'levelwise')] +
                [(name, 'two_step_chunk64') for name in ('headline_gat_att', 'headline_gcn_att', 'headline_sage_att')])


@pytest.mark.parametrize('name,sched', FORWARD_RUNS, ids=['%s-%s' % r for r in FORWARD_RUNS])
def test_forward_matches_the_reference_fixture(name, sched, monkeypatch):
    g = headline(name)[0]
    _set_env(monkeypatch, **{'two_step': {}, 'levelwise': {'PEA_FUSED2': 0}, 'two_step_chunk64': {'PEA_CHUNK': 64}}[sched])
    model = _model(g)
    model.eval()
    names = _kernel_names_of_one_forward(model)
    assert ('mlp2_fused' in names) == (sched != 'levelwise'), sorted(names)
    plan = model._engine.plan
    info = plan.relation_info(plan.relation_of[0][0])               # user2item: item 1 collects about 350 edges
    assert 300 < info['max_degree'] <= 512
    if sched == 'two_step_chunk64':
        assert info['hub_rows'] >= 1 and info['hub_chunks'] >= 6, info
    else:
        assert info['hub_rows'] == 0 and info['long_items'] >= 1 and info['short_rows'] >= 1, info
    _assert_forward_matches_the_fixture(model, g)


def test_forward_comparison_fails_on_the_other_gcn_degree_side(monkeypatch):
    """negative control: GCNConv normalised by the target's degree is another model, and the comparison says so"""
    g = headline('headline_gcn_att')[0]
    _set_env(monkeypatch)
    model = _model(g, gcn_deg_from='col')
    model.eval()
    assert 'mlp2_fused' in _kernel_names_of_one_forward(model)
    with pytest.raises(AssertionError):
        _assert_forward_matches_the_fixture(model, g)


def _training_step(model, batch):
    """(loss, {parameter: gradient}) of model.loss(batch).backward() in training mode"""
    model.train()
    model.zero_grad()
    loss = model.loss(torch.from_numpy(batch).cuda())
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is not None, k
    return float(loss.detach()), {k: _np(p.grad).astype(np.float64) for k, p in model.named_parameters()}


def _two_step_train(model):
    from graph_recsys_benchmark_amd.autograd import _Layout
    return _Layout(model._train_engine).two_step_train


@pytest.mark.parametrize('sched', ['two_step', 'levelwise'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_training_step_matches_the_reference_gradients(name, sched, monkeypatch):
    g, grads, _ = headline(name)
    _set_env(monkeypatch, **({} if sched == 'two_step' else {'PEA_FUSED2_TRAIN': 0}))
    model = _model(g)
    loss, got = _training_step(model, g.batch)
    assert _two_step_train(model) == (sched == 'two_step')
    np.testing.assert_allclose(loss, float(grads['loss64']), rtol=2e-5)
    want = stored_grads(grads)
    assert set(got) == set(want)
    frac, worst = H.grad_rule_fraction(got, want)
    print('%s, %s schedule: %.4f of the gradient rule (%s)' % (name, sched, frac, worst))
    assert frac <= 1.0, (frac, worst)


def test_entity_aware_training_step_matches_the_reference_gradients(monkeypatch):
    """csrc/entity.hip at emb 64 (entity_kernel<16>) with gradient rows, inside a whole training step: the regulariser's
    gradient lands in x.grad on top of the conv stack's; every other gradient is the plain step's."""
    g, grads, _ = headline('headline_gat_att')
    _set_env(monkeypatch)
    model = _model(g, entity_aware=True)
    loss, got = _training_step(model, g.batch9)
    assert _two_step_train(model)
    np.testing.assert_allclose(loss, g.out['loss_train_ea'], rtol=1e-5)
    np.testing.assert_allclose(loss, float(grads['loss64_ea']), rtol=2e-5)
    want = stored_grads(grads)
    want['x'] = grads['grad_ea/x'].astype(np.float64)
    assert np.abs(want['x'] - grads['grad/x']).max() > 1e-3 * np.abs(want['x']).max()       # the term shows in the gradient
    frac, worst = H.grad_rule_fraction(got, want)
    print('headline_gat_att, entity-aware step: %.4f of the gradient rule (%s)' % (frac, worst))
    assert frac <= 1.0, (frac, worst)
    plain_frac, _ = H.grad_rule_fraction({'x': got['x']}, {'x': grads['grad/x'].astype(np.float64)})
    assert plain_frac > 1.0                      # and the comparison would notice a step that left the term out


def test_gradient_comparison_fails_on_a_slightly_different_model(monkeypatch):
    """negative control: fc1.weight scaled by 1.002 moves the gradients by more than the rule allows"""
    g, grads, _ = headline('headline_gcn_att')
    _set_env(monkeypatch)
    sd = dict(g.state_dict)
    sd['fc1.weight'] = (sd['fc1.weight'] * np.float32(1.002)).astype(np.float32)
    model = _model(g, state_dict=sd)
    _, got = _training_step(model, g.batch)
    assert _two_step_train(model)
    frac, worst = H.grad_rule_fraction(got, stored_grads(grads))
    print('fc1.weight x 1.002: %.2f of the gradient rule (%s)' % (frac, worst))
    assert frac > 1.0
