"""GPU: KGAT / KGCN with native_kg=True (kg_loss on csrc/transr_train.hip) against the same model with the switch off
(the torch composition) and a float64 restatement, on the TinyKG of tests/test_gpu_dot_models.py."""
import numpy as np
import pytest
import torch

import helpers
from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel
from graph_recsys_benchmark_amd.utils.graph_input import kg_graph_input
from test_gpu_dot_models import TinyKG

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KINDS = ['kgat', 'kgcn']
KG_PARAMS = ('x', 'r', 'proj_mat')


@pytest.fixture(scope='module')
def kg():
    return TinyKG()


def build(kind, ds, native_kg, native_train=False, seed=1):
    torch.manual_seed(seed)

    class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, DEV)

    model = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0.0, native_train=native_train, native_kg=native_kg).to(DEV)
    with torch.no_grad():
        model.x.mul_(4.0)
        model.r.mul_(4.0)
        for name, prm in model.named_parameters():
            if name.endswith('bias'):
                prm.normal_(0.0, 0.1)
    return model


def pair(kind, ds, **kw):
    on, off = build(kind, ds, True, **kw), build(kind, ds, False)
    on.load_state_dict(off.state_dict())
    return on, off


def kg_batch(ds, size=256, seed=6):
    """positive triples of the dataset's edge lists with their edge-type id, uniform random negative tails"""
    rng = np.random.default_rng(seed)
    edges = np.hstack([np.vstack([ei, np.full((1, ei.shape[1]), k, dtype=np.int64)])
                       for k, ei in enumerate(ds.edge_index_nps.values())])
    pick = rng.choice(edges.shape[1], size=size, replace=size > edges.shape[1])
    rows = np.stack([edges[0, pick], edges[1, pick], rng.integers(0, ds.num_nodes, size=size), edges[2, pick]], axis=1)
    return torch.from_numpy(rows.astype(np.int64)).to(DEV)


def cf_batch(ds, size=256, seed=6):
    rng = np.random.default_rng(seed)
    lo = ds.type_accs['iid']
    u2i = ds.edge_index_nps['user2item']
    pick = rng.choice(u2i.shape[1], size=size, replace=False)
    return torch.from_numpy(np.stack([u2i[0, pick], u2i[1, pick], rng.integers(lo, lo + ds.num_iids, size=size)], axis=1)).to(DEV)


def f64_kg_loss_and_grads(model, batch):
    p = {k: getattr(model, k).detach().double().requires_grad_(True) for k in KG_PARAMS}
    head = torch.mm(p['x'][batch[:, 0]], p['proj_mat']) + p['r'][batch[:, 3]]
    pos_diff = head - torch.mm(p['x'][batch[:, 1]], p['proj_mat'])
    neg_diff = head - torch.mm(p['x'][batch[:, 2]], p['proj_mat'])
    loss = -((pos_diff * pos_diff).sum(-1) - (neg_diff * neg_diff).sum(-1)).sigmoid().log().sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize('kind', KINDS)
def test_on_against_off(kg, kind):
    on, off = pair(kind, kg)
    assert on.native_kg and not off.native_kg and not on.native_train
    batch = kg_batch(kg)
    truth_loss, truth = f64_kg_loss_and_grads(off, batch)
    got = {}
    for tag, model in (('on', on), ('off', off)):
        model.train()
        loss = model.kg_loss(batch)
        print('%s %s: loss %.9g truth %.9g' % (kind, tag, float(loss.detach()), truth_loss))
        assert abs(float(loss.detach()) - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-6, tag
        loss.backward()
        got[tag] = {k: v.grad for k, v in model.named_parameters()}
    for name in got['on']:
        if name not in KG_PARAMS:            # the convs take no part in the KG phase: no gradient on either path
            assert got['on'][name] is None and got['off'][name] is None, name
            continue
        assert float(got['on'][name].abs().max()) > 0, name
        helpers.assert_fp32_close(got['on'][name].cpu().numpy(), got['off'][name].cpu().numpy(), truth[name].cpu().numpy(),
                                  what='%s d %s' % (kind, name))


@pytest.mark.parametrize('kind', KINDS)
def test_adam_run_on_kg_loss(kg, kind):
    model = build(kind, kg, True)
    batch = kg_batch(kg)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    model.train()
    losses = []
    for it in range(21):
        opt.zero_grad()
        loss = model.kg_loss(batch)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[20] < losses[0], 'loss did not go down in 20 steps: %r -> %r' % (losses[0], losses[20])


@pytest.mark.parametrize('kind', KINDS)
def test_one_epoch_in_miniature(kg, kind):
    """KG step, attention map, CF step with both switches on; afterwards the evaluation table is the switches-off model's"""
    on, off = pair(kind, kg, native_train=True)
    assert on.native_kg and on.native_train
    opt = torch.optim.Adam(on.parameters(), lr=0.01)
    on.train()
    opt.zero_grad()
    kg_loss = on.kg_loss(kg_batch(kg))
    kg_loss.backward()
    assert bool(torch.isfinite(kg_loss))
    for name in KG_PARAMS:
        assert float(getattr(on, name).grad.abs().max()) > 0, name
    opt.step()
    att_map = on.attention_map()
    opt.zero_grad()
    cf_loss = on.loss(cf_batch(kg), att_map)
    cf_loss.backward()
    assert bool(torch.isfinite(cf_loss))
    assert float(on.x.grad.abs().max()) > 0 and float(on.conv1.bias.grad.abs().max()) > 0
    opt.step()
    off.load_state_dict(on.state_dict())
    for model in (on, off):
        model.cf_eval(model.attention_map())
    assert torch.equal(on.cached_repr, off.cached_repr)


@pytest.mark.parametrize('kind', KINDS)
def test_an_oversized_batch_takes_the_torch_path(kg, kind):
    on, off = pair(kind, kg)
    batch = kg_batch(kg, size=5462)
    grads = {}
    for tag, model in (('on', on), ('off', off)):
        model.train()
        loss = model.kg_loss(batch)
        loss.backward()
        grads[tag] = (loss.detach(), {k: getattr(model, k).grad for k in KG_PARAMS})
    assert torch.equal(grads['on'][0], grads['off'][0])
    for name in KG_PARAMS:
        assert torch.equal(grads['on'][1][name], grads['off'][1][name]), name


@pytest.mark.parametrize('kind', KINDS)
def test_eval_mode(kg, kind):
    model = build(kind, kg, True)
    batch = kg_batch(kg)
    model.train()
    trained = model.kg_loss(batch)
    assert trained.requires_grad
    model.kg_eval()
    assert not model.training
    with torch.no_grad():
        evaluated = model.kg_loss(batch)
    assert not evaluated.requires_grad and torch.equal(trained.detach(), evaluated)
