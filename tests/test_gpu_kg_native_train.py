"""GPU: KGAT / KGCN / NGCF with native_train=True (aggregate -> csrc/kg_update.hip per conv, then csrc/dot_train.hip)
against the same model with the switch off (today's autograd path) and the float64 restatement of
tests/test_gpu_dot_models.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel, NGCFRecsysModel
from graph_recsys_benchmark_amd.utils import seen_items_csr
from graph_recsys_benchmark_amd.utils.graph_input import kg_graph_input
from test_gpu_dot_models import TinyKG, restate_att, restate_table

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KINDS = ['kgat', 'kgcn', 'ngcf']


@pytest.fixture(scope='module')
def kg():
    return TinyKG()


def build(kind, ds, native, hidden=16, dropout=0.0, seed=1):
    torch.manual_seed(seed)
    if kind == 'ngcf':
        u2i = torch.from_numpy(ds.edge_index_nps['user2item']).to(DEV)
        edge_index = torch.cat([u2i, torch.flip(u2i, dims=[0])], dim=1).contiguous()

        class Model(NGCFRecsysModel):
            def update_graph_input(self, dataset):
                return edge_index

        return Model(dataset=ds, emb_dim=16, hidden_size=hidden, dropout=dropout, entity_aware=False, entity_aware_coff=0.0,
                     if_use_features=False, native_train=native).to(DEV)

    class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, DEV)

    model = Model(dataset=ds, emb_dim=16, hidden_size=hidden, dropout=dropout, native_train=native).to(DEV)
    with torch.no_grad():
        model.x.mul_(4.0)
        model.r.mul_(4.0)
        for name, prm in model.named_parameters():
            if name.endswith('bias'):
                prm.normal_(0.0, 0.1)
    return model


def pair(kind, ds, **kw):
    on, off = build(kind, ds, True, **kw), build(kind, ds, False, **kw)
    on.load_state_dict(off.state_dict())
    return on, off


def make_batch(ds, size=256, seed=6):
    rng = np.random.default_rng(seed)
    lo = ds.type_accs['iid']
    u2i = ds.edge_index_nps['user2item']
    pick = rng.choice(u2i.shape[1], size=size, replace=False)
    return torch.from_numpy(np.stack([u2i[0, pick], u2i[1, pick], rng.integers(lo, lo + ds.num_iids, size=size)], axis=1)).to(DEV)


def loss_of(kind, model, batch, att=None):
    if kind == 'ngcf':
        return model.loss(batch)
    return model.loss(batch, model.attention_map() if att is None else att)


def f64_loss_and_grads(kind, model, batch):
    """The float64 restatement under autograd, with the attention map held constant as both model paths hold it."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in model.state_dict().items()}
    att = None
    if kind != 'ngcf':
        with torch.no_grad():
            att = restate_att(kind, p, model.edge_index, model.edge_attr)
    table = restate_table(kind, p, model.edge_index, att)
    pos = (table[batch[:, 0]] * table[batch[:, 1]]).sum(-1)
    neg = (table[batch[:, 0]] * table[batch[:, 2]]).sum(-1)
    loss = -F.logsigmoid(pos - neg).sum()
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize('kind', KINDS)
def test_loss_and_gradients_against_the_autograd_path(kg, kind):
    on, off = pair(kind, kg)
    batch = make_batch(kg)
    truth_loss, truth = f64_loss_and_grads(kind, off, batch)
    got = {}
    for tag, model in (('on', on), ('off', off)):
        model.train()
        loss = loss_of(kind, model, batch)
        assert abs(float(loss.detach()) - truth_loss) <= 1e-5 * abs(truth_loss) + 1e-6, tag
        loss.backward()
        got[tag] = {k: v.grad for k, v in model.named_parameters()}
    assert on.cached_repr is None and off.cached_repr.requires_grad
    for name in got['on']:
        if name in ('r', 'proj_mat'):       # only the (constant) attention map reads them: no gradient on either path
            assert got['on'][name] is None and got['off'][name] is None
            continue
        helpers.assert_fp32_close(got['on'][name].cpu().numpy(), got['off'][name].cpu().numpy(), truth[name].cpu().numpy(),
                                  what='%s d %s' % (kind, name))


@pytest.mark.parametrize('kind', KINDS)
def test_dropout(kg, kind):
    batch = make_batch(kg)
    plain = build(kind, kg, True)
    plain.train()
    base = float(loss_of(kind, plain, batch).detach())
    model = build(kind, kg, True, dropout=0.5)
    model.train()
    torch.manual_seed(3)
    loss = loss_of(kind, model, batch)
    assert bool(torch.isfinite(loss)) and float(loss.detach()) != base
    loss.backward()
    for name, prm in model.named_parameters():
        if name in ('r', 'proj_mat'):
            continue
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
        assert float(prm.grad.abs().max()) > 0, name + ': zero gradient'


@pytest.mark.parametrize('kind', KINDS)
def test_training_run_then_evaluation(kg, kind):
    on, off = pair(kind, kg)
    batch = make_batch(kg)
    opt = torch.optim.Adam(on.parameters(), lr=0.01)
    on.train()
    losses = []
    for it in range(21):
        opt.zero_grad()
        loss = loss_of(kind, on, batch)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[20] < losses[0], 'loss did not go down in 20 steps: %r -> %r' % (losses[0], losses[20])
    u = torch.arange(8, device=DEV)
    with pytest.raises(RuntimeError, match='native_train'):
        on.predict(u, u + kg.type_accs['iid'])
    # after evaluation the table and the recommendations are those of the flag-off model with the same weights
    off.load_state_dict(on.state_dict())
    for model in (on, off):
        if kind == 'ngcf':
            model.eval()
        else:
            model.cf_eval(model.attention_map())
    assert torch.equal(on.cached_repr, off.cached_repr)
    lo, n = kg.type_accs['iid'], kg.num_iids
    u_t = torch.tensor(list(kg.test_pos_unid_inid_map.keys()), device=DEV)
    exclude = seen_items_csr(kg.edge_index_nps['user2item'], u_t, (lo, lo + n))
    a, b = on.recommend(u_t, 10, (lo, lo + n), exclude=exclude), off.recommend(u_t, 10, (lo, lo + n), exclude=exclude)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(on.predict(u, u + lo), off.predict(u, u + lo))


@pytest.mark.parametrize('kind', KINDS)
def test_unsupported_widths_train_through_the_fallback(kg, kind):
    """hidden_size = 144: conv1 is 16 -> 144, wider than csrc/kg_update.hip takes (128), so the whole step stays on autograd.
    (hidden_size = 20, widths 20 / 10 / 5, cannot be the case here: pea_weighted_aggregate itself takes multiples of 4 only,
    so such a model cannot run a forward on either path -- the next test pins that the switch does not change that.)"""
    model = build(kind, kg, True, hidden=144)
    model.train()
    batch = make_batch(kg, size=64)
    loss = loss_of(kind, model, batch)
    assert model.cached_repr is not None and model.cached_repr.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    assert model.x.grad is not None and float(model.x.grad.abs().max()) > 0


@pytest.mark.parametrize('kind', KINDS)
def test_widths_the_aggregate_refuses_fail_alike_with_the_switch_on_and_off(kg, kind):
    batch = make_batch(kg, size=64)
    for native in (True, False):
        model = build(kind, kg, native, hidden=20)      # conv2 would aggregate rows of 20, conv3 rows of 10
        model.train()
        with pytest.raises(ValueError, match='multiple of 4'):
            loss_of(kind, model, batch)


def test_an_att_map_that_requires_grad_takes_the_fallback(kg):
    model = build('kgat', kg, True)
    model.train()
    att = model.attention_map().clone().requires_grad_(True)
    loss = model.loss(make_batch(kg, size=64), att)
    loss.backward()
    assert model.cached_repr is not None and att.grad is not None
