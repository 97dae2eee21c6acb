"""CPU: HeRecRecsysModel against the reference fixture (tests/golden/herec_small.npz, written by tests/make_herec_golden.py from
the reference's models/herec.py) and the float64 restatement (tests/herec_ref.py): the state-dict layout, the torch
composition's pred / loss / gradients, the torch-built catalogue table, the eval-mode loss, and what the HIP entry points
(include/peahip.h: pea_herec_*) decide without a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import herec_ref
from graph_recsys_benchmark_amd import _lib, engine
from graph_recsys_benchmark_amd.models import HeRecRecsysModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'herec_small.npz')
ERR_ARG, ERR_NOMEM = -1, -4
PROMISED = [(d, m) for d in range(4, 65, 4) for m in (1, 2, 3, 4)] + [(128, 1)]
GRADS = {'d_user_emb': 'user_emb.weight', 'd_item_emb': 'item_emb.weight', 'd_user_rk_bias': 'user_rk_bias.weight',
         'd_item_rk_bias': 'item_rk_bias.weight'}


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope='module')
def truth(golden):
    return herec_ref.run(herec_ref.golden_inputs(golden), torch.float64)


def model_of(inp, native=False):
    d = inp['w'].shape[1]
    model = HeRecRecsysModel(embeddings=inp['tables'], num_uids=inp['user_emb'].shape[0], num_iids=inp['item_emb'].shape[0],
                             acc_uids=inp['acc_uids'], acc_iids=inp['acc_iids'], embedding_dim=d, native=native)
    return herec_ref.load_model(model, inp)


def test_state_dict_is_the_reference_layout(golden):
    inp = herec_ref.golden_inputs(golden)
    torch.manual_seed(0)
    model = HeRecRecsysModel(embeddings=inp['tables'], num_uids=60, num_iids=90, acc_uids=0, acc_iids=60, embedding_dim=20)
    want = {k[3:]: v for k, v in golden.items() if k.startswith('sd.')}
    sd = model.state_dict()
    assert sorted(sd.keys()) == sorted(want.keys())
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
    model.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()}, strict=True)
    assert model.scorer == 'dot' and model.native is True
    assert not any(t.requires_grad for t in model.rk_embeddings)
    with pytest.raises(NotImplementedError):
        model.shard(0, 2)


def test_reset_parameters_glorots_what_the_reference_glorots():
    torch.manual_seed(3)
    tables = [torch.randn(30, 8), torch.randn(30, 8)]
    model = HeRecRecsysModel(embeddings=tables, num_uids=10, num_iids=15, acc_uids=0, acc_iids=10, embedding_dim=8)
    for t, fan in ((model.emb_trans[0].weight, 16), (model.user_emb.weight, 18), (model.item_rk_bias.weight, 23)):
        assert float(t.detach().abs().max()) <= (6.0 / fan) ** 0.5 + 1e-6
    bias = model.emb_trans[1].bias.detach().clone()
    model.reset_parameters()
    assert torch.equal(bias, model.emb_trans[1].bias)          # the Linear biases keep their own init


def test_composition_reproduces_the_fixture(golden, truth):
    inp = herec_ref.golden_inputs(golden)
    model = model_of(inp).train()
    batch = torch.stack([inp['unids'], inp['inids'], inp['labels'].long()], dim=1)
    pred = model.predict(inp['unids'], inp['inids'])
    loss = model.loss(batch)
    loss.backward()
    helpers.assert_fp32_close(pred.detach().numpy(), golden['pred'], truth['pred'], what='pred')
    helpers.assert_fp32_close(loss.detach().numpy().reshape(1), golden['loss'].reshape(1), truth['loss'].reshape(1), what='loss')
    for key, name in GRADS.items():
        helpers.assert_fp32_close(dict(model.named_parameters())[name].grad.numpy(), golden['grad.' + name], truth[key], what=name)
    for m in range(3):
        helpers.assert_fp32_close(model.emb_trans[m].weight.grad.numpy(), golden['grad.emb_trans.%d.weight' % m], truth['d_w'][m],
                                  what='dW %d' % m)
        helpers.assert_fp32_close(model.emb_trans[m].bias.grad.numpy(), golden['grad.emb_trans.%d.bias' % m], truth['d_b'][m],
                                  what='db %d' % m)


def test_torch_table_row_dots_are_the_scores(golden):
    inp = herec_ref.golden_inputs(golden)
    model = model_of(inp).eval()
    table = model.cached_repr
    assert tuple(table.shape) == (200, 24) and not table.requires_grad
    u = torch.arange(0, 60).repeat_interleave(90)
    i = torch.arange(60, 150).repeat(60)
    with torch.no_grad():
        fwd = model.forward(u, i).numpy()
    dots = (table[u] * table[i]).sum(-1).numpy()
    want = herec_ref.pred_of(inp, {k: inp[k].double() for k in herec_ref.KEYS}, u, i)[0].numpy()
    helpers.assert_fp32_close(dots, fwd, want, what='row dots')
    helpers.assert_fp32_close(table.numpy(), herec_ref.table_of(inp, torch.float32), herec_ref.table_of(inp), what='table')
    assert not table[150:].any() and not table[:, 22:].any()
    assert bool((table[:60, 20] == 1).all()) and bool((table[60:150, 21] == 1).all())
    assert np.array_equal(model.predict(u, i).detach().numpy(), fwd)          # the CPU has no kernel: predict stays the composition


def test_eval_loss_is_the_reference_form(golden):
    inp = herec_ref.golden_inputs(golden)
    model = model_of(inp).eval()
    g = torch.Generator().manual_seed(1)
    batch = torch.stack([torch.full((9,), 7), torch.full((9,), 60 + 4), 60 + torch.randint(0, 90, (9,), generator=g)], dim=1)
    p = {k: inp[k].double() for k in herec_ref.KEYS}
    pos = herec_ref.pred_of(inp, p, batch[:1, 0], batch[:1, 1])[0]
    neg = herec_ref.pred_of(inp, p, batch[:, 0], batch[:, 2])[0]
    want = (((pos - 1.0) ** 2).sum() + (neg ** 2).sum()) / 10.0
    with torch.no_grad():
        got = model.loss(batch)
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    scores = torch.cat([pos, neg]).float().unsqueeze(0)
    _, rank, auc, loss = model.rank_eval(batch[:1, 0], torch.cat([batch[:1, 1], batch[:, 2]]).unsqueeze(0))
    assert abs(float(loss[0]) - float(want)) <= 1e-5 * abs(float(want))
    assert int(rank[0]) == int((scores[0, 1:] > scores[0, 0]).sum())
    with pytest.raises(RuntimeError):
        model.train().rank_eval(batch[:1, 0], batch[:1, 1:])


def test_supported_shapes_and_workspace():
    lib = _lib.load()
    for d, m in PROMISED:
        assert lib.pea_herec_supported(d, m) == 1, (d, m)
        for b in (0, 1, 1000, 5000):
            assert lib.pea_herec_train_workspace_bytes(b, d, m) >= 512, (b, d, m)
    for d, m in [(6, 1), (64, 0), (64, engine.HEREC_MAX_TABLES + 1), (0, 1), (132, 1), (-4, 1), (128, 2)]:
        assert lib.pea_herec_supported(d, m) == 0, (d, m)
        assert lib.pea_herec_train_workspace_bytes(1000, d, m) == 0, (d, m)
    assert lib.pea_herec_train_workspace_bytes(-1, 64, 2) == 0
    # one dW partial per workgroup: more pairs never need less
    assert lib.pea_herec_train_workspace_bytes(5000, 64, 2) >= lib.pea_herec_train_workspace_bytes(16, 64, 2)
    assert engine.herec_supported(64, 2, engine.ROWS_SCATTER_MAX) and not engine.herec_supported(64, 2, engine.ROWS_SCATTER_MAX + 1)
    assert not engine.herec_supported(6, 1) and not engine.herec_supported(128, 2)


_keep = []


def fake(nbytes=4096, misalign=0):
    """A 16-byte aligned host address (+ misalign) that stands in for a device pointer: the calls below fail validation
    before they would read through it."""
    buf = C.create_string_buffer(nbytes + 32)
    _keep.append(buf)
    return C.c_void_p(((C.addressof(buf) + 15) & ~15) + misalign)


def call(**over):
    a = dict(B=100, D=16, M=2, tables=[fake(), fake()], ld=[16, 16], w=fake(), b=fake(), ue=fake(), ie=fake(), urk=fake(), irk=fake(),
             acc_u=0, num_u=20, acc_i=20, num_i=30, N=60, unids=fake(), inids=fake(), labels=fake(), loss=fake(), pred=fake(),
             dw=fake(), db=fake(), g_user=fake(), g_item=fake(), ws=fake(), ws_bytes=1 << 40)
    a.update(over)
    tables = (C.c_void_p * len(a['tables']))(*[t.value if t is not None else None for t in a['tables']])
    ld = (C.c_int64 * len(a['ld']))(*a['ld'])
    return _lib.load().pea_herec_train(a['B'], a['D'], a['M'], tables, ld, a['w'], a['b'], a['ue'], a['ie'], a['urk'], a['irk'],
                                       a['acc_u'], a['num_u'], a['acc_i'], a['num_i'], a['N'], a['unids'], a['inids'], a['labels'],
                                       a['loss'], a['pred'], a['dw'], a['db'], a['g_user'], a['g_item'], a['ws'], a['ws_bytes'], None)


BAD = [dict(w=None), dict(b=None), dict(ue=None), dict(irk=None), dict(w=fake(misalign=4)), dict(urk=fake(misalign=8)),
       dict(tables=[fake(), None]), dict(tables=[fake(misalign=4), fake()]), dict(ld=[16, 12]), dict(ld=[18, 16]), dict(D=6),
       dict(D=132), dict(M=0), dict(M=5), dict(B=-1), dict(N=0), dict(num_u=0), dict(num_i=0), dict(acc_u=-1), dict(acc_i=40),
       dict(unids=None), dict(labels=None), dict(loss=None), dict(ws=None), dict(dw=None), dict(db=None), dict(g_user=None),
       dict(g_item=None, dw=None), dict(g_user=fake(misalign=4))]


@pytest.mark.parametrize('idx', range(len(BAD)))
def test_argument_errors_need_no_device(idx):
    assert call(**BAD[idx]) == ERR_ARG, BAD[idx]
    assert _lib.last_error()


@pytest.mark.parametrize('grads', [True, False])
def test_short_workspace(grads):
    need = _lib.load().pea_herec_train_workspace_bytes(100, 16, 2)
    none = {} if grads else dict(dw=None, db=None, g_user=None, g_item=None)
    assert call(ws_bytes=need - 1, **none) == ERR_NOMEM


def test_table_rejects_overlapping_blocks():
    tables = (C.c_void_p * 1)(fake().value)
    ld = (C.c_int64 * 1)(16)
    args = (fake(), fake(), fake(), fake(), fake(), fake())
    lib = _lib.load()
    assert lib.pea_herec_table(16, 1, tables, ld, *args, 0, 20, 10, 30, 60, fake(), None) == ERR_ARG
    assert lib.pea_herec_table(16, 1, tables, ld, *args, 0, 20, 20, 30, 60, None, None) == ERR_ARG
