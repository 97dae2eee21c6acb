"""CPU: what the KG-phase entry points (include/peahip.h: pea_transr_*) decide without a device -- the supported widths, the
workspace sizes, every argument error (returned before anything is launched, so no GPU is needed to see it) -- and that KGAT
and KGCN take native_kg=True without changing what kg_loss computes on the CPU."""
import ctypes as C

import pytest
import torch

from graph_recsys_benchmark_amd import _lib, engine
from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel
from graph_recsys_benchmark_amd.utils.graph_input import kg_graph_input

ERR_ARG, ERR_NOMEM = -1, -4
WIDTHS = {0: 0, 4: 1, 6: 0, 20: 1, 64: 1, 128: 1, 132: 0}

_keep = []


def fake(nbytes=4096, misalign=0):
    """A 16-byte aligned host address (+ misalign) that stands in for a device pointer: the calls below fail validation
    before they would read through it."""
    buf = C.create_string_buffer(nbytes + 32)
    _keep.append(buf)
    return C.c_void_p(((C.addressof(buf) + 15) & ~15) + misalign)


def test_supported_widths():
    lib = _lib.load()
    for emb, want in WIDTHS.items():
        assert lib.pea_transr_supported(emb) == want, emb
    assert lib.pea_transr_supported(-4) == 0
    assert engine.transr_supported(64, 5461) and not engine.transr_supported(64, 5462)
    assert not engine.transr_supported(132, 64) and not engine.transr_supported(6, 64)


def test_workspace_is_nonzero_exactly_where_supported():
    lib = _lib.load()
    for emb, want in WIDTHS.items():
        for b in (0, 1, 1000, 5461):
            assert (lib.pea_transr_train_workspace_bytes(b, emb) > 0) == bool(want), (b, emb)
    assert lib.pea_transr_train_workspace_bytes(-1, 64) == 0
    # one dproj partial per workgroup: more quadruples never need less
    assert lib.pea_transr_train_workspace_bytes(1000, 64) >= lib.pea_transr_train_workspace_bytes(16, 64)


def call(**over):
    a = dict(B=100, emb=16, x=fake(), ldx=16, num_nodes=50, proj=fake(), r=fake(), ldr=16, num_rel=3, quads=fake(), quad_stride=4,
             loss=fake(), pos=fake(), neg=fake(), grad_rows=fake(), grad_rel=fake(), dproj=fake(), ws=fake(), ws_bytes=1 << 40,
             stream=None)
    a.update(over)
    return _lib.load().pea_transr_train(a['B'], a['emb'], a['x'], a['ldx'], a['num_nodes'], a['proj'], a['r'], a['ldr'],
                                        a['num_rel'], a['quads'], a['quad_stride'], a['loss'], a['pos'], a['neg'], a['grad_rows'],
                                        a['grad_rel'], a['dproj'], a['ws'], a['ws_bytes'], a['stream'])


def case_id(over):
    """repr of the overrides with a stand-in pointer shown as 'ptr': its address differs from process to process, and a
    test id must not"""
    return repr({k: 'ptr' if isinstance(v, C.c_void_p) else v for k, v in over.items()})


BAD = [dict(x=None), dict(r=None), dict(proj=None), dict(x=fake(misalign=4)), dict(r=fake(misalign=8)),
       dict(proj=fake(misalign=4)), dict(quad_stride=3), dict(ldx=12), dict(ldx=18), dict(ldr=12), dict(ldr=18), dict(num_rel=0),
       dict(num_nodes=0), dict(pos=None), dict(neg=None), dict(grad_rows=None), dict(grad_rel=None), dict(dproj=None),
       dict(grad_rows=None, grad_rel=None), dict(grad_rel=None, dproj=None), dict(emb=6), dict(emb=132), dict(emb=0), dict(B=-1),
       dict(quads=None), dict(loss=None), dict(ws=None)]


@pytest.mark.parametrize('over', BAD, ids=[case_id(o) + ('#%d' % i) for i, o in enumerate(BAD)])
def test_argument_errors_need_no_device(over):
    assert call(**over) == ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('grads', [True, False])
def test_short_workspace(grads):
    need = _lib.load().pea_transr_train_workspace_bytes(100, 16)
    none = {} if grads else dict(grad_rows=None, grad_rel=None, dproj=None)
    assert call(ws_bytes=need - 1, **none) == ERR_NOMEM


class _DS:
    """two typed relations over 12 nodes, enough to construct the models on the CPU"""
    num_nodes, num_edge_types = 12, 2
    edge_index_nps = {'user2item': torch.tensor([[0, 1, 2, 3], [6, 7, 8, 9]]).numpy(),
                      'ent2item': torch.tensor([[10, 11], [6, 7]]).numpy()}

    def __getitem__(self, key):
        return getattr(self, key)


@pytest.mark.parametrize('kind', ['kgat', 'kgcn'])
def test_models_take_native_kg_and_the_cpu_kg_loss_is_unchanged(kind):
    class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, 'cpu')

    ds = _DS()
    on = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0.1, native_kg=True)
    off = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0.1)
    assert on.native_kg is True and off.native_kg is False and on.native_train is False
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    off.load_state_dict(on.state_dict(), strict=True)
    g = torch.Generator().manual_seed(5)
    batch = torch.stack([torch.randint(0, 12, (40,), generator=g), torch.randint(0, 12, (40,), generator=g),
                         torch.randint(0, 12, (40,), generator=g), torch.randint(0, 2, (40,), generator=g)], dim=1)
    for model in (on, off):
        model.train()
    a, b = on.kg_loss(batch), off.kg_loss(batch)
    assert torch.equal(a, b) and bool(torch.isfinite(a))
    a.backward()
    b.backward()
    for name in ('x', 'r', 'proj_mat'):
        assert torch.equal(getattr(on, name).grad, getattr(off, name).grad), name
