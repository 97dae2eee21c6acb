"""CPU: what the KGAT / KGCN / NGCF training entry points (include/peahip.h: pea_kg_update_*, pea_dot_bpr_train) decide
without a device -- the supported matrix, the workspace sizes, every argument error (returned before anything is launched,
so no GPU is needed to see it) -- and that the models take native_train=True without changing their state_dict."""
import ctypes as C

import pytest
import torch

from graph_recsys_benchmark_amd import _lib
from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel, NGCFRecsysModel
from graph_recsys_benchmark_amd.nn import KGATConv, KGCNConv, NGCFConv, kg_update_supported
from graph_recsys_benchmark_amd.utils.graph_input import kg_graph_input

KGAT, KGCN, NGCF = _lib.KGU_KGAT, _lib.KGU_KGCN, _lib.KGU_NGCF
ERR_ARG, ERR_NOMEM = -1, -4
GOOD = [(4, 4), (8, 4), (16, 8), (64, 64), (64, 32), (32, 16), (128, 128), (12, 20)]
BAD = [(0, 4), (4, 0), (6, 4), (4, 6), (132, 4), (4, 132), (-4, 4), (4, -4)]

_keep = []


def fake(nbytes=4096):
    """A 16-byte aligned host address that stands in for a device pointer: the calls below fail validation before they
    would read through it."""
    buf = C.create_string_buffer(nbytes + 16)
    _keep.append(buf)
    return C.c_void_p((C.addressof(buf) + 15) & ~15)


def test_supported_matrix():
    lib = _lib.load()
    for kind in (KGAT, KGCN, NGCF):
        for fin, fout in GOOD:
            assert lib.pea_kg_update_supported(kind, fin, fout) == 1, (kind, fin, fout)
        for fin, fout in BAD:
            assert lib.pea_kg_update_supported(kind, fin, fout) == 0, (kind, fin, fout)
    assert lib.pea_kg_update_supported(3, 64, 64) == 0 and lib.pea_kg_update_supported(-1, 64, 64) == 0
    assert kg_update_supported('kgat', 64, 64) and not kg_update_supported('ngcf', 20, 10)


def test_workspace_is_nonzero_exactly_where_supported():
    lib = _lib.load()
    for kind in (KGAT, KGCN, NGCF):
        for fin, fout in GOOD:
            assert lib.pea_kg_update_backward_workspace_bytes(kind, fin, fout) > 0
        for fin, fout in BAD:
            assert lib.pea_kg_update_backward_workspace_bytes(kind, fin, fout) == 0
    assert lib.pea_dot_bpr_train_workspace_bytes(0) > 0 and lib.pea_dot_bpr_train_workspace_bytes(4096) > 0
    assert lib.pea_dot_bpr_train_workspace_bytes(-1) == 0


def fwd_args(**over):
    a = dict(N=100, kind=KGAT, fin=16, fout=8, x=fake(), ldx=16, s=fake(), lds=16, w1=fake(), w2=fake(), bias=fake(),
             slope=0.2, keep=None, keep_scale=1.0, out=fake(), ldo=8, stream=None)
    a.update(over)
    return a


def call_fwd(**over):
    a = fwd_args(**over)
    return _lib.load().pea_kg_update_forward(a['N'], a['kind'], a['fin'], a['fout'], a['x'], a['ldx'], a['s'], a['lds'], a['w1'],
                                             a['w2'], a['bias'], a['slope'], a['keep'], a['keep_scale'], a['out'], a['ldo'],
                                             a['stream'])


def call_bwd(**over):
    a = fwd_args(g=fake(), ldg=8, dx=fake(), lddx=16, ds=fake(), ldds=16, dw1=fake(), dw2=fake(), dbias=fake(), ws=fake(),
                 ws_bytes=1 << 40)
    a.update(over)
    return _lib.load().pea_kg_update_backward(a['N'], a['kind'], a['fin'], a['fout'], a['x'], a['ldx'], a['s'], a['lds'], a['w1'],
                                              a['w2'], a['bias'], a['slope'], a['keep'], a['keep_scale'], a['g'], a['ldg'],
                                              a['dx'], a['lddx'], a['ds'], a['ldds'], a['dw1'], a['dw2'], a['dbias'], a['ws'],
                                              a['ws_bytes'], a['stream'])


SHARED_BAD = [dict(fin=6), dict(fout=6), dict(fin=132), dict(fout=0), dict(fin=-4), dict(kind=3), dict(N=-1),
              dict(x=None), dict(s=None), dict(w1=None), dict(w2=None), dict(kind=NGCF, w2=None, bias=None),
              dict(kind=KGCN), dict(kind=NGCF, bias=fake()),
              dict(ldx=18), dict(ldx=12), dict(lds=18), dict(lds=12)]


def case_id(over):
    """repr of the overrides with a stand-in pointer shown as 'ptr': its address differs from process to process, and a
    test id must not"""
    return repr({k: 'ptr' if isinstance(v, C.c_void_p) else v for k, v in over.items()})


@pytest.mark.parametrize('over', SHARED_BAD + [dict(out=None), dict(ldo=10), dict(ldo=4)], ids=case_id)
def test_forward_argument_errors_need_no_device(over):
    assert call_fwd(**over) == ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('over', SHARED_BAD + [dict(g=None), dict(ldg=10), dict(ldg=4), dict(dx=None), dict(ds=None),
                                               dict(dw1=None), dict(dw2=None), dict(ws=None), dict(lddx=18), dict(lddx=12),
                                               dict(ldds=18), dict(ldds=12)], ids=case_id)
def test_backward_argument_errors_need_no_device(over):
    assert call_bwd(**over) == ERR_ARG
    assert _lib.last_error()


def test_backward_short_workspace():
    need = _lib.load().pea_kg_update_backward_workspace_bytes(KGAT, 16, 8)
    assert call_bwd(ws_bytes=need - 1) == ERR_NOMEM


def call_dot(B=10, widths=(16, 8, 4), lds=None, ptrs=None, num_nodes=100, triples='x', stride=3, loss='x', grad='x', ws='x',
             ws_bytes=1 << 30, n_blocks=None):
    k = len(widths)
    lds = list(widths) if lds is None else lds
    ptr_arr = (C.c_void_p * max(k, 1))(*[(fake().value if ptrs is None else ptrs[i]) for i in range(k)])
    ld_arr = (C.c_int64 * max(k, 1))(*lds)
    w_arr = (C.c_int * max(k, 1))(*widths)
    pick = lambda v: fake() if v == 'x' else v
    return _lib.load().pea_dot_bpr_train(B, k if n_blocks is None else n_blocks, ptr_arr, ld_arr, w_arr, num_nodes, pick(triples),
                                         stride, pick(loss), pick(grad), pick(ws), ws_bytes, None)


@pytest.mark.parametrize('over', [dict(widths=()), dict(widths=(4,) * 5), dict(widths=(16, 6, 4)), dict(widths=(16, 0)),
                                  dict(widths=(128, 128, 4)), dict(widths=(16, 8), lds=[16, 4]), dict(widths=(16, 8), lds=[18, 8]),
                                  dict(widths=(16,), ptrs=[None]), dict(B=-1), dict(num_nodes=0), dict(triples=None),
                                  dict(stride=2), dict(loss=None), dict(grad=None), dict(ws=None)], ids=repr)
def test_dot_bpr_train_argument_errors_need_no_device(over):
    assert call_dot(**over) == ERR_ARG
    assert _lib.last_error()


def test_dot_bpr_train_short_workspace():
    need = _lib.load().pea_dot_bpr_train_workspace_bytes(1000)
    assert call_dot(B=1000, ws_bytes=need - 1) == ERR_NOMEM


def test_convs_take_the_fused_switch():
    for cls in (KGATConv, KGCNConv, NGCFConv):
        assert cls(16, 8).fused is False and cls(16, 8, fused=True).fused is True
        assert cls(16, 8, fused=True).update_supported() and not cls(20, 10, fused=True).update_supported()
        assert list(cls(16, 8, fused=True).state_dict().keys()) == list(cls(16, 8).state_dict().keys())


class _DS:
    """two typed relations over 12 nodes, enough to construct the models on the CPU"""
    num_nodes, num_edge_types = 12, 2
    edge_index_nps = {'user2item': torch.tensor([[0, 1, 2, 3], [6, 7, 8, 9]]).numpy(),
                      'ent2item': torch.tensor([[10, 11], [6, 7]]).numpy()}

    def __getitem__(self, key):
        return getattr(self, key)


SHAPES = {
    'kgat': ['x', 'r', 'proj_mat', 'conv1.weight_add', 'conv1.weight_bi', 'conv1.bias', 'conv2.weight_add', 'conv2.weight_bi',
             'conv2.bias', 'conv3.weight_add', 'conv3.weight_bi', 'conv3.bias'],
    'kgcn': ['x', 'r', 'proj_mat', 'conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias'],
    'ngcf': ['x', 'conv1.W_1', 'conv1.W_2', 'conv2.W_1', 'conv2.W_2', 'conv3.W_1', 'conv3.W_2'],
}


@pytest.mark.parametrize('kind', ['kgat', 'kgcn', 'ngcf'])
def test_models_construct_with_native_train(kind):
    ds = _DS()
    if kind == 'ngcf':
        class Model(NGCFRecsysModel):
            def update_graph_input(self, dataset):
                return torch.from_numpy(dataset.edge_index_nps['user2item'])

        extra = dict(entity_aware=False, entity_aware_coff=0.0, if_use_features=False)
    else:
        class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
            def update_graph_input(self, dataset):
                return kg_graph_input(dataset, 'cpu')

        extra = {}
    on = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0.1, native_train=True, **extra)
    off = Model(dataset=ds, emb_dim=16, hidden_size=16, dropout=0.1, **extra)
    assert on.native_train is True and off.native_train is False
    assert list(on.state_dict().keys()) == SHAPES[kind] == list(off.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in on.state_dict().items()} == {k: tuple(v.shape) for k, v in off.state_dict().items()}
    off.load_state_dict(on.state_dict(), strict=True)
