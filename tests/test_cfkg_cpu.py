"""CPU: what the CFKG entry points (include/peahip_kge.h: pea_cfkg_*) decide without a device -- the supported shapes, the
workspace sizes, every argument error (returned before anything is launched, so no GPU is needed to see it) -- that the second
header and _lib.KGE_SIGNATURES agree, and CFKGRecsysModel / kg_negative_sampling on the CPU against the reference-recorded
fixture tests/golden/cfkg_small.npz (tests/make_cfkg_golden.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cfkg_ref
from graph_recsys_benchmark_amd import _lib, engine
from graph_recsys_benchmark_amd.models import CFKGRecsysModel
from graph_recsys_benchmark_amd.utils import kg_negative_sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NOMEM = -1, -4
WIDTHS = {0: 0, 4: 1, 6: 0, 20: 1, 64: 1, 128: 1, 132: 0, -4: 0}
RELS = {0: 0, 1: 1, 64: 1, 65: 0}

_keep = []


def fake(nbytes=4096, misalign=0):
    """A 16-byte aligned host address (+ misalign) that stands in for a device pointer: the calls below fail validation
    before they would read through it."""
    buf = C.create_string_buffer(nbytes + 32)
    _keep.append(buf)
    return C.c_void_p(((C.addressof(buf) + 15) & ~15) + misalign)


def test_supported_shapes():
    lib = _lib.load()
    for emb, w_ok in WIDTHS.items():
        for rel, r_ok in RELS.items():
            assert lib.pea_cfkg_supported(emb, rel) == (w_ok and r_ok), (emb, rel)
    assert _lib.CFKG_MAX_REL == 64


def test_batch_bound():
    assert engine.cfkg_supported(64, 9, 5461) and not engine.cfkg_supported(64, 9, 5462)
    assert not engine.cfkg_supported(6, 9, 64) and not engine.cfkg_supported(64, 65, 64)


def test_workspace_is_nonzero_exactly_where_supported():
    lib = _lib.load()
    for emb, w_ok in WIDTHS.items():
        for rel, r_ok in RELS.items():
            for b in (0, 1, 1000, 5461):
                assert (lib.pea_cfkg_train_workspace_bytes(b, emb, rel) > 0) == bool(w_ok and r_ok), (b, emb, rel)
    assert lib.pea_cfkg_train_workspace_bytes(-1, 64, 9) == 0
    sizes = [lib.pea_cfkg_train_workspace_bytes(b, 64, 9) for b in (0, 1, 16, 17, 1000, 4096, 5461)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]      # one [R, E] partial per workgroup: more quadruples never need less


def call(**over):
    a = dict(B=100, emb=16, x=fake(), ldx=16, num_nodes=50, r=fake(), ldr=16, num_rel=3, quads=fake(), quad_stride=4,
             loss=fake(), pos=fake(), neg=fake(), grad_rows=fake(), grad_r=fake(), ws=fake(), ws_bytes=1 << 40, stream=None)
    a.update(over)
    return _lib.load().pea_cfkg_train(a['B'], a['emb'], a['x'], a['ldx'], a['num_nodes'], a['r'], a['ldr'], a['num_rel'], a['quads'],
                                      a['quad_stride'], a['loss'], a['pos'], a['neg'], a['grad_rows'], a['grad_r'], a['ws'],
                                      a['ws_bytes'], a['stream'])


def case_id(over):
    """repr of the overrides with a stand-in pointer shown as 'ptr': its address differs from process to process, and a
    test id must not"""
    return repr({k: 'ptr' if isinstance(v, C.c_void_p) else v for k, v in over.items()})


BAD = [dict(x=None), dict(r=None), dict(x=fake(misalign=4)), dict(r=fake(misalign=8)), dict(grad_rows=fake(misalign=4)),
       dict(grad_r=fake(misalign=8)), dict(quad_stride=3), dict(ldx=12), dict(ldx=18), dict(ldr=12), dict(ldr=18),
       dict(num_rel=0), dict(num_rel=65), dict(num_nodes=0), dict(pos=None), dict(neg=None), dict(grad_rows=None),
       dict(grad_r=None), dict(emb=6), dict(emb=132), dict(emb=0), dict(B=-1), dict(quads=None), dict(loss=None), dict(ws=None)]


@pytest.mark.parametrize('over', BAD, ids=[case_id(o) + ('#%d' % i) for i, o in enumerate(BAD)])
def test_argument_errors_need_no_device(over):
    assert call(**over) == ERR_ARG
    assert _lib.last_error()


@pytest.mark.parametrize('grads', [True, False])
def test_short_workspace(grads):
    need = _lib.load().pea_cfkg_train_workspace_bytes(100, 16, 3)
    none = {} if grads else dict(grad_rows=None, grad_r=None)
    assert call(ws_bytes=need - 1, **none) == ERR_NOMEM


# ---------------------------------------------------------------- the second header (the parsing helpers of test_cabi.py, restated)
C_WIDTH = {'void': 'void', 'int': 'int', 'int64_t': 'int64', 'size_t': 'uint64', 'uint64_t': 'uint64', 'uint32_t': 'uint32',
           'float': 'float', 'double': 'double'}


def c_width(decl, is_param):
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w not in ('const', 'struct')]
    if is_param and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    return C_WIDTH.get(' '.join(words), 'unknown C type: %s' % decl.strip())


def ctypes_width(t):
    if t is None:
        return 'void'
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return 'pointer'
    table = {C.c_int: 'int', C.c_int64: 'int64', C.c_size_t: 'uint64', C.c_uint64: 'uint64', C.c_uint32: 'uint32',
             C.c_float: 'float', C.c_double: 'double'}
    return table.get(t, 'unknown ctypes type: %r' % t)


def prototypes(header):
    """{name: (return class, [parameter classes])} of every prototype of include/<header>"""
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    protos = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w \*]*?)\b(pea_[a-z_0-9]+)\s*\(([^)]*)\)\s*;', text):
        params = [p for p in params.split(',') if p.strip() and p.strip() != 'void']
        assert name not in protos, 'declared twice: %s' % name
        protos[name] = (c_width(ret, False), [c_width(p, True) for p in params])
    return protos


def test_second_header_matches_its_ctypes_table():
    protos = prototypes('peahip_kge.h')
    assert sorted(protos) == sorted(_lib.KGE_SIGNATURES) == ['pea_cfkg_supported', 'pea_cfkg_train', 'pea_cfkg_train_workspace_bytes']
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.KGE_SIGNATURES[name]
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    first = prototypes('peahip.h')
    assert not set(first) & set(protos) and not set(_lib.SIGNATURES) & set(_lib.KGE_SIGNATURES)
    text = open(os.path.join(ROOT, 'include', 'peahip_kge.h')).read()
    assert re.search(r'#define\s+PEA_CFKG_MAX_REL\s+64\b', text)


# ---------------------------------------------------------------- the model on the CPU against the fixture
@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'cfkg_small.npz'))


def build(z, native=True, device='cpu'):
    inp = cfkg_ref.golden_inputs(z)
    ds = cfkg_ref.model_dataset(inp['num_nodes'], inp['num_uids'], inp['acc_uids'], z['sd.r'].shape[0], inp['rating_r_idx'])
    model = CFKGRecsysModel(dataset=ds, emb_dim=z['sd.x'].shape[1], native=native)
    return cfkg_ref.load_model(model, z['sd.x'], z['sd.r']).to(device), inp


def test_state_dict_and_predictions(golden):
    model, inp = build(golden)
    assert list(model.state_dict().keys()) == ['x', 'r']
    assert model.rating_r_idx == int(golden['rating_r_idx']) and model.scorer == 'dot' and model.native is True
    model.train()
    with torch.no_grad():
        np.testing.assert_allclose(model(inp['unids'], inp['inids']).numpy(), golden['pred'], rtol=1e-6)
        np.testing.assert_allclose(model.predict(inp['unids'], inp['inids']).numpy(), golden['pred'], rtol=1e-6)
    with pytest.raises(NotImplementedError):
        model.shard(0, 2)


def test_kg_loss_and_gradients(golden):
    out = {}
    for native in (True, False):
        model, inp = build(golden, native)
        model.train()
        loss = model.kg_loss(inp['batch'])
        loss.backward()
        out[native] = (loss.detach(), model.x.grad, model.r.grad)
    for a, b in zip(out[True], out[False]):
        assert torch.equal(a, b)
    loss, dx, dr = out[True]
    for want_loss, want_x, want_r in ((golden['loss'], golden['grad.x'], golden['grad.r']),
                                      (golden['f64.loss'], golden['f64.x'], golden['f64.r'])):
        np.testing.assert_allclose(loss.numpy(), want_loss, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(dx.numpy(), want_x, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(dr.numpy(), want_r, rtol=1e-5, atol=1e-6)
    # eval mode computes the same loss
    model, inp = build(golden)
    model.eval()
    assert torch.equal(model.kg_loss(inp['batch']).detach(), loss)


def test_loss_is_the_bce_composition(golden):
    model, inp = build(golden)
    pairs = torch.stack([inp['unids'], inp['inids'], (torch.arange(len(inp['unids'])) % 2)], dim=1)
    model.train()
    want = torch.nn.BCEWithLogitsLoss()(torch.from_numpy(golden['pred']), pairs[:, -1].float())
    np.testing.assert_allclose(model.loss(pairs).detach().numpy(), want.numpy(), rtol=1e-6)


def test_eval_table_in_torch(golden):
    model, inp = build(golden)
    model.eval()
    t = model.cached_repr
    assert t.shape == model.x.shape and not t.requires_grad
    u0, nu = int(golden['acc_uids']), int(golden['num_uids'])
    assert torch.equal(t[u0 + nu:], model.x.detach()[u0 + nu:]) and torch.equal(t[u0:u0 + nu], model.x.detach()[u0:u0 + nu] + model.r.detach()[model.rating_r_idx])
    with torch.no_grad():
        dots = torch.exp(torch.sum(t[inp['unids']] * t[inp['inids']], dim=-1))
        np.testing.assert_allclose(dots.numpy(), model(inp['unids'], inp['inids']).numpy(), rtol=1e-6)
        np.testing.assert_allclose(model.predict(inp['unids'], inp['inids']).numpy(), golden['pred'], rtol=1e-6)


def test_rank_eval_on_the_cpu_agrees_with_a_direct_sort(golden):
    model, inp = build(golden)
    with pytest.raises(RuntimeError):
        model.rank_eval(inp['unids'][:4], inp['inids'][:4].view(4, 1))
    model.eval()
    i0, ni = int(golden['acc_iids']), int(golden['num_iids'])
    g = torch.Generator().manual_seed(3)
    unids = inp['unids'][:12]
    cand = i0 + torch.stack([torch.randperm(ni, generator=g)[:25] for _ in range(12)])      # distinct items per row
    pred, rank, auc, loss = model.rank_eval(unids, cand)
    with torch.no_grad():
        want = model(unids.repeat_interleave(25), cand.reshape(-1)).view(12, 25)
    np.testing.assert_allclose(pred.numpy(), want.numpy(), rtol=1e-6)
    order = torch.argsort(want, dim=1, descending=True)
    want_rank = (order == 0).nonzero()[:, 1]                     # position of column 0 in the sorted row
    assert torch.equal(rank.long(), want_rank)
    np.testing.assert_allclose(auc.numpy(), 1.0 - want_rank.numpy() / 24.0, rtol=1e-6)
    label = torch.zeros_like(want)
    label[:, 0] = 1.0
    want_loss = torch.stack([torch.nn.BCEWithLogitsLoss()(want[k], label[k]) for k in range(12)])
    np.testing.assert_allclose(loss.numpy(), want_loss.numpy(), rtol=1e-6)


def test_kg_negative_sampling(golden):
    import random
    names = [str(n) for n in golden['kg.relations']]
    ds = cfkg_ref.FakeDataset(int(golden['kg.num_nodes']), 1, 0, {n: golden['kg.edge.' + n] for n in names})
    seed = int(golden['kg.seed'])
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    out = kg_negative_sampling(ds)
    n_edges = sum(golden['kg.edge.' + n].shape[1] for n in names)
    assert out is ds.train_data and out.dtype == torch.int64 and tuple(out.shape) == (n_edges, 4)
    assert ds.train_data_length == n_edges == int(golden['kg.train_data_length'])
    assert np.array_equal(cfkg_ref.sorted_rows(out.numpy()), golden['kg.train_data_sorted'])
    # the same relations without the dict: typed by their position, as the reference's dataset types them
    del ds.edge_type_dict
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    assert torch.equal(kg_negative_sampling(ds), out)
