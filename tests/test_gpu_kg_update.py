"""GPU: the fused dense update of the KGAT / KGCN / NGCF convs (csrc/kg_update.hip) against torch.

Exact cases: integer-valued x, s in [-2, 2], weights in {-1, 0, 1}, bias and g_out in [-2, 2], keep_scale = 2 and
negative_slope = 0.5 make every product and partial sum exactly representable (largest |dW| entry at N = 40,001 is below
2^24), so float32 in any order equals float64: out, dx, ds, dw1, dw2, dbias must be torch.equal to the float64 autograd
result.  Many pre-activations are exactly 0 there, which pins the mask rule (z == 0 takes the slope; 0 for the relu).
Random-float cases go through helpers.assert_fp32_close with today's unfused float32 composition as the peer.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
from graph_recsys_benchmark_amd import _lib
from graph_recsys_benchmark_amd.nn import KGATConv, KGCNConv, NGCFConv, kg_update
from graph_recsys_benchmark_amd.utils.graph_input import kg_graph_input
from test_gpu_dot_models import TinyKG

pytestmark = pytest.mark.gpu

DEV = 'cuda'
KINDS = ['kgat', 'kgcn', 'ngcf']
KIND_ID = {'kgat': _lib.KGU_KGAT, 'kgcn': _lib.KGU_KGCN, 'ngcf': _lib.KGU_NGCF}
WIDTHS = [(4, 4), (8, 4), (16, 8), (12, 20), (64, 64), (64, 32), (32, 16), (128, 128)]
ROWS = [1, 15, 16, 17, 63, 64, 65, 300, 40001]
SENTINEL = 777.0


def compose(kind, x, s, w1, w2, bias, slope, keep, scale, merged=True):
    """The conv's dense update in torch, any dtype.  merged=False: NGCF as nn/kg_conv.py writes it (three products)."""
    a1, a2 = x + s, x * s
    if kind == 'kgat':
        y = F.leaky_relu(a1 @ w1, slope) + F.leaky_relu(a2 @ w2, slope)
        if bias is not None:
            y = y + bias
    elif kind == 'kgcn':
        y = torch.relu(a1 @ w1 + bias) if bias is not None else torch.relu(a1 @ w1)
    elif merged:
        y = F.leaky_relu(a1 @ w1 + a2 @ w2, slope)
    else:
        y = F.leaky_relu(x @ w1 + s @ w1 + a2 @ w2, slope)
    if keep is not None:
        y = y * keep.to(y.dtype) * scale
    return y


def torch_side(kind, t, dtype, merged=True):
    """(out, dx, ds, dw1, dw2, dbias) of compose under autograd in `dtype`."""
    leaf = {k: (None if t[k] is None else t[k].detach().to(dtype).clone().requires_grad_(True)) for k in ('x', 's', 'w1', 'w2', 'bias')}
    out = compose(kind, leaf['x'], leaf['s'], leaf['w1'], leaf['w2'], leaf['bias'], t['slope'], t['keep'], t['scale'], merged)
    out.backward(t['g'].to(dtype))
    return (out.detach(),) + tuple(None if leaf[k] is None else leaf[k].grad for k in ('x', 's', 'w1', 'w2', 'bias'))


def make(kind, n, fin, fout, seed, exact, with_keep=True, with_bias=True, device=DEV):
    g = torch.Generator().manual_seed(seed)
    if exact:
        draw = lambda *shape: torch.randint(-2, 3, shape, generator=g).float()
        weight = lambda: torch.randint(-1, 2, (fin, fout), generator=g).float()
        slope, scale = 0.5, 2.0
    else:
        draw = lambda *shape: torch.randn(shape, generator=g)
        bound = (6.0 / (fin + fout)) ** 0.5
        weight = lambda: (torch.rand((fin, fout), generator=g) * 2 - 1) * bound
        slope, scale = 0.2, 1.0 / 0.9
    t = {'x': draw(n, fin), 's': draw(n, fin), 'w1': weight(), 'w2': None if kind == 'kgcn' else weight(),
         'bias': draw(fout) if kind != 'ngcf' and with_bias else None, 'g': draw(n, fout), 'slope': slope, 'scale': scale,
         'keep': (torch.rand((n, fout), generator=g) >= (0.5 if exact else 0.1)).to(torch.uint8) if with_keep else None}
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in t.items()}


def block(t, pad):
    """t as a column block (at column 4) of a buffer `pad` columns wider, filled with a sentinel elsewhere."""
    if not pad:
        return t.clone(), None
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENTINEL, device=DEV)
    buf[:, 4:4 + t.shape[1]] = t
    return buf[:, 4:4 + t.shape[1]], buf


def raw(kind, t, pad=0):
    """The two C entry points called directly: (out, dx, ds, dw1, dw2, dbias) and the wide buffers behind out / dx / ds."""
    lib = _lib.require_device()
    n, fin = t['x'].shape
    fout = t['w1'].shape[1]
    p = _lib.ptr
    x, _ = block(t['x'], pad)
    s, _ = block(t['s'], pad)
    g, _ = block(t['g'], pad)
    out, out_buf = block(torch.zeros((n, fout), device=DEV), pad)
    dx, dx_buf = block(torch.zeros((n, fin), device=DEV), pad)
    ds, ds_buf = block(torch.zeros((n, fin), device=DEV), pad)
    dw1 = torch.full((fin, fout), SENTINEL, device=DEV)
    dw2 = None if t['w2'] is None else torch.full((fin, fout), SENTINEL, device=DEV)
    dbias = None if t['bias'] is None else torch.full((fout,), SENTINEL, device=DEV)
    kid = KIND_ID[kind]
    _lib.check(lib.pea_kg_update_forward(n, kid, fin, fout, p(x), x.stride(0), p(s), s.stride(0), p(t['w1']), p(t['w2']), p(t['bias']),
                                         t['slope'], p(t['keep']), t['scale'], p(out), out.stride(0), _lib.current_stream()))
    nbytes = int(lib.pea_kg_update_backward_workspace_bytes(kid, fin, fout))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.pea_kg_update_backward(n, kid, fin, fout, p(x), x.stride(0), p(s), s.stride(0), p(t['w1']), p(t['w2']), p(t['bias']),
                                          t['slope'], p(t['keep']), t['scale'], p(g), g.stride(0), p(dx), dx.stride(0), p(ds),
                                          ds.stride(0), p(dw1), p(dw2), p(dbias), p(ws), nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    return (out, dx, ds, dw1, dw2, dbias), (out_buf, dx_buf, ds_buf)


NAMES = ('out', 'dx', 'ds', 'dw1', 'dw2', 'dbias')


def assert_exact(kind, t, got):
    want = torch_side(kind, t, torch.float64)
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a.double(), b), '%s %s: %d of %d elements differ, max |diff| %g' % (
                kind, name, int((a.double() != b).sum()), a.numel(), float((a.double() - b).abs().max()))
    return want


EXACT = [(n, 64, 64) for n in ROWS] + [(n, fin, fout) for fin, fout in WIDTHS if (fin, fout) != (64, 64) for n in (17, 300)]


def exact_inputs(kind, n, fin, fout, device=DEV):
    # the keep mask is present in every second case, so both pointer states meet every kind and both tile paths
    return make(kind, n, fin, fout, seed=n + fin + 3 * fout, exact=True, with_keep=(n + fin // 4) % 2 == 0, device=device)


def check_exact(kind, n, fin, fout):
    t = exact_inputs(kind, n, fin, fout)
    got, _ = raw(kind, t)
    want = assert_exact(kind, t, got)
    if n >= 300 and kind == 'kgat':      # the run does land on z == 0 with a non-zero gradient behind it
        z = (t['x'] + t['s']).double() @ t['w1'].double()
        assert int((z == 0).sum()) > 0 and float(want[1].abs().max()) > 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,fin,fout', EXACT)
def test_exact(kind, n, fin, fout):
    check_exact(kind, n, fin, fout)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('with_keep', [False, True])
def test_exact_both_keep_states_at_the_reference_shape(kind, with_keep):
    t = make(kind, 300, 64, 64, seed=5, exact=True, with_keep=with_keep)
    assert_exact(kind, t, raw(kind, t)[0])


def test_exact_kgat_without_bias():
    t = make('kgat', 300, 64, 32, seed=9, exact=True, with_bias=False)
    got, _ = raw('kgat', t)
    assert got[5] is None
    assert_exact('kgat', t, got)


def check_column_blocks(kind, t):
    fin, fout = t['w1'].shape
    got, bufs = raw(kind, t, pad=12)
    assert_exact(kind, t, got)
    for buf, width in zip(bufs, (fout, fin, fin)):
        outside = torch.cat([buf[:, :4], buf[:, 4 + width:]], dim=1)
        assert bool((outside == SENTINEL).all()), 'columns outside the block were written'


@pytest.mark.parametrize('kind', KINDS)
def test_exact_column_blocks_of_wider_buffers(kind):
    check_column_blocks(kind, make(kind, 65, 12, 20, seed=2, exact=True))


RANDOM_FLOAT = [(300, 64, 64), (1000, 64, 64), (300, 64, 32), (1000, 32, 16), (300, 128, 128), (300, 12, 20)]


def check_random_float(kind, n, fin, fout):
    t = make(kind, n, fin, fout, seed=n + fout, exact=False)
    got, _ = raw(kind, t)
    want = torch_side(kind, t, torch.float32, merged=False)
    truth = torch_side(kind, t, torch.float64)
    for name, a, b, c in zip(NAMES, got, want, truth):
        if a is not None:
            helpers.assert_fp32_close(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy(), what='%s %s' % (kind, name))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,fin,fout', RANDOM_FLOAT)
def test_random_float(kind, n, fin, fout):
    check_random_float(kind, n, fin, fout)


@pytest.mark.parametrize('kind', KINDS)
def test_backward_is_bitwise_reproducible(kind):
    t = make(kind, 40001, 64, 64, seed=1, exact=False)
    first, _ = raw(kind, t)
    second, _ = raw(kind, t)
    for name, a, b in zip(NAMES, first, second):
        if a is not None:
            assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------ autograd wiring
@pytest.fixture(scope='module')
def graph():
    ds = TinyKG()
    edge_index, _ = kg_graph_input(ds, DEV)
    g = torch.Generator().manual_seed(8)
    att = torch.rand(edge_index.shape[1], generator=g).to(DEV)
    u2i = torch.from_numpy(ds.edge_index_nps['user2item']).to(DEV)
    return {'n': ds.num_nodes, 'kg': edge_index, 'att': att,
            'cf': torch.cat([u2i, torch.flip(u2i, dims=[0])], dim=1).contiguous()}


def conv_f64(kind, p, x, edge_index, att, dtype):
    """The conv restated in torch (dtype float64 = truth)."""
    src, dst = edge_index[0], edge_index[1]
    if kind == 'ngcf':
        deg = torch.bincount(edge_index.reshape(-1), minlength=x.shape[0]).to(dtype) / 2
        att = 1 / torch.sqrt(deg[dst] * deg[src])
    aggr = torch.zeros_like(x).index_add_(0, dst, x[src] * att.to(dtype)[:, None])
    if kind == 'kgat':
        return F.leaky_relu((x + aggr) @ p['weight_add'], 0.2) + F.leaky_relu((x * aggr) @ p['weight_bi'], 0.2) + p['bias']
    if kind == 'kgcn':
        return torch.relu((aggr + x) @ p['weight'] + p['bias'])
    return F.leaky_relu(x @ p['W_1'] + aggr @ p['W_1'] + (x * aggr) @ p['W_2'], 0.2)


@pytest.mark.parametrize('kind', KINDS)
def test_fused_conv_matches_unfused_under_autograd(graph, kind):
    cls = {'kgat': KGATConv, 'kgcn': KGCNConv, 'ngcf': NGCFConv}[kind]
    torch.manual_seed(4)
    plain, fused = cls(16, 8).to(DEV), cls(16, 8, fused=True).to(DEV)
    with torch.no_grad():
        for prm in plain.parameters():
            if prm.dim() == 1:
                prm.normal_(0.0, 0.1)
    fused.load_state_dict(plain.state_dict())
    edge_index = graph['cf'] if kind == 'ngcf' else graph['kg']
    args = () if kind == 'ngcf' else (graph['att'],)
    x0 = torch.randn((graph['n'], 16), generator=torch.Generator().manual_seed(6)).to(DEV)
    gout = torch.randn((graph['n'], 8), generator=torch.Generator().manual_seed(7)).to(DEV)

    def run(conv):
        x = x0.clone().requires_grad_(True)
        conv.zero_grad()
        out = conv(x, edge_index, *args)
        out.backward(gout)
        return [out.detach(), x.grad] + [prm.grad for prm in conv.parameters()]

    x64 = x0.double().requires_grad_(True)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in plain.state_dict().items()}
    out64 = conv_f64(kind, p64, x64, edge_index, None if kind == 'ngcf' else graph['att'], torch.float64)
    out64.backward(gout.double())
    truth = [out64.detach(), x64.grad] + [p64[k].grad for k, _ in plain.named_parameters()]
    names = ['out', 'dx'] + [k for k, _ in plain.named_parameters()]
    for name, a, b, c in zip(names, run(fused), run(plain), truth):
        helpers.assert_fp32_close(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy(), what='%s conv %s' % (kind, name))


def test_kg_update_function_refuses_unsupported_widths():
    x = torch.zeros((8, 20), device=DEV)
    with pytest.raises(_lib.PeaError):
        kg_update('kgcn', x, x, torch.zeros((20, 10), device=DEV), None, torch.zeros(10, device=DEV))
