"""Edge softmax and the KGAT / KGCN attention maps (csrc/kg_attention.hip, nn/kg_attention.py) against float64:
oracle.pyg_restatement.segment_softmax (torch_geometric.utils.softmax 1.5.0) and a float64 restatement of the reference's
att_map blocks (experiments/kgat_solver_bpr.py:313-320, kgcn_solver_bpr.py:313-319).

Per edge: |hip - f64| <= 2e-5 |f64| + 1e-9."""
import functools

import pytest
import torch

from oracle.pyg_restatement import segment_softmax

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 1e-9


def _close(got, want, what):
    err = (got.double() - want).abs()
    bound = RTOL * want.abs() + ATOL
    bad = err > bound
    assert not bool(bad.any()), '%s: %d of %d edges off, worst excess %.3g (max rel err %.3g)' % (
        what, int(bad.sum()), bad.numel(), float((err - bound).max()), float((err / want.abs().clamp_min(1e-30)).max()))


def f64_alpha(mode, x, proj, r, ei, ea, chunk=1 << 21, reversed_zero_sign=1.0):
    """The reference's alpha in float64 (chunked over edges).  reversed_zero_sign=-1 gives the 'fixed' sign rule for
    the flipped half's type-0 edges, which the reference does NOT apply."""
    x64, r64 = x.double(), r.double()
    xp = x64 @ proj.double() if mode == 'kgat' else None
    t = ea[:, 0]
    signs = torch.sign(t).double()
    signs[signs == 0] = 1
    if reversed_zero_sign != 1.0:
        half = ei.shape[1] // 2
        flip0 = torch.zeros_like(signs, dtype=torch.bool)
        flip0[half:] = t[half:] == 0
        signs[flip0] = reversed_zero_sign
    out = torch.empty(ei.shape[1], dtype=torch.float64, device=x.device)
    for b in range(0, ei.shape[1], chunk):
        sl = slice(b, b + chunk)
        trans = r64[t[sl].abs()] * signs[sl].view(-1, 1)
        if mode == 'kgat':
            out[sl] = (xp[ei[1, sl]] * torch.tanh(xp[ei[0, sl]] + trans)).sum(-1)
        else:
            out[sl] = (x64[ei[1, sl]] * trans).sum(-1)
    return out


def params(n, n_types, emb, seed, scale):
    g = torch.Generator().manual_seed(seed)
    if scale == 'glorot':      # the reference's initialisation (models/kgat.py: glorot of x, r, proj_mat)
        def glorot(a, b):
            s = (6.0 / (a + b)) ** 0.5
            return (torch.rand(a, b, generator=g) * 2 - 1) * s
        return glorot(n, emb).cuda(), glorot(emb, emb).cuda(), glorot(n_types, emb).cuda()
    return ((torch.randn(n, emb, generator=g) * scale).cuda(), (torch.randn(emb, emb, generator=g) / emb ** 0.5).cuda(),
            (torch.randn(n_types, emb, generator=g) * scale).cuda())


@functools.lru_cache(maxsize=None)
def kg(preset, scale=1.0):
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, kg_graph_input
    d = SyntheticHIN(preset, scale=scale)
    ei, ea = kg_graph_input(d, 'cuda')
    return d.num_nodes, len(d.edge_index_nps), ei, ea


def hip_map(mode, x, proj, r, ei, ea, n):
    from graph_recsys_benchmark_amd.nn import kgat_attention_map, kgcn_attention_map
    return kgat_attention_map(x, proj, r, ei, ea, n) if mode == 'kgat' else kgcn_attention_map(x, r, ei, ea, n)


def check_map(mode, n, n_types, ei, ea, emb=64, seed=0, scale=0.3):
    x, proj, r = params(n, n_types, emb, seed, scale)
    got = hip_map(mode, x, proj, r, ei, ea, n)
    assert got.dtype == torch.float32 and tuple(got.shape) == (ei.shape[1],) and not got.requires_grad
    want = segment_softmax(f64_alpha(mode, x, proj, r, ei, ea), ei[1], n)
    _close(got, want, '%s map' % mode)
    again = hip_map(mode, x, proj, r, ei, ea, n)
    assert torch.equal(got, again), 'two calls differ'
    sums = torch.zeros(n, dtype=torch.float64, device='cuda').index_add_(0, ei[1], got.double())
    has = torch.bincount(ei[1], minlength=n) > 0
    assert float((sums[has] - 1).abs().max()) <= 1e-5
    assert bool((sums[~has] == 0).all())
    return x, proj, r, got, want


# ---------------------------------------------------------------------------------------------- generic softmax
def softmax_case(seed, n_edges, num_nodes, hubs=(), spread=3.0):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, num_nodes, (n_edges,), generator=g)
    idx = idx[idx % 7 != 3]                       # empty segments
    parts = [idx] + [torch.full((k,), h, dtype=torch.int64) for h, k in hubs]
    idx = torch.cat(parts)
    idx = idx[torch.randperm(idx.numel(), generator=g)]   # unsorted
    src = torch.randn(idx.numel(), generator=g) * spread
    return src.cuda(), idx.cuda()


@pytest.mark.parametrize('case', ['small', 'chunked', 'many_chunks'])
@pytest.mark.parametrize('num_nodes_arg', ['none', 'larger'])
def test_softmax_forward_backward_match_float64(case, num_nodes_arg):
    from graph_recsys_benchmark_amd.nn import softmax
    n = 5000
    hubs = {'small': (), 'chunked': ((11, 700), (12, 5000)), 'many_chunks': ((13, 150000), (14, 3000))}[case]
    src, idx = softmax_case(len(case), 40000, n, hubs)
    num_nodes = None if num_nodes_arg == 'none' else int(idx.max()) + 1 + 37
    nn_ = int(idx.max()) + 1 if num_nodes is None else num_nodes
    s = src.clone().requires_grad_(True)
    y = softmax(s, idx, num_nodes)
    s64 = src.double().requires_grad_(True)
    y64 = segment_softmax(s64, idx, nn_)
    _close(y.detach(), y64.detach(), 'softmax')
    assert torch.equal(y.detach(), softmax(src, idx, num_nodes)), 'two calls differ'
    gr = torch.randn(y.numel(), generator=torch.Generator().manual_seed(7)).cuda()
    y.backward(gr)
    y64.backward(gr.double())
    err = (s.grad.double() - s64.grad).abs()
    bound = RTOL * s64.grad.abs() + 1e-6 * y64.detach() * float(gr.abs().max()) + ATOL
    assert bool((err <= bound).all()), float((err - bound).max())


def test_softmax_rejects_bad_input():
    from graph_recsys_benchmark_amd.nn import softmax
    idx = torch.zeros(4, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        softmax(torch.zeros(4, 2, device='cuda'), idx)
    with pytest.raises(ValueError):
        softmax(torch.zeros(5, device='cuda'), idx)
    with pytest.raises(ValueError):
        softmax(torch.zeros(4, device='cuda', dtype=torch.float64), idx)
    with pytest.raises(ValueError):
        softmax(torch.zeros(4), idx.cpu())


# ---------------------------------------------------------------------------------------------- KG maps
@pytest.mark.parametrize('mode', ['kgat', 'kgcn'])
@pytest.mark.parametrize('scale', [0.3, 'glorot'])
def test_kg_map_ml_small(mode, scale):
    n, nt, ei, ea = kg('ml_small')
    x, proj, r, got, _ = check_map(mode, n, nt, ei, ea, scale=scale)
    if scale == 0.3:
        # the flipped user2item half has type 0 and must keep +r[0] (signs[signs == 0] = 1), not -r[0]
        wrong = segment_softmax(f64_alpha(mode, x, proj, r, ei, ea, reversed_zero_sign=-1.0), ei[1], n)
        half = ei.shape[1] // 2
        rev0 = torch.zeros(ei.shape[1], dtype=torch.bool, device='cuda')
        rev0[half:] = ea[half:, 0] == 0
        assert float((got[rev0].double() - wrong[rev0]).abs().max()) > 1e-3


@pytest.mark.parametrize('mode', ['kgat', 'kgcn'])
def test_kg_map_ml25m_reduced(mode):
    n, nt, ei, ea = kg('ml25m_shaped', 0.05)
    assert int(torch.bincount(ei[1], minlength=n).max()) > 4096     # hub rows merged over several chunks
    check_map(mode, n, nt, ei, ea, seed=1)


@pytest.mark.parametrize('emb', [4, 12, 128, 256])
def test_kg_map_other_widths(emb):
    n, nt, ei, ea = kg('ml_small')
    check_map('kgat', n, nt, ei, ea, emb=emb, seed=emb, scale=0.3 * (64.0 / emb) ** 0.5)
    check_map('kgcn', n, nt, ei, ea, emb=emb, seed=emb, scale=0.3 * (64.0 / emb) ** 0.5)


@pytest.mark.parametrize('mode', ['kgat', 'kgcn'])
def test_kg_map_ml25m_full_size_sampled_rows(mode):
    n, nt, ei, ea = kg('ml25m_shaped')
    assert ei.shape[1] > 55_000_000
    x, proj, r = params(n, nt, 64, 5, 0.3)
    got = hip_map(mode, x, proj, r, ei, ea, n)
    again = hip_map(mode, x, proj, r, ei, ea, n)
    assert torch.equal(got, again), 'two calls differ'
    deg = torch.bincount(ei[1], minlength=n)
    g = torch.Generator(device='cuda').manual_seed(3)
    rows = torch.cat([deg.topk(20).indices, torch.nonzero(deg > 0).view(-1)[
        torch.randint(0, int((deg > 0).sum()), (300,), device='cuda', generator=g)]]).unique()
    sel = torch.isin(ei[1], rows)
    want = segment_softmax(f64_alpha(mode, x, proj, r, ei[:, sel], ea[sel]), ei[1, sel], n)
    _close(got[sel], want, '%s map, full size' % mode)
    sums = torch.zeros(n, dtype=torch.float64, device='cuda').index_add_(0, ei[1], got.double())
    assert float((sums[deg > 0] - 1).abs().max()) <= 1e-5


def test_kgat_conv_with_hip_map_matches_float64_map():
    from graph_recsys_benchmark_amd.nn import KGATConv
    n, nt, ei, ea = kg('ml_small')
    x, proj, r, got, want = check_map('kgat', n, nt, ei, ea, seed=2)
    torch.manual_seed(0)
    conv = KGATConv(64, 64).cuda()
    with torch.no_grad():
        a = conv(x, ei, got)
        b = conv(x, ei, want.float())
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


def test_kg_map_errors():
    from graph_recsys_benchmark_amd import _lib
    n, nt, ei, ea = kg('ml_small')
    x, proj, r = params(n, nt, 64, 0, 0.3)
    with pytest.raises(_lib.PeaError):       # r has nt rows: type nt is out of range
        hip_map('kgat', x, proj, r, ei, (ea + nt).clone(), n)
    with pytest.raises(_lib.PeaError):
        hip_map('kgcn', x, proj, r, ei, (ea - nt).clone(), n)
    with pytest.raises(ValueError):          # emb % 4 != 0
        hip_map('kgat', x[:, :62].contiguous(), proj[:62, :62].contiguous(), r[:, :62].contiguous(), ei, ea, n)
    with pytest.raises(ValueError):          # one type per edge
        hip_map('kgcn', x, proj, r, ei, ea[:-1].clone(), n)
    with pytest.raises(ValueError):
        hip_map('kgat', x.cpu(), proj, r, ei, ea, n)
    with pytest.raises(ValueError):
        hip_map('kgcn', x.double(), proj, r, ei, ea, n)
