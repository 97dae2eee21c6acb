"""Micro-benchmark of the KG attention maps and the edge softmax (csrc/kg_attention.hip) on the ml25m_shaped KG.

    timeout -k 10 600 python profiles/kg_attention.py [--preset ml25m_shaped] [--emb 64] [--repeats 20] [--hip-only]

Prints one JSON line: ms per fused KGAT map, KGCN map and generic softmax (HIP events around each call, warm-up first,
median of the repeats), the same maps through the reference's torch composition on the same GPU
(experiments/kgat_solver_bpr.py:313-320, kgcn_solver_bpr.py:313-319, the softmax restated as scatter_reduce('amax') +
index_add_), the gathered bytes per second of the byte model below, and the largest relative error against float64 on
sampled destination rows (the 20 largest hubs + 300 random rows).  --hip-only skips the torch composition and the error
check (the kernel-trace run: rocprofv3 --kernel-trace --stats -- python profiles/kg_attention.py --hip-only).

Byte model per edge (fp32): KGAT gathers the source row xp[j] (4 emb B) and reads eid, col and the type (12 B) and writes
one value (4 B); KGCN reads eid and the type and writes one value (r is a table of a few rows, served on chip); the
softmax reads eid, the score through it and writes one value.  Per node: the destination row once (4 emb B), and for
KGAT x read + xp written by the projection (8 emb B).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def torch_softmax(alpha, index, n):
    m = torch.full((n,), float('-inf'), device=alpha.device).scatter_reduce(0, index, alpha, 'amax', include_self=True)
    out = (alpha - m[index]).exp()
    return out / (torch.zeros(n, device=alpha.device).index_add_(0, index, out)[index] + 1e-16)


def torch_map(mode, x, proj, r, ei, ea, n):
    """The reference's att_map block, verbatim but for the softmax (restated above)."""
    signs = torch.sign(ea[:, 0])
    signs[signs == 0] = 1
    trans_vec = r[torch.abs(ea[:, 0])] * signs.view(-1, 1)
    if mode == 'kgat':
        alpha = torch.mm(x[ei[1]], proj) * torch.tanh(torch.mm(x[ei[0]], proj) + trans_vec)
        alpha = alpha.sum(-1)
    else:
        alpha = torch.sum(x[ei[1]] * trans_vec, dim=-1)
    return torch_softmax(alpha, ei[1], n)


def f64_rows_error(mode, got, x, proj, r, ei, ea, n):
    from oracle.pyg_restatement import segment_softmax
    deg = torch.bincount(ei[1], minlength=n)
    g = torch.Generator(device='cuda').manual_seed(3)
    nz = torch.nonzero(deg > 0).view(-1)
    rows = torch.cat([deg.topk(20).indices, nz[torch.randint(0, nz.numel(), (300,), device='cuda', generator=g)]]).unique()
    sel = torch.isin(ei[1], rows)
    e, t = ei[:, sel], ea[sel, 0]
    s = torch.sign(t).double()
    s[s == 0] = 1
    trans = r.double()[t.abs()] * s.view(-1, 1)
    if mode == 'kgat':
        xp = x.double() @ proj.double()
        alpha = (xp[e[1]] * torch.tanh(xp[e[0]] + trans)).sum(-1)
    else:
        alpha = (x.double()[e[1]] * trans).sum(-1)
    want = segment_softmax(alpha, e[1], n)
    return float(((got[sel].double() - want).abs() / want.abs()).max()), int(sel.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--torch-repeats', type=int, default=3)
    ap.add_argument('--hip-only', action='store_true')
    a = ap.parse_args()
    from graph_recsys_benchmark_amd.nn import kgat_attention_map, kgcn_attention_map, softmax
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, kg_graph_input
    torch.cuda.set_device(0)
    d = SyntheticHIN(a.preset)
    ei, ea = kg_graph_input(d, 'cuda')
    n, E, emb = d.num_nodes, int(ei.shape[1]), a.emb
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, emb, generator=g) * 0.3).cuda()
    proj = (torch.randn(emb, emb, generator=g) / emb ** 0.5).cuda()
    r = (torch.randn(len(d.edge_index_nps), emb, generator=g) * 0.3).cuda()
    scores = (torch.randn(E, generator=g) * 3).cuda()
    dst = ei[1]                               # one tensor object: the softmax plan is cached per index tensor
    res = {'preset': a.preset, 'edges': E, 'nodes': n, 'emb': emb, 'timing': 'HIP events, median of %d after %d warm-up'
           % (a.repeats, a.warmup)}
    runs = {'kgat': lambda: kgat_attention_map(x, proj, r, ei, ea, n), 'kgcn': lambda: kgcn_attention_map(x, r, ei, ea, n),
            'softmax': lambda: softmax(scores, dst, n)}
    # bytes of the model in the docstring
    node_b = {'kgat': 12.0 * emb * n, 'kgcn': 4.0 * emb * n, 'softmax': 0.0}
    edge_b = {'kgat': 4.0 * emb + 16.0, 'kgcn': 12.0, 'softmax': 12.0}
    gather_b = {'kgat': 4.0 * emb, 'kgcn': 0.0, 'softmax': 4.0}
    out = {}
    for k, fn in runs.items():
        out[k] = fn()                         # plan + slot-order types are built here (cached afterwards)
        ms = timed(fn, a.warmup, a.repeats)
        res['hip_%s_ms' % k] = round(ms, 4)
        res['hip_%s_model_GB' % k] = round((node_b[k] + edge_b[k] * E) / 1e9, 3)
        res['hip_%s_model_TBps' % k] = round((node_b[k] + edge_b[k] * E) / ms / 1e9, 3)
        if gather_b[k]:
            res['hip_%s_gathered_TBps' % k] = round(gather_b[k] * E / ms / 1e9, 3)
    if not a.hip_only:
        for k in ('kgat', 'kgcn'):
            res['%s_max_rel_err_f64' % k], res['f64_checked_edges'] = f64_rows_error(k, out[k], x, proj, r, ei, ea, n)
        del out
        torch.cuda.empty_cache()
        for k in ('kgat', 'kgcn'):
            ms = timed(lambda: torch_map(k, x, proj, r, ei, ea, n), 1, a.torch_repeats)
            res['torch_%s_ms' % k] = round(ms, 3)
            res['speedup_%s' % k] = round(ms / res['hip_%s_ms' % k], 1)
            torch.cuda.empty_cache()
        ms = timed(lambda: torch_softmax(scores, dst, n), 1, a.torch_repeats)
        res['torch_softmax_ms'] = round(ms, 3)
        res['speedup_softmax'] = round(ms / res['hip_softmax_ms'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
