"""Measurement of the inner-product full-catalogue entry points (csrc/dot_score.hip) at the catalogue of the headline
preset and the table width of the KGAT / KGCN / NGCF models at hidden_size 64 (D = 64 + 32 + 16 = 112).

    timeout -k 10 900 python profiles/recommend_dot.py [--users 162541] [--serving-users 1024] [--items 59047] [--k 20]
                                                       [--d 112] [--repeats 20] [--torch-repeats 5] [--chunk 2048]
                                                       [--hip-only] [--out FILE]

Workloads (unit-scale random table; only the shapes matter for the timing):
  (a) dot_recommend_topk, every user against every item, each user's seen items excluded
  (b) dot_recommend_topk, --serving-users users, same catalogue (the item-range split has to fill the machine)
  (c) dot_rank_full on (a)
Exclusion lists as in profiles/recommend.py (log-normal user degrees scaled to the preset's interactions).

Yardstick: what a user of these models writes from torch today on the same GPU: per chunk of --chunk users
table[u] @ table[items].T, the seen items masked (index_put of -inf; NaN for the rank), torch.topk (for (c): two
comparisons and sums).

Timing: HIP events around each call, warm-up, the two sides alternated call by call in one process, median.  Per-launch
times come from the library's own events (pea_profile_*) in one extra call.  The scan is a GEMM of 2 U items D flop; its
floor is that over the 155 TF of the f32-input MFMA.  One JSON line (also written to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_FLOPS = 155e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fused, composed, warmup, repeats, torch_repeats):
    for _ in range(warmup):
        fused()
    if composed:
        composed()
    torch.cuda.synchronize()
    f, t = [], []
    for r in range(repeats):
        f.append(event_ms(fused))
        if composed and r < torch_repeats:
            t.append(event_ms(composed))
    f.sort()
    t.sort()
    return f[len(f) // 2], (t[len(t) // 2] if t else None), (f[0], f[-1])


def exclusion_lists(n_users, lo, n_items, total, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    deg = torch.exp(torch.randn(n_users, device='cuda', generator=g) * 0.8)
    for _ in range(20):
        deg = torch.clamp(deg * (total / deg.sum()), 11, min(299, n_items))
    deg = deg.floor().long()
    users = torch.repeat_interleave(torch.arange(n_users, device='cuda'), deg)
    items = torch.randint(0, n_items, (users.numel(),), device='cuda', generator=g)
    keys = torch.unique(users * n_items + items)
    ku = torch.div(keys, n_items, rounding_mode='floor')
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device='cuda')
    rowptr[1:] = torch.cumsum(torch.bincount(ku, minlength=n_users), 0)
    return rowptr, keys % n_items + lo


def profile_scopes(fn):
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.pea_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.pea_profile_enable(0)
    cap = 64
    names, ms, units, cnt = C.create_string_buffer(cap * 32), (C.c_float * cap)(), (C.c_double * cap)(), C.c_int()
    lib.pea_profile_read(cap, names, ms, units, C.byref(cnt))
    return {names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode(): round(ms[i], 4) for i in range(cnt.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=162541)
    ap.add_argument('--serving-users', type=int, default=1024)
    ap.add_argument('--items', type=int, default=59047)
    ap.add_argument('--interactions', type=int, default=24800000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--d', type=int, default=112)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--torch-repeats', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd import engine
    torch.cuda.set_device(0)
    nu, ni, D, K = a.users, a.items, a.d, a.k
    lo, n_nodes = nu, nu + ni + 1000
    g = torch.Generator().manual_seed(0)
    table = torch.randn(n_nodes, D, generator=g).cuda()
    rowptr, seen = exclusion_lists(nu, lo, ni, a.interactions, 1)
    users_all = torch.arange(nu, device='cuda')
    users_srv = torch.randperm(nu, generator=g)[:a.serving_users].cuda()
    srv_ptr = torch.zeros(users_srv.numel() + 1, dtype=torch.int64, device='cuda')
    cnt = rowptr[users_srv + 1] - rowptr[users_srv]
    srv_ptr[1:] = torch.cumsum(cnt, 0)
    row = torch.repeat_interleave(torch.arange(users_srv.numel(), device='cuda'), cnt)
    srv_seen = seen[rowptr[users_srv][row] + torch.arange(row.numel(), device='cuda') - srv_ptr[:-1][row]]
    pos = torch.randint(lo, lo + ni, (nu,), generator=torch.Generator(device='cuda').manual_seed(2), device='cuda')
    items_t = table[lo:lo + ni].T.contiguous()

    def composed(users, ptr, items, rank_of=None):
        out = []
        for s in range(0, users.numel(), a.chunk):
            u = users[s:s + a.chunk]
            sc = table[u] @ items_t
            e0, e1 = int(ptr[s]), int(ptr[min(s + a.chunk, users.numel())])
            rows = torch.repeat_interleave(torch.arange(u.numel(), device='cuda'), ptr[s + 1:s + 1 + u.numel()] - ptr[s:s + u.numel()])
            if rank_of is None:
                sc[rows, items[e0:e1] - lo] = float('-inf')
                out.append(torch.topk(sc, K, dim=1))
            else:
                p = sc.gather(1, (rank_of[s:s + a.chunk] - lo)[:, None])
                sc[rows, items[e0:e1] - lo] = float('nan')
                out.append(((sc > p).sum(1), (sc < p).sum(1)))
        return out

    res = {'users': nu, 'serving_users': int(users_srv.numel()), 'items': ni, 'K': K, 'D': D, 'excluded_pairs': int(seen.numel()),
           'chunk_users': a.chunk, 'timing': 'HIP events, alternated, median of %d (torch side: %d) after %d warm-up'
           % (a.repeats, a.torch_repeats, a.warmup)}
    work = {
        'a_topk_all': (lambda: engine.dot_recommend_topk(table, users_all, K, (lo, lo + ni), exclude=(rowptr, seen)),
                       lambda: composed(users_all, rowptr, seen), nu, 'dot_topk_scan'),
        'b_topk_serving': (lambda: engine.dot_recommend_topk(table, users_srv, K, (lo, lo + ni), exclude=(srv_ptr, srv_seen)),
                           lambda: composed(users_srv, srv_ptr, srv_seen), int(users_srv.numel()), 'dot_topk_scan'),
        'c_rank_all': (lambda: engine.dot_rank_full(table, users_all, pos, (lo, lo + ni), exclude=(rowptr, seen)),
                       lambda: composed(users_all, rowptr, seen, rank_of=pos), nu, 'dot_rank_multi_scan'),
    }
    for name, (fused, comp, n_u, scope) in work.items():
        f_ms, t_ms, f_min_max = alternated(fused, None if a.hip_only else comp, a.warmup, a.repeats, a.torch_repeats)
        res[name + '_hip_ms'] = round(f_ms, 4)
        res[name + '_hip_min_max_ms'] = [round(v, 4) for v in f_min_max]
        if t_ms is not None:
            res[name + '_torch_ms'] = round(t_ms, 3)
            res[name + '_speedup'] = round(t_ms / f_ms, 2)
        scopes = profile_scopes(fused)
        res[name + '_launch_ms'] = scopes
        floor_ms = 2.0 * n_u * ni * D / MFMA_F32_FLOPS * 1e3
        res[name + '_scan_floor_ms'] = round(floor_ms, 4)
        if scope in scopes:                     # (a PEA_LIB build may name its launches otherwise)
            res[name + '_scan_share_of_mfma_floor'] = round(floor_ms / scopes[scope], 3)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
