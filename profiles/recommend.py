"""Measurement of the full-catalogue entry points (csrc/topk.hip) at the catalogue of the headline preset.

    timeout -k 10 900 python profiles/recommend.py [--users 162541] [--serving-users 1024] [--items 59047] [--k 20]
                                                   [--repeats 20] [--torch-repeats 5] [--chunk 2048] [--hip-only]

Workloads (R = 16, unit-scale random tables; only the shapes matter for the timing):
  (a) recommend_topk, every user against every item, each user's seen items excluded
  (b) recommend_topk, --serving-users users, same catalogue (the item-range split has to fill the machine)
  (c) rank_full on (a)
Exclusion lists: user degrees log-normal (sigma 0.8) clipped to [11, 299] and scaled to the preset's 24.8 M interactions
(utils/synthetic.py: the ml25m_shaped user->item relation), items uniform over the catalogue and distinct per user -- drawn
on the device in a second instead of building the preset's graph.

Yardstick: nothing in the reference scores a whole catalogue, so the other side is what a user would write from torch on
the same GPU: per chunk of --chunk users  relu(A[:, None, :] + B[None, :, :]) @ fc2_w + fc2_b  (A, B hoisted exactly as the
kernel does), the seen items masked (index_put of -inf; NaN for the rank), torch.topk (for (c): two comparisons and sums).
At the default chunk the [chunk, items, R] intermediate is 7.7 GB.

Timing: HIP events around each call, warm-up, the two sides alternated call by call in one process, median.  The scan
kernel's own time comes from the library's per-launch events (pea_profile_*) in one extra call; lane-operations are
3 R per pair (add, max, fma), and the vector-rate floor is 1024 SIMDs x 32 lanes x 2.4 GHz.  --hip-only skips the torch side
(the kernel-trace run: rocprofv3 --kernel-trace --stats -- python profiles/recommend.py --hip-only).  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_RATE = 1024 * 32 * 2.4e9


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
    ap.add_argument('--r', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--torch-repeats', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--hip-only', action='store_true')
    a = ap.parse_args()
    from graph_recsys_benchmark_amd import engine
    torch.cuda.set_device(0)
    nu, ni, R, K = a.users, a.items, a.r, a.k
    lo, n_nodes = nu, nu + ni + 1000
    g = torch.Generator().manual_seed(0)
    table = torch.randn(n_nodes, R, generator=g).cuda()
    torch.manual_seed(0)
    fc1, fc2 = torch.nn.Linear(2 * R, R).cuda(), torch.nn.Linear(R, 1).cuda()
    w = tuple(t.detach() for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))
    rowptr, seen = exclusion_lists(nu, lo, ni, a.interactions, 1)
    users_all = torch.arange(nu, device='cuda')
    users_srv = torch.randperm(nu, generator=g)[:a.serving_users].cuda()
    srv_ptr = torch.zeros(users_srv.numel() + 1, dtype=torch.int64, device='cuda')
    cnt = rowptr[users_srv + 1] - rowptr[users_srv]
    srv_ptr[1:] = torch.cumsum(cnt, 0)
    row = torch.repeat_interleave(torch.arange(users_srv.numel(), device='cuda'), cnt)
    srv_seen = seen[rowptr[users_srv][row] + torch.arange(row.numel(), device='cuda') - srv_ptr[:-1][row]]
    pos = torch.randint(lo, lo + ni, (nu,), generator=torch.Generator(device='cuda').manual_seed(2), device='cuda')

    A_all = table[:nu] @ w[0][:, :R].T + w[1]
    B = table[lo:lo + ni] @ w[0][:, R:].T
    w2, b2 = w[2].reshape(-1), w[3].reshape(())

    def composed(users, ptr, items, rank_of=None, fill=float('-inf')):
        out = []
        for s in range(0, users.numel(), a.chunk):
            u = users[s:s + a.chunk]
            sc = torch.relu(A_all[u][:, None, :] + B[None, :, :]) @ w2 + b2
            e0, e1 = int(ptr[s]), int(ptr[min(s + a.chunk, users.numel())])
            rows = torch.repeat_interleave(torch.arange(u.numel(), device='cuda'), ptr[s + 1:s + 1 + u.numel()] - ptr[s:s + u.numel()])
            if rank_of is None:
                sc[rows, items[e0:e1] - lo] = fill
                out.append(torch.topk(sc, K, dim=1))
            else:
                p = sc.gather(1, (rank_of[s:s + a.chunk] - lo)[:, None])
                sc[rows, items[e0:e1] - lo] = float('nan')
                out.append(((sc > p).sum(1), (sc < p).sum(1)))
        return out

    res = {'users': nu, 'serving_users': int(users_srv.numel()), 'items': ni, 'K': K, 'R': R, 'excluded_pairs': int(seen.numel()),
           'chunk_users': a.chunk, 'timing': 'HIP events, alternated, median of %d (torch side: %d) after %d warm-up'
           % (a.repeats, a.torch_repeats, a.warmup)}
    work = {
        'a_topk_all': (lambda: engine.recommend_topk(table, users_all, K, (lo, lo + ni), *w, exclude=(rowptr, seen)),
                       lambda: composed(users_all, rowptr, seen), nu, 'topk_scan'),
        'b_topk_serving': (lambda: engine.recommend_topk(table, users_srv, K, (lo, lo + ni), *w, exclude=(srv_ptr, srv_seen)),
                           lambda: composed(users_srv, srv_ptr, srv_seen), int(users_srv.numel()), 'topk_scan'),
        'c_rank_all': (lambda: engine.rank_full(table, users_all, pos, (lo, lo + ni), *w, exclude=(rowptr, seen)),
                       lambda: composed(users_all, rowptr, seen, rank_of=pos), nu, 'rank_multi_scan'),
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
        lane_ops = 3.0 * R * n_u * ni
        if scope in scopes:                     # (a PEA_LIB build may name its launches otherwise)
            res[name + '_scan_lane_ops_per_s'] = round(lane_ops / (scopes[scope] * 1e-3), 0)
            res[name + '_scan_share_of_vector_floor'] = round(lane_ops / LANE_RATE / (scopes[scope] * 1e-3), 3)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
