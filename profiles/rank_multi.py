"""Measurement of the multi-positive all-item evaluation (include/peahip_eval.h: engine.rank_full_multi, engine.dot_rank_full_multi)
against the flattened route on the single-positive entry points, at the catalogue of the headline preset.

    timeout -k 10 900 python profiles/rank_multi.py [--users 162541] [--items 59047] [--r 16] [--d 112] [--max-pos 20]
                                                    [--repeats 10] [--warmup 2] [--out profiles/r13/rank_multi_r13.json]
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python profiles/rank_multi.py --trace-only      (a run of its own)
    python profiles/rank_multi.py --kernel-stats DIR/.../trace_kernel_stats.csv --out FILE              (folds it into FILE)

Shape: every user against every item, the users' seen items excluded (log-normal degrees scaled to the preset's interactions,
as profiles/recommend_dot.py), both scorers: the fc1 / fc2 scorer on an [N, --r] table, the inner product on an [N, --d] table.
  leg 'multi'  positives per user drawn uniformly from 1 .. --max-pos (distinct catalogue items, ascending)
  leg 'one'    exactly one positive per user
Yardstick: the flattened route, i.e. engine.rank_full / engine.dot_rank_full -- one (user, positive) pair per flat positive,
the pair's exclusion row the sorted union of the user's seen items and the user's positives (built once, outside the timed
region: only the kernel time of the route is charged).  On the inner product both sides run the same kernels (dot_rank_full
is dot_rank_full_multi without a row pointer): the yardstick is another ROW LAYOUT of them, one scan row of one threshold per
flat pair against chunked rows of up to 8 thresholds per user, so its 'one' leg compares a call with itself but for the row
pointer.  On the fc scorer rank_full has a scan of its own.
Timing: HIP events around each call, warm-up, the two sides alternated call by call in one process, median.  The per-launch
split of the library's own events (pea_profile_*) comes from one extra call per side; the per-kernel split of rocprofv3
from a run of its own (--trace-only: one warm call and one traced call per form, leg and side).  One JSON line (also --out).
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

from recommend_dot import event_ms, exclusion_lists, profile_scopes    # noqa: E402


def positives(n_users, lo, n_items, max_pos, seed):
    """(rowptr, items): per user 1 .. max_pos distinct catalogue items, ascending (a repeated draw is dropped, so a few users
    hold one fewer than drawn; every user keeps at least one)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    cnt = torch.randint(1, max_pos + 1, (n_users,), device='cuda', generator=g)
    users = torch.repeat_interleave(torch.arange(n_users, device='cuda'), cnt)
    items = torch.randint(0, n_items, (users.numel(),), device='cuda', generator=g)
    keys = torch.unique(users * n_items + items)
    ku = torch.div(keys, n_items, rounding_mode='floor')
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device='cuda')
    rowptr[1:] = torch.cumsum(torch.bincount(ku, minlength=n_users), 0)
    return rowptr, keys % n_items + lo


def flatten(n_users, lo, n_items, excl, pos):
    """the arguments of the flattened route: (users [Q], positives [Q], (rowptr [Q + 1], union rows))"""
    e_ptr, e_items = excl
    p_ptr, p_items = pos
    arange = torch.arange(n_users, device='cuda')
    eu = torch.repeat_interleave(arange, e_ptr[1:] - e_ptr[:-1])
    pu = torch.repeat_interleave(arange, p_ptr[1:] - p_ptr[:-1])
    keys = torch.unique(torch.cat([eu * n_items + (e_items - lo), pu * n_items + (p_items - lo)]))
    ku = torch.div(keys, n_items, rounding_mode='floor')
    u_ptr = torch.zeros(n_users + 1, dtype=torch.int64, device='cuda')
    u_ptr[1:] = torch.cumsum(torch.bincount(ku, minlength=n_users), 0)
    union = keys % n_items + lo
    del keys, ku, eu
    size = (u_ptr[1:] - u_ptr[:-1])[pu]                       # per flat positive: its user's union row
    f_ptr = torch.zeros(pu.numel() + 1, dtype=torch.int64, device='cuda')
    f_ptr[1:] = torch.cumsum(size, 0)
    total = int(f_ptr[-1])
    row = torch.repeat_interleave(torch.arange(pu.numel(), device='cuda'), size, output_size=total)
    within = torch.arange(total, device='cuda') - f_ptr[:-1][row]
    f_items = union[u_ptr[:-1][pu][row] + within]
    return pu.contiguous(), p_items, (f_ptr, f_items)


def fold_kernel_stats(path):
    """{kernel name (template arguments cut): [calls, total ms]} of a rocprofv3 --kernel-trace --stats table, the kernels of
    csrc/topk.hip and csrc/dot_score.hip only"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row['Name']
            if not any(k in name for k in ('rank_', 'topk_', 'dot_')):
                continue
            short = name.replace('void ', '').replace('pea::(anonymous namespace)::', '').split('(')[0]
            cur = out.setdefault(short, [0, 0.0])
            cur[0] += int(row['Calls'])
            cur[1] = round(cur[1] + float(row['TotalDurationNs']) / 1e6, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=162541)
    ap.add_argument('--items', type=int, default=59047)
    ap.add_argument('--interactions', type=int, default=24800000)
    ap.add_argument('--r', type=int, default=16)
    ap.add_argument('--d', type=int, default=112)
    ap.add_argument('--max-pos', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.loads(f.read())
        res['rocprofv3_kernel_stats_calls_ms'] = fold_kernel_stats(a.kernel_stats)
        res['rocprofv3_run'] = 'one warm call and one more per form, leg and side (--trace-only), a run of its own'
        line = json.dumps(res)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
        print(line)
        return
    from graph_recsys_benchmark_amd import engine
    torch.cuda.set_device(0)
    nu, ni = a.users, a.items
    lo, n_nodes = nu, nu + ni + 1000
    g = torch.Generator().manual_seed(0)
    tables = {'mlp': torch.randn(n_nodes, a.r, generator=g).cuda(), 'dot': torch.randn(n_nodes, a.d, generator=g).cuda()}
    torch.manual_seed(0)
    fc1, fc2 = torch.nn.Linear(2 * a.r, a.r), torch.nn.Linear(a.r, 1)
    fc = tuple(t.detach().cuda() for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias))
    excl = exclusion_lists(nu, lo, ni, a.interactions, 1)
    users_all = torch.arange(nu, device='cuda')
    legs = {'multi': positives(nu, lo, ni, a.max_pos, 2), 'one': positives(nu, lo, ni, 1, 3)}
    item_range = (lo, lo + ni)
    res = {'users': nu, 'items': ni, 'R': a.r, 'D': a.d, 'excluded_pairs': int(excl[1].numel()),
           'timing': 'HIP events, sides alternated call by call, median of %d after %d warm-up' % (a.repeats, a.warmup)}

    def native(form, pos):
        if form == 'mlp':
            return lambda: engine.rank_full_multi(tables['mlp'], users_all, pos[0], pos[1], item_range, *fc, exclude=excl)
        return lambda: engine.dot_rank_full_multi(tables['dot'], users_all, pos[0], pos[1], item_range, exclude=excl)

    def flat(form, args):
        fu, fp, fex = args
        if form == 'mlp':
            return lambda: engine.rank_full(tables['mlp'], fu, fp, item_range, *fc, exclude=fex)
        return lambda: engine.dot_rank_full(tables['dot'], fu, fp, item_range, exclude=fex)

    for leg, pos in legs.items():
        args = flatten(nu, lo, ni, excl, pos)
        res[leg + '_positives'] = int(pos[1].numel())
        res[leg + '_flattened_exclusion_entries'] = int(args[2][1].numel())
        for form in ('mlp', 'dot'):
            nat, fl = native(form, pos), flat(form, args)
            key = '%s_%s' % (form, leg)
            if a.trace_only:
                for fn in (nat, fl, nat, fl):
                    fn()
                torch.cuda.synchronize()
                continue
            # the two routes give the same integers (tests/test_gpu_rank_multi.py); checked here too, at size
            above, below, ps, n_neg = nat()
            rank, auc, ps2 = fl()
            assert torch.equal(above, rank) and torch.equal(ps, ps2), key
            for _ in range(a.warmup):
                nat(); fl()
            torch.cuda.synchronize()
            n_ms, f_ms = [], []
            for _ in range(a.repeats):
                n_ms.append(event_ms(nat))
                f_ms.append(event_ms(fl))
            n_ms.sort(); f_ms.sort()
            mid = len(n_ms) // 2
            res[key + '_native_ms'] = round(n_ms[mid], 4)
            res[key + '_flattened_ms'] = round(f_ms[mid], 4)
            res[key + '_native_min_max_ms'] = [round(n_ms[0], 4), round(n_ms[-1], 4)]
            res[key + '_flattened_min_max_ms'] = [round(f_ms[0], 4), round(f_ms[-1], 4)]
            res[key + '_flattened_over_native'] = round(f_ms[mid] / n_ms[mid], 3)
            res[key + '_native_launch_ms'] = profile_scopes(nat)
            res[key + '_flattened_launch_ms'] = profile_scopes(fl)
        del args
        torch.cuda.empty_cache()
    if a.trace_only:
        return
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
