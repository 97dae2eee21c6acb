"""Measurement of NFMRecsysModel's HIP routes against the same model's torch composition on one GPU, at the project's
ml25m shape: 162,541 users, 59,047 items, emb_dim = hidden_size = 64, dropout 0.3.

    timeout -k 10 900 python profiles/tools/nfm_measure.py [--repeats 10] [--out profiles/r15/nfm_r15.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/tools/nfm_measure.py --trace 5

Legs, each native against torch in the same process, the two sides alternated call by call:
  (a) loss() + backward() at B = 1024 and 4096      native_train=True  vs  native_train=False
  (b) the same plus Adam.step()
  (c) eval(): the fold                              native=True        vs  native=False (the torch fold)
  (d) rank_eval of all users x 100 candidates
  (e) recommend top-20 for 1,024 users over the whole catalogue
Timing: HIP events around one call, warm-up first, median of the repeats with min and max stated.  The per-phase times of
the native side come from the library's own events (pea_profile_*) in one extra call; each is set against its floor: the
phase's compulsory bytes at 8 TB/s for the training step (latency-bound, as HeRec's), MFMA flops 2 E H per pair at 155 TF or
the gathered bytes at 8 TB/s, whichever is larger, for the scorer.  One JSON line (also written to --out).

    timeout -k 10 900 python profiles/tools/nfm_measure.py --scan [--full] [--out profiles/r16/nfm_scan_r16.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/tools/nfm_measure.py --scan --trace 3

--scan measures the fused catalogue scan (csrc/nfm_scan.hip) against the SAME model with fused_scan=False in the same run:
  (f) recommend top-20 for 1,024 users
  (g) rank_full for 4,096 users with exclusion rows of ml25m's density (24.7 M entries over 162,541 users: 152 a user)
  (h) rank_full_multi for 4,096 users with 1..20 positives each, against solvers.rank_full_multi_flattened over the composition
  (i) --full: the fused top-20 and rank_full for all 162,541 users, one call each
with the mismatches between the two sides at the timed size, the peak memory of either side and the fused side's launches
against the MFMA floor 2 EP HP pairs / 155 TF."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'profiles'))

from kg_train import event_ms, peak_bytes, profile_launches      # noqa: E402

N_USER, N_ITEM = 162541, 59047
HBM, MFMA = 8.0e12, 155.0e12


def alternated(first, second, warmup, repeats):
    """[median, min, max] ms of each of two callables, alternated call by call after `warmup` calls of each"""
    for _ in range(warmup):
        first()
        second()
    torch.cuda.synchronize()
    f, s = [], []
    for _ in range(repeats):
        f.append(event_ms(first))
        s.append(event_ms(second))
    f.sort()
    s.sort()
    return [[round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)] for v in (f, s)]


def train_floors_us(e, h, b):
    """compulsory bytes of each phase of the training step -> microseconds at 8 TB/s"""
    wg = min((b + 15) // 16, 128)
    by = {
        'nfm_c': 4.0 * (2 * b * e + b * e + wg * 3 * e),                         # two gathered rows, c out, the partials
        'nfm_h': 4.0 * (b * e + b * h + wg * (h * e + 3 * h)) + b * e,           # c in, h out, W1 per workgroup, mask bytes
        'nfm_out': 4.0 * (b * h + 4 * b + wg * (3 * h + 2)) + b * h,
        'nfm_bwd': 4.0 * (2 * b * e + b * h + b * e + wg * (2 * h * e + h + 2 * e)) + b * (e + h),
        'nfm_rows': 4.0 * (2 * b * e + 2 * b * e + 2 * b * (e + 4)),
    }
    return {k: 1e6 * v / HBM for k, v in by.items()}


def with_floors(launches, floors):
    return [[nm, round(1e3 * ms, 2), round(floors[nm], 3) if nm in floors else None] for nm, ms in launches]


def build(native, native_train):
    from graph_recsys_benchmark_amd.models import NFMRecsysModel
    return NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=64, hidden_size=64, dropout=0.3, acc_uids=0, acc_iids=N_USER,
                          native=native, native_train=native_train).cuda()


def exclusion_rows(users, per_user, gen):
    """(rowptr, items) on the GPU: per requested user a strictly ascending row of item NODE ids, `per_user` on average"""
    n = users.numel()
    counts = torch.randint(per_user // 2, per_user + per_user // 2 + 1, (n,), generator=gen)
    rows = torch.repeat_interleave(torch.arange(n), counts).cuda()
    keys = torch.unique(rows * N_ITEM + torch.randint(0, N_ITEM, (rows.numel(),), generator=gen).cuda())      # sorted, no duplicates
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
    rowptr[1:] = torch.cumsum(torch.bincount(keys // N_ITEM, minlength=n), 0)
    return rowptr, N_USER + keys % N_ITEM


def positive_rows(n, gen):
    """(pos_rowptr, pos_items) on the GPU: 1..20 positives per user, strictly ascending item NODE ids"""
    counts = torch.randint(1, 21, (n,), generator=gen)
    rows = torch.repeat_interleave(torch.arange(n), counts).cuda()
    keys = torch.unique(rows * N_ITEM + torch.randint(0, N_ITEM, (rows.numel(),), generator=gen).cuda())
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
    rowptr[1:] = torch.cumsum(torch.bincount(keys // N_ITEM, minlength=n), 0)
    return rowptr, N_USER + keys % N_ITEM


def scan_main(a):
    import numpy as np
    from graph_recsys_benchmark_amd import solvers
    from graph_recsys_benchmark_amd.models import NFMRecsysModel
    torch.cuda.set_device(0)
    torch.manual_seed(1)
    gen = torch.Generator().manual_seed(0)
    kw = dict(num_users=N_USER, num_items=N_ITEM, emb_dim=64, hidden_size=64, dropout=0.3, acc_uids=0, acc_iids=N_USER)
    composed = NFMRecsysModel(fused_scan=False, **kw).cuda()
    fused = NFMRecsysModel(fused_scan=True, **kw).cuda()
    fused.load_state_dict(composed.state_dict())
    composed.eval()
    fused.eval()
    rng = (N_USER, N_USER + N_ITEM)
    u1k = torch.randint(0, N_USER, (1024,), generator=gen).cuda()
    u4k = torch.randint(0, N_USER, (4096,), generator=gen).cuda()
    excl4k = exclusion_rows(u4k, 152, gen)
    pos4k = (N_USER + torch.randint(0, N_ITEM, (4096,), generator=gen)).cuda()
    multi4k = positive_rows(4096, gen)
    flat_args = (u4k.cpu().numpy(), multi4k[0].cpu().numpy(), multi4k[1].cpu().numpy(), rng, excl4k)
    flattened = lambda: solvers.rank_full_multi_flattened(composed.rank_full, *flat_args, device='cuda')
    legs = {
        'recommend_top20_1024': (lambda: fused.recommend(u1k, 20, rng), lambda: composed.recommend(u1k, 20, rng), 1024 * N_ITEM),
        'rank_full_4096': (lambda: fused.rank_full(u4k, pos4k, rng, exclude=excl4k),
                           lambda: composed.rank_full(u4k, pos4k, rng, exclude=excl4k), 4096 * N_ITEM),
        'rank_full_multi_4096': (lambda: fused.rank_full_multi(u4k, multi4k[0], multi4k[1], rng, exclude=excl4k), flattened, 4096 * N_ITEM),
    }
    if a.trace:
        for _ in range(a.trace):
            for first, _, _ in legs.values():
                first()
        torch.cuda.synchronize()
        return
    res = {'users': N_USER, 'items': N_ITEM, 'emb_dim': 64, 'hidden_size': 64, 'exclusion_entries_4096': int(excl4k[1].numel()),
           'positives_4096': int(multi4k[1].numel()),
           'timing': 'HIP events, fused and composition alternated, [median, min, max] ms of %d after %d warm-up' % (a.repeats, a.warmup),
           'floor': 'MFMA: 2 EP HP flops per pair at 155 TF'}
    for name, (first, second, pairs) in legs.items():
        res[name + '_fused_ms'], res[name + '_composed_ms'] = alternated(first, second, a.warmup, a.repeats)
        res[name + '_fused_peak_MB'] = round(peak_bytes(first) / 1e6, 1)
        res[name + '_composed_peak_MB'] = round(peak_bytes(second) / 1e6, 1)
        floor_us = 1e6 * pairs * 2.0 * 64 * 64 / MFMA
        res[name + '_fused_launch_us'] = [[nm, round(1e3 * ms, 1)] for nm, ms in profile_launches(first)]
        res[name + '_floor_us'] = round(floor_us, 1)
        res[name + '_fused_wins'] = bool(res[name + '_fused_ms'][0] < res[name + '_composed_ms'][1])
        got, want = first(), second()
        to_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        res[name + '_mismatches'] = [int((to_np(g) != to_np(w)).sum()) for g, w in zip(got, want)]
    if a.full:
        users = torch.arange(N_USER, device='cuda')
        excl = exclusion_rows(users, 152, gen)
        pos = (N_USER + torch.randint(0, N_ITEM, (N_USER,), generator=gen)).cuda()
        res['full_exclusion_entries'] = int(excl[1].numel())
        res['full_floor_ms'] = round(1e3 * N_USER * N_ITEM * 2.0 * 64 * 64 / MFMA, 1)
        res['full_recommend_top20_fused_ms'] = round(event_ms(lambda: fused.recommend(users, 20, rng, exclude=excl)), 1)
        res['full_rank_full_fused_ms'] = round(event_ms(lambda: fused.rank_full(users, pos, rng, exclude=excl)), 1)
        res['full_rank_full_fused_peak_MB'] = round(peak_bytes(lambda: fused.rank_full(users, pos, rng, exclude=excl)) / 1e6, 1)
    else:
        res['full'] = 'not measured'
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scan', action='store_true', help='measure the fused catalogue scan against the composition and nothing else')
    ap.add_argument('--full', action='store_true', help='with --scan: one fused top-20 and one fused rank_full over all users as well')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--trace', type=int, default=0, help='run this many untimed native calls of each leg (B = 4096) and nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.scan:
        a.warmup, a.repeats = min(a.warmup, 1), min(a.repeats, 5)       # r15's protocol for the catalogue legs: median of 5
        return scan_main(a)
    torch.cuda.set_device(0)
    torch.manual_seed(1)
    gen = torch.Generator().manual_seed(0)
    off, on = build(False, False), build(True, True)
    on.load_state_dict(off.state_dict())
    opts = {id(m): torch.optim.Adam(m.parameters(), lr=1e-3) for m in (on, off)}
    res = {'users': N_USER, 'items': N_ITEM, 'emb_dim': 64, 'hidden_size': 64, 'dropout': 0.3,
           'timing': 'HIP events, sides alternated, [median, min, max] ms of %d after %d warm-up' % (a.repeats, a.warmup),
           'floors': 'training: bytes at 8 TB/s; scorer: MFMA flops 2 E H per pair at 155 TF or gathered bytes at 8 TB/s'}
    for size in (1024, 4096):
        batch = torch.stack([torch.randint(0, N_USER, (size,), generator=gen), torch.randint(0, N_ITEM, (size,), generator=gen),
                             torch.randint(0, 2, (size,), generator=gen)], dim=1).cuda()

        def step(model, adam=False):
            model.train()
            for p in model.parameters():
                p.grad = None
            loss = model.loss(batch)
            loss.backward()
            if adam:
                opts[id(model)].step()
            return loss

        key = 'b%d' % size
        if a.trace:
            for _ in range(a.trace if size == 4096 else 0):
                step(on, True)
            continue
        for leg, fn in (('step', step), ('step_adam', lambda mdl: step(mdl, True))):
            res['%s_%s_native_ms' % (key, leg)], res['%s_%s_torch_ms' % (key, leg)] = alternated(
                lambda: fn(on), lambda: fn(off), a.warmup, a.repeats)
            on.load_state_dict(off.state_dict())      # the Adam legs moved the two sides apart
        res[key + '_native_peak_MB'] = round(peak_bytes(lambda: step(on)) / 1e6, 1)
        res[key + '_torch_peak_MB'] = round(peak_bytes(lambda: step(off)) / 1e6, 1)
        res[key + '_native_phase_us_floor_us'] = with_floors(profile_launches(lambda: step(on)), train_floors_us(64, 64, size))

    on.load_state_dict(off.state_dict())      # the running statistics too: the two sides drew different masks
    if a.trace:
        on.eval()
    else:
        res['eval_fold_native_ms'], res['eval_fold_torch_ms'] = alternated(lambda: on.eval(), lambda: off.eval(), a.warmup, a.repeats)
        res['eval_fold_native_phase_us'] = with_floors(profile_launches(lambda: on.eval()), {})
        res['fold_max_abs_diff'] = float((on.folded.w - off.folded.w).abs().max())

    users = torch.arange(N_USER, device='cuda')
    cand = (N_USER + torch.randint(0, N_ITEM, (N_USER, 100), generator=gen)).cuda()
    if a.trace:
        for _ in range(a.trace):
            on.eval()
            on.rank_eval(users, cand)
            on.recommend(users[:1024], 20, (N_USER, N_USER + N_ITEM))
        torch.cuda.synchronize()
        return
    reps = max(a.repeats // 2, 3)
    res['rank_eval_native_ms'], res['rank_eval_torch_ms'] = alternated(lambda: on.rank_eval(users, cand), lambda: off.rank_eval(users, cand),
                                                                       1, reps)
    pairs = N_USER * 100
    floor = 1e6 * max(pairs * 2.0 * 64 * 64 / MFMA, pairs * (64 * 4.0 + 8 + 8) / HBM)
    res['rank_eval_native_phase_us_floor_us'] = with_floors(profile_launches(lambda: on.rank_eval(users, cand)), {'nfm_score': floor})
    res['rank_eval_rank_mismatches'] = int((on.rank_eval(users, cand)[1] != off.rank_eval(users, cand)[1]).sum())

    some = torch.randint(0, N_USER, (1024,), generator=gen).cuda()
    rng = (N_USER, N_USER + N_ITEM)
    res['recommend_native_ms'], res['recommend_torch_ms'] = alternated(lambda: on.recommend(some, 20, rng), lambda: off.recommend(some, 20, rng),
                                                                       1, reps)
    pairs = 256 * N_ITEM
    floor = 1e6 * max(pairs * 2.0 * 64 * 64 / MFMA, pairs * (64 * 4.0 + 4) / HBM)
    res['recommend_native_phase_us_floor_us'] = with_floors(profile_launches(lambda: on.recommend(some, 20, rng)), {'nfm_score': floor})
    res['recommend_item_mismatches'] = int((on.recommend(some, 20, rng)[0] != off.recommend(some, 20, rng)[0]).sum())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
