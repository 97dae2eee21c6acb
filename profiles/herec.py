"""Measurement of HeRecRecsysModel with native=True against native=False (the torch composition) on one GPU, at ml25m-shaped
sizes: N = 273,744 nodes, 162,541 users at 0, 59,047 items behind them, M = 2 metapath2vec tables of width D = 64 (seeded
random, scale 0.3), batches of 1024 and 4096 labelled pairs.

    timeout -k 10 600 python profiles/herec.py [--dim 64] [--tables 2] [--batches 1024,4096] [--repeats 10] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/herec.py --trace 5 --batches 4096

Legs: loss() + backward(); the same plus Adam.step(); eval() (the table build).  Both sides are the same model class with the
same weights.  Timing: HIP events, warm-up, the two sides alternated call by call in one process, median.  Per-launch times of
the native side come from the library's own events (pea_profile_*) in one extra step, each set against its floor (the
launch's compulsory bytes at 8 TB/s, or its MFMA flops at 155 TF, whichever is larger); --trace K runs K untimed steps of each
leg and side instead, for a kernel trace taken from outside.  One JSON line (also written to --out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kg_train import alternated, peak_bytes, profile_launches      # noqa: E402

N, N_USER, N_ITEM = 273744, 162541, 59047
HBM, MFMA = 8.0e12, 155.0e12


def floors_us(d, m, b):
    """Compulsory traffic and MFMA work per launch -> (bytes, flops, floor in microseconds)"""
    wg = min((b + 15) // 16, 256)
    rows = N_USER + N_ITEM
    out = {
        # rows of M tables and 4 embedding tables per pair, both ends; the weights once per workgroup; the gradient rows; the partials
        'herec_train': (4.0 * (2 * b * d * (m + 2) + wg * m * d * d + 4 * b * d + wg * m * d * (d + 1)), 2.0 * 2 * b * m * d * d * 2),
        'herec_final': (4.0 * wg * m * d * (d + 1), 0.0),
        'herec_table': (4.0 * (rows * d * (m + 2) + N * (d + 4)), 2.0 * rows * m * d * d),
    }
    return {k: (by, fl, 1e6 * max(by / HBM, fl / MFMA)) for k, (by, fl) in out.items()}


def build(tables, d, native):
    from graph_recsys_benchmark_amd.models import HeRecRecsysModel
    return HeRecRecsysModel(embeddings=tables, num_uids=N_USER, num_iids=N_ITEM, acc_uids=0, acc_iids=N_USER, embedding_dim=d,
                            native=native).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--tables', type=int, default=2)
    ap.add_argument('--batches', default='1024,4096')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--trace', type=int, default=0, help='run this many untimed steps of each leg and side and nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(0)
    tables = [(0.3 * torch.randn(N, a.dim, generator=gen)).cuda() for _ in range(a.tables)]
    torch.manual_seed(1)
    off = build(tables, a.dim, False)
    on = build(tables, a.dim, True)
    on.load_state_dict(off.state_dict())
    opts = {id(m): torch.optim.Adam(m.parameters(), lr=1e-3) for m in (on, off)}
    res = {'nodes': N, 'users': N_USER, 'items': N_ITEM, 'dim': a.dim, 'tables': a.tables,
           'timing': 'HIP events, sides alternated, median of %d after %d warm-up' % (a.repeats, a.warmup),
           'floors': 'bytes at 8 TB/s or MFMA flops at 155 TF, whichever is larger'}

    def evaluate(model):
        model.eval()
        return model.cached_repr

    for size in [int(s) for s in a.batches.split(',')]:
        batch = torch.stack([torch.randint(0, N_USER, (size,), generator=gen), N_USER + torch.randint(0, N_ITEM, (size,), generator=gen),
                             torch.randint(1, 6, (size,), generator=gen)], dim=1).cuda()

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
        l_on, l_off = step(on).item(), step(off).item()
        if a.trace:
            for _ in range(a.trace):
                step(on)
                step(off)
            torch.cuda.synchronize()
            continue
        res[key + '_loss_native_torch'] = [round(l_on, 4), round(l_off, 4)]
        for leg, fn in (('step', step), ('step_adam', lambda mdl: step(mdl, True))):
            on_ms, off_ms = alternated(lambda: fn(on), lambda: fn(off), a.warmup, a.repeats)
            res['%s_%s_native_ms' % (key, leg)] = round(on_ms, 4)
            res['%s_%s_torch_ms' % (key, leg)] = round(off_ms, 4)
            res['%s_%s_speedup' % (key, leg)] = round(off_ms / on_ms, 3)
            on.load_state_dict(off.state_dict())      # the Adam legs moved the two sides apart by rounding
        res[key + '_native_peak_MB'] = round(peak_bytes(lambda: step(on)) / 1e6, 1)
        res[key + '_torch_peak_MB'] = round(peak_bytes(lambda: step(off)) / 1e6, 1)
        fl = floors_us(a.dim, a.tables, size)
        res[key + '_native_launch_us_floor_us'] = [[nm, round(1e3 * ms, 2), round(fl[nm][2], 2) if nm in fl else None]
                                                   for nm, ms in profile_launches(lambda: step(on))]
    if a.trace:
        for _ in range(a.trace):
            evaluate(on)
            evaluate(off)
        torch.cuda.synchronize()
        return
    on_ms, off_ms = alternated(lambda: evaluate(on), lambda: evaluate(off), a.warmup, a.repeats)
    res['eval_native_ms'], res['eval_torch_ms'], res['eval_speedup'] = round(on_ms, 4), round(off_ms, 4), round(off_ms / on_ms, 3)
    fl = floors_us(a.dim, a.tables, 0)
    res['eval_native_launch_us_floor_us'] = [[nm, round(1e3 * ms, 2), round(fl[nm][2], 2) if nm in fl else None]
                                             for nm, ms in profile_launches(lambda: evaluate(on))]
    res['eval_table_max_abs_diff'] = float((evaluate(on) - evaluate(off)).abs().max())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
