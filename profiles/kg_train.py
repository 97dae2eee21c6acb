"""Measurement of one training step (loss() + backward()) of KGAT / KGCN / NGCF with native_train on and off, on the
ml25m_shaped KG at the reference's own shape emb = hidden = 64, batch 4096, dropout 0.1.

    timeout -k 10 900 python profiles/kg_train.py [--preset ml25m_shaped] [--emb 64] [--hidden 64] [--batch 4096]
                                                  [--dropout 0.1] [--repeats 20] [--kinds kgat,kgcn,ngcf] [--out FILE]

Both sides are the same model class with the same weights and graph; the flag-off side is the autograd path (HIP
aggregate + torch dense update + torch loss).  The attention map (KGAT / KGCN) is computed once outside the timed region,
as the solver recomputes it per epoch, not per step.

Timing: HIP events around loss() + backward(), warm-up, the two sides alternated call by call in one process, median.
torch.cuda.max_memory_allocated is taken over one extra step of each side after reset_peak_memory_stats.  Per-launch
times come from the library's own events (pea_profile_*) in one extra native step; every kg_update launch is set against
its two floors: flops over the 155 TF of the f32-input MFMA, and compulsory bytes over 8 TB/s
  forward   2 N in out nw flop,  4 N (2 in + out) + N out [keep] bytes
  backward  6 N in out nw flop,  4 N (4 in + out) + N out [keep] bytes        (nw = 2 weights, 1 for KGCN)
One JSON line (also written to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_FLOPS = 155e12
HBM_BYTES_PER_S = 8e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(first, second, warmup, repeats):
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
    return f[len(f) // 2], s[len(s) // 2]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated())


def profile_launches(fn):
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.pea_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.pea_profile_enable(0)
    cap = 256
    names, ms, units, cnt = C.create_string_buffer(cap * 32), (C.c_float * cap)(), (C.c_double * cap)(), C.c_int()
    lib.pea_profile_read(cap, names, ms, units, C.byref(cnt))
    return [(names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode(), float(ms[i])) for i in range(cnt.value)]


def build(kind, d, emb, hidden, dropout, native):
    from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel, NGCFRecsysModel
    from graph_recsys_benchmark_amd.utils import kg_graph_input
    if kind == 'ngcf':
        class Model(NGCFRecsysModel):
            def update_graph_input(self, dataset):
                u2i = torch.from_numpy(dataset.edge_index_nps['user2item'].astype(np.int64)).cuda()
                return torch.cat([u2i, torch.flip(u2i, dims=[0])], dim=1).contiguous()

        return Model(dataset=d, emb_dim=emb, hidden_size=hidden, dropout=dropout, entity_aware=False, entity_aware_coff=0.0,
                     if_use_features=False, native_train=native).cuda()

    class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, 'cuda')

    return Model(dataset=d, emb_dim=emb, hidden_size=hidden, dropout=dropout, native_train=native).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--kinds', default='kgat,kgcn,ngcf')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd.utils import SyntheticHIN
    torch.cuda.set_device(0)
    d = SyntheticHIN(a.preset)
    if not hasattr(d, 'num_edge_types'):
        d.num_edge_types = len(d.edge_index_nps)
    n = d.num_nodes
    rng = np.random.default_rng(0)
    u2i = d.edge_index_nps['user2item']
    pick = rng.choice(u2i.shape[1], size=a.batch, replace=False)
    lo = d.type_accs['iid']
    batch = torch.from_numpy(np.stack([u2i[0, pick], u2i[1, pick], rng.integers(lo, lo + d.num_iids, size=a.batch)],
                                      axis=1).astype(np.int64)).cuda()
    widths = [(a.emb, a.hidden), (a.hidden, a.hidden // 2), (a.hidden // 2, a.hidden // 4)]
    res = {'preset': a.preset, 'nodes': n, 'emb': a.emb, 'hidden': a.hidden, 'batch': a.batch, 'dropout': a.dropout,
           'timing': 'HIP events around loss() + backward(), sides alternated, median of %d after %d warm-up' % (a.repeats, a.warmup)}
    for kind in a.kinds.split(','):
        torch.manual_seed(1)
        off = build(kind, d, a.emb, a.hidden, a.dropout, False)
        on = build(kind, d, a.emb, a.hidden, a.dropout, True)
        on.load_state_dict(off.state_dict())
        if kind != 'ngcf':          # share the graph tensors (and so the cached plan) between the two sides
            on.edge_index, on.edge_attr = off.edge_index, off.edge_attr
        else:
            on.edge_index = off.edge_index
        res[kind + '_edges'] = int(off.edge_index.shape[1])
        att = None if kind == 'ngcf' else off.attention_map()
        nw = 1 if kind == 'kgcn' else 2

        def step(model):
            model.train()
            for p in model.parameters():
                p.grad = None
            loss = model.loss(batch) if kind == 'ngcf' else model.loss(batch, att)
            loss.backward()
            return loss

        l_on, l_off = float(step(on)), float(step(off))        # plans are built here
        on_ms, off_ms = alternated(lambda: step(on), lambda: step(off), a.warmup, a.repeats)
        res[kind + '_native_ms'] = round(on_ms, 3)
        res[kind + '_autograd_ms'] = round(off_ms, 3)
        res[kind + '_speedup'] = round(off_ms / on_ms, 3)
        res[kind + '_native_peak_MB'] = round(peak_bytes(lambda: step(on)) / 1e6, 1)
        res[kind + '_autograd_peak_MB'] = round(peak_bytes(lambda: step(off)) / 1e6, 1)
        res[kind + '_loss_native_autograd'] = [round(l_on, 3), round(l_off, 3)]
        launches = profile_launches(lambda: step(on))
        res[kind + '_native_launch_ms'] = [[nm, round(ms, 4)] for nm, ms in launches]
        total = {}
        for nm, ms in launches:
            total[nm] = total.get(nm, 0.0) + ms
        res[kind + '_native_launch_total_ms'] = {k: round(v, 4) for k, v in total.items()}
        res[kind + '_autograd_launch_total_ms'] = {}
        for nm, ms in profile_launches(lambda: step(off)):
            res[kind + '_autograd_launch_total_ms'][nm] = round(res[kind + '_autograd_launch_total_ms'].get(nm, 0.0) + ms, 4)
        # floors of the update launches, in launch order: forward conv1..3, backward conv3..1
        fwd = [ms for nm, ms in launches if nm == 'kg_update_fwd']
        bwd = [ms for nm, ms in launches if nm == 'kg_update_bwd']
        keep_b = 1.0 if a.dropout > 0 else 0.0
        rows = []
        for tag, times, order, fl, by in (('fwd', fwd, widths, 2.0, lambda i, o: 4.0 * (2 * i + o) + keep_b * o),
                                          ('bwd', bwd, widths[::-1], 6.0, lambda i, o: 4.0 * (4 * i + o) + keep_b * o)):
            for (fin, fout), ms in zip(order, times):
                mfma_ms = fl * n * fin * fout * nw / MFMA_F32_FLOPS * 1e3
                hbm_ms = n * by(fin, fout) / HBM_BYTES_PER_S * 1e3
                rows.append({'launch': 'kg_update_%s %d->%d' % (tag, fin, fout), 'ms': round(ms, 4), 'mfma_floor_ms': round(mfma_ms, 4),
                             'hbm_floor_ms': round(hbm_ms, 4), 'x_mfma_floor': round(ms / mfma_ms, 1),
                             'x_hbm_floor': round(ms / hbm_ms, 1)})
        res[kind + '_update_floors'] = rows
        del on, off, att
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
