"""Measurement of one KG-phase step (kg_loss(batch) + backward()) of KGAT / KGCN with native_kg on and off, on the
ml25m_shaped KG (N = 273,744 nodes) at emb = 64, batches of 1024 and 4096 quadruples.

    timeout -k 10 600 python profiles/kg_phase.py [--preset ml25m_shaped] [--emb 64] [--batches 1024,4096] [--repeats 20]
                                                  [--kinds kgat,kgcn] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/kg_phase.py --trace 5 --batches 4096

Both sides are the same model class with the same weights; the switch-off side is the torch composition of
models/kg_base.py, which is what the library ran before the switch existed, and is the yardstick.  A KG batch is positive
triples of the dataset's edge lists with their edge-type id and uniform random negative tails.

Timing: HIP events around kg_loss() + backward(), warm-up, the two sides alternated call by call in one process, median.
Per-launch times of the native side come from the library's own events (pea_profile_*) in one extra step; --trace K runs K
untimed steps of each side instead, for a kernel trace taken from outside.  One JSON line (also written to --out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kg_train import alternated, peak_bytes, profile_launches      # noqa: E402


def build(kind, d, emb, native_kg):
    from graph_recsys_benchmark_amd.models import KGATRecsysModel, KGCNRecsysModel
    from graph_recsys_benchmark_amd.utils import kg_graph_input

    class Model({'kgat': KGATRecsysModel, 'kgcn': KGCNRecsysModel}[kind]):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, 'cuda')

    return Model(dataset=d, emb_dim=emb, hidden_size=emb, dropout=0.1, native_kg=native_kg).cuda()


def kg_batch(d, size, rng):
    names = list(d.edge_index_nps.keys())
    counts = np.array([d.edge_index_nps[k].shape[1] for k in names], dtype=np.int64)
    rel = rng.choice(len(names), size=size, p=counts / counts.sum())
    rows = np.empty((size, 4), dtype=np.int64)
    for i, k in enumerate(rel):
        ei = d.edge_index_nps[names[k]]
        e = rng.integers(0, ei.shape[1])
        rows[i] = (ei[0, e], ei[1, e], rng.integers(0, d.num_nodes), k)
    return torch.from_numpy(rows).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--batches', default='1024,4096')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--kinds', default='kgat,kgcn')
    ap.add_argument('--trace', type=int, default=0, help='run this many untimed steps of each side and nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd.utils import SyntheticHIN
    torch.cuda.set_device(0)
    d = SyntheticHIN(a.preset)
    if not hasattr(d, 'num_edge_types'):
        d.num_edge_types = len(d.edge_index_nps)
    rng = np.random.default_rng(0)
    res = {'preset': a.preset, 'nodes': int(d.num_nodes), 'relations': int(d.num_edge_types), 'emb': a.emb,
           'timing': 'HIP events around kg_loss() + backward(), sides alternated, median of %d after %d warm-up' % (a.repeats, a.warmup)}
    for kind in a.kinds.split(','):
        torch.manual_seed(1)
        off = build(kind, d, a.emb, False)
        on = build(kind, d, a.emb, True)
        on.load_state_dict(off.state_dict())
        on.edge_index, on.edge_attr = off.edge_index, off.edge_attr
        for size in [int(s) for s in a.batches.split(',')]:
            batch = kg_batch(d, size, rng)

            def step(model):
                model.train()
                for p in model.parameters():
                    p.grad = None
                loss = model.kg_loss(batch)
                loss.backward()
                return loss

            key = '%s_b%d' % (kind, size)
            l_on, l_off = float(step(on)), float(step(off))
            if a.trace:
                for _ in range(a.trace):
                    step(on)
                    step(off)
                torch.cuda.synchronize()
                continue
            on_ms, off_ms = alternated(lambda: step(on), lambda: step(off), a.warmup, a.repeats)
            res[key + '_native_ms'] = round(on_ms, 4)
            res[key + '_torch_ms'] = round(off_ms, 4)
            res[key + '_speedup'] = round(off_ms / on_ms, 3)
            res[key + '_native_peak_MB'] = round(peak_bytes(lambda: step(on)) / 1e6, 1)
            res[key + '_torch_peak_MB'] = round(peak_bytes(lambda: step(off)) / 1e6, 1)
            res[key + '_loss_native_torch'] = [round(l_on, 3), round(l_off, 3)]
            res[key + '_native_launch_ms'] = [[nm, round(ms, 4)] for nm, ms in profile_launches(lambda: step(on))]
        del on, off
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
