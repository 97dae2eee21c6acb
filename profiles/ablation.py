"""Measurement of the one-pass metapath ablation sweep (csrc/ablate.hip) on the headline preset.

    timeout -k 10 900 python profiles/ablation.py [--preset ml25m_shaped] [--kind gat] [--cand 100] [--repeats 20]
                                                  [--warmup 3] [--sweep-only] [--out profiles/r05/ablation_r05.json]

Workload: every user of the preset (ml25m_shaped: 162,541) ranked on ONE pre-drawn block of 1 + 99 candidates (the
positive and the negatives uniform over the items: only the shapes matter for the timing), for all P + 1 ablation variants.
  (a) sweep      model.eval_ablation(keep_att=False) + engine.rank_eval_multi(model.ablation_repr, ...)
                 one forward, one fusion pass that writes the P + 1 tables, one ranking launch
  (b) composed   for v in 0 .. P:  model.eval(v - 1 or None);  engine.rank_eval(model.cached_repr, ...)
                 what the per-mask entry points give (the reference's loop, solvers.py:224-241): P + 1 forwards and launches
Both produce the same bytes (tests/test_gpu_ablation.py); here the last variant's ranks are compared once as a guard.

Timing: HIP events around each side, warm-up, the two sides alternated call by call in one process, median.  The split of
(a) by launch comes from the library's per-launch events (pea_profile_*) in one extra call.  The fusion pass reads the
stack once (N P R 4 bytes) and writes P + 1 tables ((P + 1) N R 4 bytes): its achieved bytes/s is reported against that sum.
--sweep-only runs (a) alone (the kernel-trace run: rocprofv3 --kernel-trace --stats -- python profiles/ablation.py
--sweep-only).  One JSON line; --out also writes it to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def build_model(dataset, kind, device):
    from graph_recsys_benchmark_amd import models
    from graph_recsys_benchmark_amd.utils import update_pea_graph_input
    base = {'gat': models.PEAGATRecsysModel, 'gcn': models.PEAGCNRecsysModel, 'sage': models.PEASageRecsysModel}[kind]
    dataset_args = dataset.dataset_args()
    train_args = {'device': device, 'num_metapaths': dataset.spec['num_metapaths']}

    class PEARecsysModel(base):
        def update_graph_input(self, ds):
            return update_pea_graph_input(dataset_args, train_args, dataset)

    torch.manual_seed(2020)
    model = PEARecsysModel(**dataset.model_args(kind=kind))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.uniform_(-0.05, 0.05)
    return model.to(device)


def launch_split(fn):
    """{launch name: [count, ms]} of one call, from the library's per-launch events"""
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.pea_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.pea_profile_enable(0)
    cap = 4096
    names, ms, units, cnt = C.create_string_buffer(cap * 32), (C.c_float * cap)(), (C.c_double * cap)(), C.c_int()
    lib.pea_profile_read(cap, names, ms, units, C.byref(cnt))
    out = {}
    for i in range(cnt.value):
        rec = out.setdefault(names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode(), [0, 0.0])
        rec[0] += 1
        rec[1] = round(rec[1] + ms[i], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--kind', default='gat', choices=['gat', 'gcn', 'sage'])
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--cand', type=int, default=100, help='candidates per user, the positive included')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sweep-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd import engine
    from graph_recsys_benchmark_amd.utils import SyntheticHIN
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    ds = SyntheticHIN(a.preset, seed=2019, scale=a.scale)
    model = build_model(ds, a.kind, dev)
    P, N, R = len(model.meta_path_steps), model.x.shape[0], model._dims[2]
    u0, i0 = ds.type_accs['uid'], ds.type_accs['iid']
    users = torch.arange(u0, u0 + ds.num_uids, device=dev)
    g = torch.Generator(device='cuda').manual_seed(1)
    cand = torch.randint(i0, i0 + ds.num_iids, (users.numel(), a.cand), generator=g, device=dev)
    fc = tuple(t.detach() for t in (model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias))

    last = {}

    def sweep():
        model.eval_ablation(keep_att=False)
        last['sweep'] = engine.rank_eval_multi(model.ablation_repr, users, cand, *fc)[1][P]

    def composed():
        for v in range(P + 1):
            model.eval(v - 1 if v else None)
            last['composed'] = engine.rank_eval(model.cached_repr, users, cand, *fc)[1]

    with torch.no_grad():
        for _ in range(a.warmup):
            sweep()
            if not a.sweep_only:
                composed()
        torch.cuda.synchronize()
        if not a.sweep_only:
            assert torch.equal(last['sweep'], last['composed']), 'the two sides rank the last variant differently'
        s_ms, c_ms = [], []
        for _ in range(a.repeats):
            s_ms.append(event_ms(sweep))
            if not a.sweep_only:
                c_ms.append(event_ms(composed))
        split = launch_split(sweep)
        split_composed = None if a.sweep_only else launch_split(composed)
    fuse_bytes = 4.0 * N * R * (P + (P + 1))
    res = {'preset': a.preset, 'scale': a.scale, 'kind': a.kind, 'num_nodes': N, 'metapaths': P, 'repr_dim': R,
           'users': int(users.numel()), 'candidates': a.cand, 'candidate_block': 'shared',
           'timing': 'HIP events, alternated, median of %d after %d warm-up' % (a.repeats, a.warmup),
           'a_sweep_ms': round(median(s_ms), 4), 'a_sweep_launch_ms': split,
           'fusion_pass_bytes': fuse_bytes, 'fusion_pass_ms': split['fuse_ablate'][1],
           'fusion_pass_bytes_per_s': round(fuse_bytes / (split['fuse_ablate'][1] * 1e-3), 0),
           'tables_bytes': 4.0 * (P + 1) * N * R}
    if not a.sweep_only:
        res['b_composed_ms'] = round(median(c_ms), 4)
        res['b_composed_launch_ms'] = split_composed
        res['speedup'] = round(median(c_ms) / median(s_ms), 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
