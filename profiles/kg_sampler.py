"""Measurement of the on-device KG triple sampler (csrc/kg_sampler.hip) on every triple of the ml25m_shaped KG, and of the CFKG
KG phase fed by it.

    timeout -k 10 1100 python profiles/kg_sampler.py [--preset ml25m_shaped] [--repeats 10] [--steps 200] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/kg_sampler.py --trace 3

Legs:
  host     utils.kg_negative_sampling (the reference's numpy / torch calls on the CPU) plus the copy of its table to the
           device; wall clock, --host-runs runs.
  torch    the same table composed on the GPU by torch: randint, stack, randperm, index.  The yardstick.
  native   one pea_kg_sample launch for random / typed / typed + filtered, with the shuffle off and on.
           torch and native are timed with HIP events around the calls alone (no host read inside), the two sides alternated call
           by call, median of --repeats; the key table of the filtered draws (torch.unique, once per store) is timed apart.
  phase    --steps steps of the CFKG KG phase at batch 4096, wall clock between synchronisations: the reference driver's loop
           (CPU table, one batch copied per step, every loss read with .item()) against solvers.kg_epoch on the device table.
           Both over plain slices of their table: the reference's DataLoader machinery is left out of its side.
Peak memory of a leg is torch.cuda.max_memory_allocated over one call minus what was allocated before it.  The byte floor
of a launch is 16 bytes read and 32 written per triple at 8 TB/s.  --trace K runs K native launches of every variant and
nothing else, for a kernel trace taken from outside.  One JSON line (also written to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kg_train import alternated, event_ms      # noqa: E402

HBM_BYTES_PER_S = 8.0e12
SEED = (7 << 32) | 2020


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = sorted(event_ms(fn) for _ in range(repeats))
    return t[len(t) // 2]


def extra_peak_bytes(fn):
    """peak of allocated device memory during fn() above what was allocated before it (its result included)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated()) - int(before)
    del out
    return peak


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-runs', type=int, default=3)
    ap.add_argument('--trace', type=int, default=0, help='run this many native launches of every variant and nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd import _lib, solvers
    from graph_recsys_benchmark_amd.models import CFKGRecsysModel
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, kg_negative_sampling, kg_triple_store
    torch.cuda.set_device(0)
    lib = _lib.require_device()
    note = lambda text: print(text, file=sys.stderr, flush=True)
    d = SyntheticHIN(a.preset)
    store = kg_triple_store(d, 'cuda')
    note('store built: %d triples' % store.num_triples)
    n, n_nodes = store.num_triples, store.num_nodes
    out = torch.empty((n, 4), dtype=torch.int64, device='cuda')
    exhausted = torch.zeros(1, dtype=torch.int32, device='cuda')
    epoch = [0]

    def native(strategy, filtered, shuffle):
        lo, cnt = (store.seg_lo, store.seg_n) if strategy == 'typed' else (store.any_lo, store.any_n)
        keys = store.keys() if filtered else None
        epoch[0] += 1
        _lib.check(lib.pea_kg_sample(n, _lib.ptr(store.heads), _lib.ptr(store.tails), store.num_segments, _lib.ptr(store.seg_ptr),
                                     _lib.ptr(store.seg_rel), _lib.ptr(lo), _lib.ptr(cnt), n_nodes, _lib.ptr(keys),
                                     0 if keys is None else keys.numel(), SEED, epoch[0], shuffle, _lib.ptr(out), 4,
                                     _lib.ptr(exhausted), _lib.current_stream()))
        return out

    variants = [(s, f, form) for s, f in (('random', False), ('typed', False), ('typed', True)) for form in (0, 1)]
    form_name = {0: 'ordered', 1: 'shuffled'}
    if a.trace:
        store.keys()
        for v in variants:
            for _ in range(a.trace):
                native(*v)
        torch.cuda.synchronize()
        return

    res = {'preset': a.preset, 'nodes': n_nodes, 'relations': store.num_segments, 'triples': n,
           'timing': 'HIP events around the calls, torch and native alternated, median of %d after %d warm-up; host and phase legs: '
                     'wall clock between synchronisations' % (a.repeats, a.warmup)}
    floor_ms = 48.0 * n / HBM_BYTES_PER_S * 1e3
    res['byte_floor_ms'] = round(floor_ms, 4)

    # ---- host leg
    host = []
    for k in range(a.host_runs):
        np.random.seed(k)
        torch.manual_seed(k)
        ms, table = wall_ms(lambda: kg_negative_sampling(d).cuda())
        host.append(ms)
        note('host run %d: %.0f ms' % (k, ms))
    res['host_ms_runs'] = [round(t, 1) for t in host]
    res['host_ms'] = round(sorted(host)[len(host) // 2], 1)
    res['host_peak_MB'] = round(table.numel() * 8 / 1e6, 1)           # the device holds the copied table alone
    cpu_table = d.train_data
    del table

    # ---- torch composition on the device
    rel_col = store.seg_rel[store.segment_of_rows()]

    def composed():
        neg = torch.randint(0, n_nodes, (n,), device='cuda', dtype=torch.int64)
        table = torch.stack([store.heads, store.tails, neg, rel_col], dim=1)
        return table[torch.randperm(n, device='cuda')]

    nat_ms, torch_ms = alternated(lambda: native('random', False, 1), composed, a.warmup, a.repeats)
    res['torch_ms'] = round(torch_ms, 4)
    res['torch_peak_MB'] = round(extra_peak_bytes(composed) / 1e6, 1)
    res['native_random_shuffled_alternated_ms'] = round(nat_ms, 4)
    res['native_over_torch'] = round(torch_ms / nat_ms, 3)
    res['native_over_host'] = round(res['host_ms'] / nat_ms, 1)

    note('torch %.3f ms, native %.3f ms' % (torch_ms, nat_ms))
    # ---- the native variants
    ms, _ = wall_ms(store.keys)
    res['key_table_build_ms'] = round(ms, 2)
    res['key_table_MB'] = round(store.keys().numel() * 8 / 1e6, 1)
    for strategy, filtered, form in variants:
        name = '%s%s_%s' % (strategy, '_filtered' if filtered else '', form_name[form])
        t = median_ms(lambda: native(strategy, filtered, form), a.warmup, a.repeats)
        res['native_%s_ms' % name] = round(t, 4)
        res['native_%s_x_floor' % name] = round(t / floor_ms, 2)
        res['native_%s_exhausted' % name] = int(exhausted.item())
    res['native_peak_MB'] = round(n * 32 / 1e6, 1)                     # the output table: the launch allocates nothing
    src = native('random', False, 0).clone()
    dst = torch.empty_like(src)
    res['permute_rows_w4_ms'] = round(median_ms(lambda: _lib.check(lib.pea_permute_rows(
        n, 4, _lib.ptr(src), 4, _lib.ptr(dst), 4, SEED, 1, _lib.current_stream())), a.warmup, a.repeats), 4)
    res['randperm_index_w4_ms'] = round(median_ms(lambda: src[torch.randperm(n, device='cuda')], a.warmup, a.repeats), 4)
    del src, dst

    note('variants timed')
    # ---- the CFKG KG phase, both ways, from the same weights
    def fresh():
        torch.manual_seed(1)
        model = CFKGRecsysModel(dataset=d, emb_dim=a.emb).cuda()
        return model.train(), torch.optim.Adam(model.parameters(), lr=1e-3)

    def reference_loop(model, opt, steps):
        losses = []
        for k in range(steps):
            batch = cpu_table[k * a.batch:(k + 1) * a.batch].cuda()
            opt.zero_grad()
            loss = model.kg_loss(batch)
            loss.backward()
            opt.step()
            losses.append(loss.detach().cpu().item())
        return float(np.mean(losses))

    dev_table = native('random', False, 1)
    model, opt = fresh()
    reference_loop(model, opt, 5)                                        # warm-up: allocator, lazy kernels
    solvers.kg_epoch(model, opt, dev_table, a.batch, max_steps=5)
    model, opt = fresh()
    ref_ms, ref_loss = wall_ms(lambda: reference_loop(model, opt, a.steps))
    model, opt = fresh()
    dev_ms, dev_loss = wall_ms(lambda: solvers.kg_epoch(model, opt, dev_table, a.batch, max_steps=a.steps))
    res['phase_steps'], res['phase_batch'] = a.steps, a.batch
    res['phase_reference_loop_ms_per_step'] = round(ref_ms / a.steps, 4)
    res['phase_kg_epoch_ms_per_step'] = round(dev_ms / a.steps, 4)
    res['phase_speedup'] = round(ref_ms / dev_ms, 3)
    res['phase_mean_loss_reference_kg_epoch'] = [round(ref_loss, 3), round(dev_loss, 3)]      # different negatives: not equal
    model, opt = fresh()
    res['phase_reference_loop_peak_MB'] = round(extra_peak_bytes(lambda: reference_loop(model, opt, 5)) / 1e6, 1)
    res['phase_kg_epoch_peak_MB'] = round(extra_peak_bytes(lambda: solvers.kg_epoch(model, opt, dev_table, a.batch, max_steps=5)) / 1e6, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
