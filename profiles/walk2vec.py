"""Measurement of one metapath2vec step (models/metapath2vec.py) with native on and off, on the ml25m_shaped preset with the
reference's metapath user -> item -> genre -> item -> user: emb 64, walk_length 100, context_size 7, 5 negative walks per
positive, 2,048 positive walks per step.

    timeout -k 10 900 python profiles/walk2vec.py [--preset ml25m_shaped] [--emb 64] [--walks 2048] [--repeats 10] [--out FILE]

Three legs, each native against the torch side on the same GPU:
  (a) sample():  csrc/walk.hip against a per-step torch composition on the GPU (rowptr gather, torch.rand, col gather, L
      rounds; torch.randint per step for the negative walks) -- the reference itself draws the positive walks on the CPU.
      The kernel leaves a walk at its dead end, the composition runs all L rounds for every walk: dead_end_walks and
      pos_mean_ids_per_walk in the JSON say how much of the positive side there is;
  (b) loss() + backward() with sparse on and off: csrc/skipgram.hip against native=False (the reference's formula) on the
      SAME walks and weights;
  (c) (b) + the optimiser step (SparseAdam for sparse, Adam for dense).
Timing: HIP events, warm-up, the two sides alternated call by call in one process, median.  Per-launch times of the native
step come from the library's own events (pea_profile_*) in one extra step, each with the bytes the launch must move (walk
rows read once, gradient rows written once, ...) and its distance from them at 8 TB/s.  Peak memory is what a step
allocates above what is live before it.  One JSON line (also to --out).
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

from kg_train import HBM_BYTES_PER_S, alternated, peak_bytes, profile_launches      # noqa: E402


def hin(d, genre_rel):
    """(edge_index_dict in global ids on the GPU, metapath, types, num_nodes_dict) as the reference's driver builds them
    (experiments/metapath2vec_solver_bpr.py:147-159)"""
    u2i = torch.from_numpy(d.edge_index_nps['user2item']).long().cuda()
    g2i = torch.from_numpy(d.edge_index_nps[genre_rel]).long().cuda()
    eid = {('genre', 'as the genre of', 'iid'): g2i, ('iid', 'has been watched by', 'uid'): torch.flip(u2i, [0]).contiguous(),
           ('uid', 'has watched', 'iid'): u2i, ('iid', 'has the genre', 'genre'): torch.flip(g2i, [0]).contiguous()}
    metapath = [('uid', 'has watched', 'iid'), ('iid', 'has the genre', 'genre'), ('genre', 'as the genre of', 'iid'),
                ('iid', 'has been watched by', 'uid')]
    types = [t for t, _ in d.spec['types']]
    return eid, metapath, types, dict(d.type_sizes)


def torch_sampler(model):
    """the per-step torch composition of both walk kinds on the GPU, over the same CSRs the kernel walks"""
    plan = model._get_plan()
    csrs = [tuple(t.long() for t in plan.export_csr(r)) for r in model._relations]
    lo = [model.start[k[-1]] for k in model.metapath]
    cnt = [model.num_nodes_dict[k[-1]] for k in model.metapath]
    length, wpn, nneg = model.walk_length, model.walks_per_node, model.num_negative_samples

    def sample(batch):
        cur = (batch + model.start[model.metapath[0][0]]).repeat(wpn)
        alive = torch.ones_like(cur, dtype=torch.bool)
        rws = [cur]
        for t in range(length):
            rowptr, col = csrs[t % len(csrs)]
            safe = cur.clamp(min=0)
            beg = rowptr[safe]
            deg = rowptr[safe + 1] - beg
            alive = alive & (deg > 0)
            slot = beg + (torch.rand(cur.shape, device=cur.device) * deg).long().minimum((deg - 1).clamp(min=0))
            cur = torch.where(alive, col[slot.clamp(max=col.numel() - 1)], torch.full_like(cur, -1))
            rws.append(cur)
        pos = torch.stack(rws, dim=-1)
        start = (batch + model.start[model.metapath[0][0]]).repeat(wpn * nneg)
        rws = [start]
        for t in range(length):
            s = t % len(lo)
            rws.append(torch.randint(lo[s], lo[s] + cnt[s], (start.numel(),), device=start.device))
        return pos, torch.stack(rws, dim=-1)

    return sample


def launch_floor(name, n, d, n_nodes, touched, rows):
    """bytes a launch of the native step must move"""
    return {'sg_grad_zero': 4.0 * n_nodes * d, 'sg_keys': 16.0 * n, 'sg_walk': 8.0 * n * d + 8.0 * n, 'sg_sort': 16.0 * n,
            'sg_runs': 4.0 * n * d + 8.0 * n + 4.0 * touched * d, 'sg_merge': 0.0, 'sg_touched': 9.0 * n + 4.0 * touched,
            'sg_final': 4.0 * rows}.get(name, 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--genre_rel', default='genre2item')
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--walk_length', type=int, default=100)
    ap.add_argument('--context_size', type=int, default=7)
    ap.add_argument('--negatives', type=int, default=5)
    ap.add_argument('--walks', type=int, default=2048)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd.models import MetaPath2Vec
    from graph_recsys_benchmark_amd.utils import SyntheticHIN
    torch.cuda.set_device(0)
    d = SyntheticHIN(a.preset)
    eid, metapath, types, counts = hin(d, a.genre_rel)

    def build(native, sparse):
        torch.manual_seed(1)
        return MetaPath2Vec(eid, a.emb, metapath, a.walk_length, a.context_size, counts, types, d.type_accs,
                            walks_per_node=1, num_negative_samples=a.negatives, sparse=sparse, native=native, seed=2019).cuda()

    sampler = build(True, False)
    batch = torch.from_numpy(np.random.default_rng(0).integers(0, counts['uid'], a.walks)).cuda()
    pos, neg = sampler.sample(batch)
    rows, t = pos.shape[0] + neg.shape[0], pos.shape[1]
    n, n_nodes = rows * t, sampler.embedding.num_embeddings
    ids = torch.cat([pos.reshape(-1), neg.reshape(-1)])
    touched = int(torch.unique(ids[ids >= 0]).numel())
    res = {'preset': a.preset, 'nodes': int(n_nodes), 'emb': a.emb, 'walk_length': a.walk_length, 'context_size': a.context_size,
           'pos_walks': int(pos.shape[0]), 'neg_walks': int(neg.shape[0]), 'positions': int(n), 'touched_nodes': touched,
           'dead_end_walks': int((pos[:, -1] < 0).sum()), 'pos_positions_reached': int((pos >= 0).sum()),
           'pos_mean_ids_per_walk': round(float((pos >= 0).sum()) / pos.shape[0], 2),
           'sort_bits': int(n - 1).bit_length() + int(n_nodes).bit_length(), 'posgrad_MB': round(4.0 * n * a.emb / 1e6, 1),
           'genre_nodes': int(counts['genre']),
           'longest_run': int(torch.bincount(ids[ids >= 0]).max()),
           'timing': 'HIP events, sides alternated, median of %d after %d warm-up' % (a.repeats, a.warmup)}

    # (a) sample()
    torch_sample = torch_sampler(sampler)
    on_ms, off_ms = alternated(lambda: sampler.sample(batch), lambda: torch_sample(batch), a.warmup, a.repeats)
    res.update(sample_native_ms=round(on_ms, 4), sample_torch_ms=round(off_ms, 4), sample_speedup=round(off_ms / on_ms, 2))
    # a walk launch must write its walks once (8 bytes per id); the CSR reads of the positive walks come on top
    walk_bytes = {'metapath_walks': 8.0 * pos.numel(), 'uniform_walks': 8.0 * neg.numel()}
    res['sample_native_launch_ms_floor_ms_ratio'] = [
        [nm, round(ms, 4), round(walk_bytes[nm] / HBM_BYTES_PER_S * 1e3, 5), round(ms / (walk_bytes[nm] / HBM_BYTES_PER_S * 1e3), 1)]
        for nm, ms in profile_launches(lambda: sampler.sample(batch))]
    del sampler
    torch.cuda.empty_cache()

    # (b), (c) loss() + backward() (+ optimiser step), sparse on and off
    for sparse in (True, False):
        on, off = build(True, sparse), build(False, sparse)
        off.load_state_dict(on.state_dict())
        opt_class = torch.optim.SparseAdam if sparse else torch.optim.Adam
        opts = {id(on): opt_class(list(on.parameters()), lr=0.01), id(off): opt_class(list(off.parameters()), lr=0.01)}

        def step(model, optimise):
            model.embedding.weight.grad = None
            loss = model.loss(pos, neg)
            loss.backward()
            if optimise:
                opts[id(model)].step()
            return loss

        key = 'sparse' if sparse else 'dense'
        l_on, l_off = step(on, False).item(), step(off, False).item()
        res[key + '_loss_native_torch'] = [round(l_on, 5), round(l_off, 5)]
        if sparse:
            # the same formula in float64: where a pair's score leaves float32's 1 - sigmoid (beyond ~17) the torch side's term
            # sticks at -log(1e-15) and its gradient at 0; the kernel forms 1 - sigmoid as sigmoid(-x)
            with torch.no_grad():
                res['loss_float64'] = round(float(build(False, False).double().loss(pos, neg)), 5)
            torch.cuda.empty_cache()
        g_on, g_off = on.embedding.weight.grad, off.embedding.weight.grad
        g_on, g_off = (g.to_dense() if g.is_sparse else g for g in (g_on, g_off))
        res[key + '_grad_max_abs_diff'] = float((g_on - g_off).abs().max())
        res[key + '_grad_max_abs'] = float(g_off.abs().max())
        del g_on, g_off
        for leg, optimise in (('step', False), ('step_opt', True)):
            on_ms, off_ms = alternated(lambda: step(on, optimise), lambda: step(off, optimise), a.warmup, a.repeats)
            res['%s_%s_native_ms' % (key, leg)] = round(on_ms, 4)
            res['%s_%s_torch_ms' % (key, leg)] = round(off_ms, 4)
            res['%s_%s_speedup' % (key, leg)] = round(off_ms / on_ms, 2)
        for side, model in (('native', on), ('torch', off)):
            on.embedding.weight.grad = off.embedding.weight.grad = None      # what the other side left is not this side's peak
            torch.cuda.synchronize()
            live = torch.cuda.memory_allocated()             # graph, walks, both tables, optimiser states
            res['%s_%s_peak_MB' % (key, side)] = round((peak_bytes(lambda: step(model, False)) - live) / 1e6, 1)
        on.embedding.weight.grad = off.embedding.weight.grad = None
        if sparse:
            launches = []
            for nm, ms in profile_launches(lambda: step(on, False)):
                floor = launch_floor(nm, n, a.emb, n_nodes, touched, rows) / HBM_BYTES_PER_S * 1e3
                launches.append([nm, round(ms, 4), round(floor, 4), round(ms / floor, 1) if floor > 0 else None])
            res['native_launch_ms_floor_ms_ratio'] = launches
        del on, off, opts
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
