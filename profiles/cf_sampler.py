"""Measurement of the on-device CF epoch sampler (csrc/cf_sampler.hip) on the user2item pairs of the ml25m_shaped preset, and of
entity-aware PEAGAT training fed by it.

    timeout -k 10 1100 python profiles/cf_sampler.py [--preset ml25m_shaped] [--repeats 10] [--steps 200] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/cf_sampler.py --trace 3

Legs, for k = 1 and 4 negatives per positive (4 is the reference's default: 99.2 M rows):
  native   one pea_cf_sample launch for the BPR rows, the nine-column entity-aware rows, the BCE rows and the BPR rows with
           'unseen' negatives, each with the shuffle off and on, into a table allocated once.  HIP events around the call alone
           (no host read inside), median of --repeats after --warmup.
  torch    the nine-column shuffled table composed on the GPU by torch: the launch of device_negative_sampling(shuffle=False)
           for the three columns (pea_sample_negatives on the positives both sides keep on the device: no copy of the pairs and
           no host read inside the timed call), CSR gathers with torch.rand draws and a bucketize for the six entity columns,
           randperm and an index.  The yardstick; alternated call by call with the native launch it is compared to.
  host     utils.entity_aware_row, the bit-exact Python route, on the first --host-rows rows of a table: wall clock, reported
           per row and as measured, not scaled up to the table.
  train    --steps PEAGAT steps at batch 4096 through solvers.cf_epoch on the device table, entity_aware=True on its nine-column
           table against entity_aware=False on the three-column one, wall clock between synchronisations.
Peak memory of a leg is torch.cuda.max_memory_allocated over one call minus what was allocated before it.  The byte floor of
a launch is 16 bytes read and 72 (nine columns) or 24 (three) written per row at 8 TB/s.  --trace K runs K native launches of
every variant and nothing else, for a kernel trace taken from outside.  One JSON line (also written to --out).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kg_sampler import HBM_BYTES_PER_S, SEED, extra_peak_bytes, median_ms, wall_ms      # noqa: E402
from kg_train import alternated                                                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='ml25m_shaped')
    ap.add_argument('--scale', type=float, default=1.0)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-rows', type=int, default=100000)
    ap.add_argument('--trace', type=int, default=0, help='run this many native launches of every variant and nothing else')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from graph_recsys_benchmark_amd import _lib, models, solvers
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, entity_aware_row, entity_store, update_pea_graph_input
    torch.cuda.set_device(0)
    lib = _lib.require_device()
    note = lambda text: print(text, file=sys.stderr, flush=True)
    d = SyntheticHIN(a.preset, scale=a.scale)
    d.entity_lists()
    d.cf_loss_type, d.sampling_strategy, d.entity_aware, d.num_negative_samples = 'BPR', 'random', True, 4
    store = entity_store(d, 'cuda')
    pos = torch.as_tensor(d.edge_index_nps['user2item']).to(device='cuda', dtype=torch.int64)
    pos_u, pos_i = pos[0].contiguous(), pos[1].contiguous()
    del pos
    n_pos = pos_u.numel()
    i_lo, n_items, u_lo, n_users = d.type_accs['iid'], d.num_iids, d.type_accs['uid'], d.num_uids
    keys = torch.unique(pos_u * n_items + (pos_i - i_lo))
    note('store built: %d positives, %d / %d list entries, %d blocks' % (n_pos, store.nnz_i, store.nnz_u, store.num_blocks))
    buf = torch.empty(n_pos * 4 * 9, dtype=torch.int64, device='cuda')          # the largest table: nine columns at k = 4
    counts = torch.zeros(2, dtype=torch.int32, device='cuda')
    epoch = [0]
    ent_tables = [_lib.ptr(store.item_ptr), _lib.ptr(store.item_ent), store.nnz_i, _lib.ptr(store.user_ptr), _lib.ptr(store.user_ent),
                  store.nnz_u, store.num_blocks, _lib.ptr(store.block_lo), _lib.ptr(store.block_n)]
    no_tables = [None, None, 0, None, None, 0, 0, None, None]
    # form -> (mode, entity tables, key table, rows per positive as a function of k, row width)
    forms = {'bpr': (_lib.CF_BPR, False, False, lambda k: k, 3), 'bpr_entity': (_lib.CF_BPR, True, False, lambda k: k, 9),
             'bce': (_lib.CF_BCE, False, False, lambda k: k + 1, 3), 'bpr_unseen': (_lib.CF_BPR, False, True, lambda k: k, 3)}

    def native(form, k, shuffle):
        mode, ent, unseen, rows_of, width = forms[form]
        n_rows = n_pos * rows_of(k)
        out = buf[:n_rows * width].view(n_rows, width)
        epoch[0] += 1
        _lib.check(lib.pea_cf_sample(n_pos, k, mode, _lib.ptr(pos_u), _lib.ptr(pos_i), i_lo, n_items, u_lo, n_users,
                                     _lib.ptr(keys) if unseen else None, keys.numel() if unseen else 0,
                                     *(ent_tables if ent else no_tables), SEED, epoch[0], shuffle, _lib.ptr(out), width,
                                     _lib.ptr(counts), _lib.ptr(counts[1:]), _lib.current_stream()))
        return out

    variants = [(form, k, sh) for k in (1, 4) for form in forms for sh in (0, 1)]
    if a.trace:
        for v in variants:
            for _ in range(a.trace):
                native(*v)
        torch.cuda.synchronize()
        return

    res = {'preset': a.preset, 'scale': a.scale, 'positives': n_pos, 'item_list_entries': store.nnz_i, 'user_list_entries': store.nnz_u,
           'blocks': store.num_blocks, 'key_table_MB': round(keys.numel() * 8 / 1e6, 1),
           'timing': 'HIP events around the calls, median of %d after %d warm-up; torch and native alternated; host and train legs: '
                     'wall clock between synchronisations' % (a.repeats, a.warmup)}

    # ---- the native variants
    for form, k, sh in variants:
        mode, ent, unseen, rows_of, width = forms[form]
        n_rows = n_pos * rows_of(k)
        floor_ms = (8.0 * width + 16.0) * n_rows / HBM_BYTES_PER_S * 1e3
        name = '%s_k%d_%s' % (form, k, 'shuffled' if sh else 'ordered')
        t = median_ms(lambda: native(form, k, sh), a.warmup, a.repeats)
        ex, bad = counts.tolist()
        res['native_%s' % name] = {'rows': n_rows, 'ms': round(t, 4), 'byte_floor_ms': round(floor_ms, 4), 'x_floor': round(t / floor_ms, 2),
                                   'table_MB': round(n_rows * width * 8 / 1e6, 1), 'exhausted': ex, 'bad_rows': bad}
        note('%s: %.3f ms (%.2fx floor)' % (name, t, t / floor_ms))

    # ---- the torch composition of the nine-column shuffled table
    def composed(k):
        epoch[0] += 1
        n = n_pos * k
        t = torch.empty((n, 3), dtype=torch.int64, device='cuda')
        _lib.check(lib.pea_sample_negatives(n_pos, k, _lib.ptr(pos_u), _lib.ptr(pos_i), i_lo, n_items, None, 0, SEED, epoch[0],
                                            _lib.ptr(t), 3, _lib.ptr(counts), _lib.current_stream()))

        def triple(ptr, ent, own):
            lo = ptr[own]
            length = ptr[own + 1] - lo
            has = length > 0
            pick = lo + torch.minimum((torch.rand(n, device='cuda', dtype=torch.float64) * length).long(), (length - 1).clamp_(min=0))
            e = ent[torch.where(has, pick, torch.zeros_like(pick))]
            blk = torch.bucketize(e, store.block_lo, right=True) - 1
            e_neg = store.block_lo[blk] + (torch.rand(n, device='cuda', dtype=torch.float64) * store.block_n[blk]).long()
            zero = torch.zeros_like(e)
            return [torch.where(has, e, zero), torch.where(has, e_neg, zero), has.long()]

        cols = triple(store.item_ptr, store.item_ent, t[:, 1] - i_lo) + triple(store.user_ptr, store.user_ent, t[:, 0] - u_lo)
        table = torch.cat([t, torch.stack(cols, dim=1)], dim=1)
        return table[torch.randperm(n, device='cuda')]

    for k in (1, 4):
        nat_ms, torch_ms = alternated(lambda: native('bpr_entity', k, 1), lambda: composed(k), a.warmup, a.repeats)
        res['torch_bpr_entity_k%d_shuffled' % k] = {
            'ms': round(torch_ms, 3), 'native_alternated_ms': round(nat_ms, 4), 'native_over_torch': round(torch_ms / nat_ms, 2),
            'peak_MB': round(extra_peak_bytes(lambda: composed(k)) / 1e6, 1),
            'native_peak_MB': round(n_pos * k * 72 / 1e6, 1)}                   # the output table: the launch allocates nothing
        note('k=%d: torch %.2f ms, native %.3f ms' % (k, torch_ms, nat_ms))

    # ---- the host route on a sample of rows
    rows3 = native('bpr', 4, 0)[:a.host_rows].cpu()
    t0 = time.perf_counter()
    for r in range(rows3.shape[0]):
        entity_aware_row(d, rows3[r])
    host_s = time.perf_counter() - t0
    res['host_entity_aware_row'] = {'rows': int(rows3.shape[0]), 'seconds': round(host_s, 3),
                                    'us_per_row': round(host_s / max(rows3.shape[0], 1) * 1e6, 2)}
    note('host: %.2f s for %d rows' % (host_s, rows3.shape[0]))

    # ---- PEAGAT training through cf_epoch, entity-aware against plain
    dataset_args = d.dataset_args()
    train_args = {'device': torch.device('cuda', 0), 'num_metapaths': d.spec['num_metapaths']}

    class Model(models.PEAGATRecsysModel):
        def update_graph_input(self, dataset):
            return update_pea_graph_input(dataset_args, train_args, d)

    def fresh(entity_aware):
        torch.manual_seed(2020)
        model = Model(**d.model_args(kind='gat', entity_aware=entity_aware)).cuda()
        return model.train(), torch.optim.Adam(model.parameters(), lr=1e-3)

    need = (a.steps + 5) * a.batch
    wide = native('bpr_entity', 4, 1)[:need].clone()
    narrow = wide[:, :3].contiguous()
    res['train_steps'], res['train_batch'] = a.steps, a.batch
    for name, table, flag in (('entity_aware', wide, True), ('plain', narrow, False)):
        model, opt = fresh(flag)
        solvers.cf_epoch(model, opt, table, a.batch, max_steps=5)              # warm-up: plan, allocator, lazy kernels
        ms, loss = wall_ms(lambda: solvers.cf_epoch(model, opt, table[5 * a.batch:], a.batch, max_steps=a.steps))
        res['train_%s_ms_per_step' % name] = round(ms / a.steps, 4)
        res['train_%s_mean_loss' % name] = round(loss, 3)
        note('train %s: %.3f ms per step' % (name, ms / a.steps))
        del model, opt
    res['train_entity_aware_over_plain'] = round(res['train_entity_aware_ms_per_step'] / res['train_plain_ms_per_step'], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
