"""Digest of everything the schedule host code (csrc/model.hip, csrc/model_bwd.hip) decides, for comparing two builds of
libpeahip.so: run once per library (PEA_LIB selects it) and diff the two outputs.

    PEA_LIB=/path/to/libpeahip.so python profiles/tools/schedule_digest.py > digest.txt

Per case it prints the schedule's sizes and statistics (doubles as hex floats), the pea_model_describe vector, sha256 of
every output of the forward-family entry points and of one backward_conv_stack (dense and batch-sparse), and the launch
log of each call: name, algorithmic bytes, gathered bytes and table bytes per launch, in order.  Sharded cases (world 3,
rank 0, collectives skipped: ShardLayout.dry) print launch logs only; their values are pinned by tests/test_gpu_sharded.py.
The last cases are there for the gathers: gather_paths for csrc/agg.hip (the fat-lane kernels (PEA_FAT=1), lane width 64, heads
of 16 columns and the per-edge weighted sum), backward_paths for csrc/agg_bwd.hip (hub rows and their merges at PEA_CHUNK=64, row
flags on every node, flagged last layers of lane width 4, 16 and 64, the flagged linear pass of a two-step SAGE); each fails if
the launch log does not show the kernel it is there for.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import build_model, random_hin, random_state_dict  # noqa: E402
from graph_recsys_benchmark_amd import _lib  # noqa: E402
from graph_recsys_benchmark_amd.autograd import backward_conv_stack  # noqa: E402

N, BLOCKS, REL = random_hin(21, n_user=3000, n_item=900, n_attr=50, e_u2i=40000, e_attr=2500)
U2I, A2I = REL['u2i'], REL['a2i']


def flip(e):
    return np.ascontiguousarray(e[::-1])


MIXED = ([[U2I, flip(U2I)], [flip(U2I), U2I], [A2I, flip(U2I)], [flip(A2I), A2I, flip(U2I)], [A2I]], [2, 2, 2, 3, 1])
MIXED_HEADS = (MIXED[0][:4], [2, 2, 2, 3])
TWO = ([[U2I, flip(U2I)], [flip(U2I), U2I], [A2I, flip(U2I)], [A2I, flip(U2I)], [flip(A2I), A2I]], [2] * 5)


def many(n):
    """n two-step channels over n distinct relation pairs: more groups in a level than one aggregation launch takes."""
    subs = [np.ascontiguousarray(U2I[:, 500 * k:]) for k in range(n)]
    return [[s, flip(s)] for s in subs], [2] * n


def sha(t):
    return 'none' if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


SEEN = []   # every launch name logged so far (gather_paths checks that a case reached the kernel it is there for)


def launch_log(tag):
    lib = _lib.load()
    torch.cuda.synchronize()
    cap = 1 << 13
    names = C.create_string_buffer(cap * 32)
    ms, units, gathered, table = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    cnt = C.c_int()
    _lib.check(lib.pea_profile_read_ex(cap, names, ms, units, gathered, table, C.byref(cnt)))
    for i in range(cnt.value):
        name = names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode()
        SEEN.append(name)
        print('%s launch %d %s %s %s %s' % (tag, i, name, units[i].hex(), gathered[i].hex(), table[i].hex()))


def logged(tag, fn):
    """fn() with the launch log on; prints the log, returns fn's result."""
    lib = _lib.load()
    lib.pea_profile_enable(1)
    try:
        with torch.no_grad():
            out = fn()
    finally:
        torch.cuda.synchronize()
        lib.pea_profile_enable(0)
    launch_log(tag)
    return out


def describe(tag, eng):
    lib = _lib.load()
    print('%s workspace_bytes %d' % (tag, eng.workspace_bytes))
    print('%s stats %d %s compulsory %s' % (tag, eng.messages, eng.algorithmic_bytes.hex(), eng.compulsory_bytes.hex()))
    need = C.c_int()
    _lib.check(lib.pea_model_describe(eng._h, None, 0, C.byref(need)))
    buf = (C.c_int64 * need.value)()
    _lib.check(lib.pea_model_describe(eng._h, buf, need.value, C.byref(need)))
    print('%s describe %s' % (tag, ' '.join(str(v) for v in buf)))


def make(kind, edges, steps, emb, hid, rep, heads, aggr, deg):
    model = build_model(kind, N, edges, steps, emb, hid, rep, heads=heads, channel_aggr=aggr, gcn_deg_from=deg)
    model.load_state_dict(random_state_dict(model, 9, scale=0.2))
    model.eval()
    return model, model._layer_params(), model.x.detach(), getattr(model, 'att', None)


def batch_ids():
    rng = np.random.default_rng(4)
    (u0, u1), (i0, i1) = BLOCKS['u'], BLOCKS['i']
    ids = np.unique(np.concatenate([rng.integers(u0, u1, 256), rng.integers(i0, i1, 512)]))
    return torch.from_numpy(ids.astype(np.int64)).cuda()


def backward_digest(tag, eng, lp, x, sparse, ids=None):
    """One backward_conv_stack after a training forward: dense d_stack, or the rows `ids` only (default: a batch's) with their
    flags set."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    d_stack = (torch.randn((N, eng.P, eng.repr_dim), generator=g) * 0.1).cuda()
    mask = None
    if sparse:
        ids = batch_ids() if ids is None else ids
        keep = torch.zeros(N, dtype=torch.bool, device='cuda').index_fill_(0, ids, True)
        d_stack = d_stack * keep.view(-1, 1, 1)
        mask = keep.to(torch.uint8)
        _lib.check(lib.pea_model_set_active_rows(eng._h, _lib.ptr(mask)))
    os.environ['PEA_SPARSE_BWD'] = '1' if sparse else '0'
    try:
        dx, grads = logged(tag, lambda: backward_conv_stack(eng, d_stack, x, lp, active_ids=ids, batch_flags=mask))
    finally:
        os.environ.pop('PEA_SPARSE_BWD')
        if sparse:
            _lib.check(lib.pea_model_set_active_rows(eng._h, None))
    print('%s dx %s' % (tag, sha(dx)))
    for li, gl in enumerate(grads):
        for q, t in enumerate(gl):
            print('%s grad %d.%d %s' % (tag, li, q, sha(t)))


def inference(tag, args):
    model, lp, x, att = make(*args)
    eng = model._get_engine()
    describe(tag, eng)
    out, stack = logged(tag + ' forward', lambda: eng.forward(lp, x, att, want_stack=True))
    print('%s forward %s %s' % (tag, sha(out), sha(stack)))
    print('%s masked1 %s' % (tag, sha(logged(tag + ' masked1', lambda: eng.forward(lp, x, att, masked=1)))))
    tables, weights = logged(tag + ' ablate', lambda: eng.forward_ablate(lp, x, att, want_att=True))
    print('%s ablate %s %s' % (tag, sha(tables), sha(weights)))


def training(tag, args, fused2_train, every_node=False):
    os.environ['PEA_FUSED2_TRAIN'] = str(fused2_train)
    try:
        model, lp, x, att = make(*args)
        eng = model._get_engine(train=True)
    finally:
        os.environ.pop('PEA_FUSED2_TRAIN')
    tag = '%s train%d' % (tag, fused2_train)
    describe(tag, eng)
    for sparse in (False, True):
        t = '%s %s' % (tag, 'sparse' if sparse else 'dense')
        out, stack = logged(t + ' forward', lambda: eng.forward(lp, x, att, want_stack=True, train=True))
        print('%s forward %s %s' % (t, sha(out), sha(stack)))
        backward_digest(t + ' backward', eng, lp, x, sparse)
    if every_node:      # flags on every row: the survivor queue of the S pass fills with every batch of 64 edges
        t = tag + ' allrows'
        out, stack = logged(t + ' forward', lambda: eng.forward(lp, x, att, want_stack=True, train=True))
        print('%s forward %s %s' % (t, sha(out), sha(stack)))
        backward_digest(t + ' backward', eng, lp, x, True, ids=torch.arange(N, device='cuda'))


def sharded(tag, args):
    """World 3, rank 0, collectives skipped: the launch logs of the inference forward (both parts per stage) and of the
    stage-wise training forward and backward."""
    model, lp, x, att = make(*args)
    model.shard(0, 3, tile=64)
    eng = model._get_engine()
    eng.plan.layout.dry = True
    describe(tag, eng)
    logged(tag + ' forward', lambda: eng.forward(lp, x, att, want_stack=True))
    teng = model._get_engine(train=True)
    describe(tag + ' train', teng)
    logged(tag + ' train forward', lambda: teng.forward(lp, x, att, want_stack=True, train=True, gather=False))
    g = torch.Generator().manual_seed(5)
    d_stack = (torch.randn((N, teng.P, teng.repr_dim), generator=g) * 0.1).cuda()
    logged(tag + ' train backward', lambda: backward_conv_stack(teng, d_stack, x, lp))


def single_convs():
    from graph_recsys_benchmark_amd.nn import GATConv, GCNConv, SAGEConv
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((N, 32), generator=g) * 0.2).cuda()
    ei = torch.from_numpy(U2I).cuda()
    for name, conv in (('gat', GATConv(32, 24, heads=2)), ('gcn', GCNConv(32, 24)), ('sage', SAGEConv(32, 24))):
        conv = conv.cuda()
        with torch.no_grad():
            for p in conv.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * 0.2).cuda())
        for relu in (False, True):
            tag = 'conv %s relu%d' % (name, int(relu))
            print('%s %s' % (tag, sha(logged(tag, lambda: conv(x, ei, relu=relu)))))


def reached(tag, since, part):
    if not any(part in name for name in SEEN[since:]):
        raise RuntimeError('%s: no launch named *%s*' % (tag, part))


def gather_paths():
    """The forward gather's remaining paths (csrc/agg.hip): fat lanes, lane width 64, heads of 16 columns, per-edge weights."""
    heads2 = lambda hid: ('gat', MIXED_HEADS[0], MIXED_HEADS[1], 32, hid, 16, 2, 'att', 'row')
    os.environ['PEA_FAT'] = '1'
    try:
        for kind in ('gat', 'gcn', 'sage'):
            for emb in (64, 128):
                tag, since = '%s fat twostep%d' % (kind, emb), len(SEEN)
                inference(tag, (kind, TWO[0], TWO[1], emb, 64, 16, 1, 'att', 'row'))
                reached(tag, since, 'agg_long_fat_')
        since = len(SEEN)
        inference('gat fat heads2x64', heads2(64))
        reached('gat fat heads2x64', since, 'agg_long_fat_')
    finally:
        os.environ.pop('PEA_FAT')
    for kind in ('gat', 'gcn', 'sage'):
        tag, since = '%s wide256' % kind, len(SEEN)
        inference(tag, (kind, MIXED[0], MIXED[1], 256, 256, 16, 1, 'att', 'row'))
        reached(tag, since, '_g64_')
    inference('gat heads2x16', heads2(16))
    from graph_recsys_benchmark_amd.nn.kg_conv import weighted_aggregate
    g = torch.Generator().manual_seed(7)
    ei = torch.from_numpy(U2I).cuda()
    w = torch.rand(U2I.shape[1], generator=g).cuda()
    for width in (16, 64, 260):   # 260: two groups, 256 + 4 columns
        x = (torch.randn((N, width), generator=g) * 0.2).cuda()
        tag, since = 'wsum %d' % width, len(SEEN)
        print('%s %s' % (tag, sha(logged(tag, lambda: weighted_aggregate(x, ei, w)))))
        reached(tag, since, '_wsum')


def backward_paths():
    """The backward gathers' remaining paths (csrc/agg_bwd.hip)."""
    level_wise = lambda kind, rep: (kind, MIXED[0], MIXED[1], 32, 24, rep, 1, 'att', 'row')
    os.environ['PEA_CHUNK'] = '64'      # read when a plan is made: hub rows of many chunks, dense and flagged
    try:
        for kind, parts in (('gat', ('gat_bwd_dst_merge', 'gat_bwd_src_merge', 'gat_bwd_src_g4_batch')),
                            ('gcn', ('sum_bwd_src_merge', 'sum_bwd_src_g4_batch'))):
            tag, since = '%s chunk64 levelwise' % kind, len(SEEN)
            training(tag, level_wise(kind, 16), 1, every_node=True)
            for part in parts:
                reached(tag, since, part)
    finally:
        os.environ.pop('PEA_CHUNK')
    tag, since = 'gat allrows levelwise', len(SEEN)
    training(tag, level_wise('gat', 16), 1, every_node=True)
    reached(tag, since, 'gat_bwd_src_g4_batch')
    for rep, G in ((64, 16), (256, 64)):        # (16 columns, lane width 4: the cases above)
        for kind, part in (('gat', 'gat_bwd_src_g%d_batch'), ('gcn', 'sum_bwd_src_g%d_batch')):
            tag, since = '%s last%d levelwise' % (kind, rep), len(SEEN)
            training(tag, level_wise(kind, rep), 1, every_node=True)
            reached(tag, since, part % G)
            if kind == 'gat':
                reached(tag, since, 'gat_bwd_dst_g%d_batch' % G)
    tag, since = 'sage flags twostep64', len(SEEN)
    training(tag, ('sage', TWO[0], TWO[1], 64, 64, 16, 1, 'att', 'row'), 1, every_node=True)
    reached(tag, since, 'sum_bwd_src_g')
    if not any(n.startswith('sum_bwd_src_g') and n.endswith('_batch') for n in SEEN[since:]):
        raise RuntimeError('%s: no launch named sum_bwd_src_g*_batch' % tag)


def flagged_heads():
    """Row flags on a layer of several heads: the one-channel, one-step engine of nn.conv (its last layer is heads * out wide),
    backward_conv_stack called with the flags directly.  (heads, out): lane width and head class of the flagged kernels."""
    from graph_recsys_benchmark_amd.engine import PEAEngine
    from graph_recsys_benchmark_amd.nn import conv
    ei = torch.from_numpy(U2I).cuda()
    for chunk in (512, 64):
        os.environ['PEA_CHUNK'] = str(chunk)
        try:
            plan = conv._train_plan_for(ei.clone(), N, True)
        finally:
            os.environ.pop('PEA_CHUNK')
        for heads, out in ((2, 8), (2, 16), (4, 16), (2, 32), (3, 12)):
            width = heads * out
            G = next(g for g in (4, 8, 16, 32, 64) if 4 * g >= width)
            eng = PEAEngine(plan, 'gat', [1], 32, out, out, heads=heads, channel_aggr='mean', enable_backward=True)
            g = torch.Generator().manual_seed(100 * heads + out)
            rand = lambda *shape: (torch.randn(shape, generator=g) * 0.2).cuda()
            x, lp = rand(N, 32), [(rand(width, 32), rand(1, heads, out), rand(1, heads, out), rand(width))]
            scratch = torch.empty((N, out), dtype=torch.float32, device='cuda')
            for name, ids in (('batch', batch_ids()), ('allrows', torch.arange(N, device='cuda'))):
                tag, since = 'flagged heads%dx%d chunk%d %s' % (heads, out, chunk, name), len(SEEN)
                logged(tag + ' forward', lambda: eng.forward(lp, x, att=None, train=True, out=scratch))
                keep = torch.zeros(N, dtype=torch.bool, device='cuda').index_fill_(0, ids, True)
                d_out = rand(N, 1, width) * keep.view(-1, 1, 1)
                mask = keep.to(torch.uint8)
                _lib.check(_lib.load().pea_model_set_active_rows(eng._h, _lib.ptr(mask)))
                try:
                    dx, grads = logged(tag, lambda: backward_conv_stack(eng, d_out, x, lp, active_ids=ids, batch_flags=mask))
                finally:
                    _lib.check(_lib.load().pea_model_set_active_rows(eng._h, None))
                print('%s dx %s %s' % (tag, sha(dx), ' '.join(sha(t) for t in grads[0])))
                for part in ('gat_bwd_dst_g%d_batch' % G, 'gat_bwd_src_g%d_batch' % G):
                    reached(tag, since, part)


def main():
    torch.cuda.set_device(0)
    print('library %s' % _lib.load().pea_version().decode())
    for kind in ('gat', 'gcn', 'sage'):
        level_wise = (kind, MIXED[0], MIXED[1], 32, 24, 16, 1, 'att', 'row')
        two_step = (kind, TWO[0], TWO[1], 64, 64, 16, 1, 'att', 'row')
        cases = [('levelwise', level_wise, (1,)),
                 ('twostep64', two_step, (0, 1)),
                 ('twostep128', (kind, TWO[0], TWO[1], 128, 64, 16, 1, 'att', 'row'), (0, 1)),
                 ('many33x32', (kind,) + many(33) + (32, 32, 16, 1, 'att', 'row'), (1,)),
                 ('many20x64', (kind,) + many(20) + (64, 64, 16, 1, 'att', 'row'), (0, 1)),
                 ('mean', (kind, TWO[0], TWO[1], 64, 64, 16, 1, 'mean', 'row'), (1,)),
                 ('mean levelwise', (kind, MIXED[0], MIXED[1], 32, 24, 16, 1, 'mean', 'row'), (1,))]
        if kind == 'gat':
            cases.append(('heads2', (kind, MIXED_HEADS[0], MIXED_HEADS[1], 32, 24, 16, 2, 'att', 'row'), (1,)))
        if kind == 'gcn':
            cases.append(('col levelwise', (kind, MIXED[0], MIXED[1], 32, 24, 16, 1, 'att', 'col'), (1,)))
            cases.append(('col twostep64', (kind, TWO[0], TWO[1], 64, 64, 16, 1, 'att', 'col'), (0, 1)))
        for name, args, modes in cases:
            tag = '%s %s' % (kind, name)
            inference(tag, args)
            for mode in modes:
                training(tag, args, mode)
        # LDS-staged hot sources (off by default; the graph's relations are below the default size threshold)
        os.environ.update(PEA_HOT='1', PEA_HOT_MIN_EDGES='1000')
        try:
            inference('%s hot levelwise' % kind, level_wise)
            inference('%s hot twostep64' % kind, two_step)
        finally:
            os.environ.pop('PEA_HOT')
            os.environ.pop('PEA_HOT_MIN_EDGES')
        sharded('%s sharded levelwise' % kind, level_wise)
        sharded('%s sharded twostep64' % kind, two_step)
        if kind == 'gat':
            sharded('gat sharded heads2', (kind, MIXED_HEADS[0], MIXED_HEADS[1], 32, 24, 16, 2, 'att', 'row'))
    single_convs()
    gather_paths()
    backward_paths()
    flagged_heads()
    print('done')


if __name__ == '__main__':
    main()
