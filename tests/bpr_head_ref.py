"""The BPR training head (csrc/bpr_train.hip) and the row scatter (csrc/rows_scatter.hip) restated without a GPU, with the case
lists of tests/test_gpu_bpr_head_matrix.py.  tests/test_bpr_head_cpu.py checks all of it on the CPU.  A helper: not collected.

head_reference     the head in torch at a chosen dtype (reference models/base.py:193-203, :208-214, :46-48): the loss, the autograd
                   gradients of every input, and the raw outputs in the layout bpr_train.hip documents (zx, dhx, dsc, grad_rows)
gate_margin        the triples whose relu gate float32 may decide otherwise than float64
HEAD_CELLS         the matrix, one row per cell, the id names what the cell is there for
scatter_reference  pea_rows_scatter_sum as a sequential float32 loop over the positions, with a float64 total
scatter_ids        id vectors with prescribed run lengths, shared LDS buckets and skipped ids"""
import numpy as np
import torch

import helpers

KEYS = ('picked', 'att', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b')
RAW = ('zx', 'dhx', 'dsc', 'grad_rows')
PER_TRIPLE = {'dhx': 2, 'dsc': 3, 'grad_rows': 3}        # rows per triple of the outputs a gate flip changes
K_TB = 64                                                # bpr_train.hip: kTB, triples per workgroup
GATE_ULPS = 64.0
EXCLUDE_SHARE = 0.005                                    # a cell may exclude 0.5 % of its triples, one triple where B < 200


def ceil4(v):
    return (v + 3) // 4 * 4


def head_supported(p, r):
    """pea_bpr_train_supported, written down by hand"""
    return p > 0 and r > 0 and r % 4 == 0 and r <= 32 and p <= 64 and p * r <= 1024


def head_inputs(b, p, r, mode, seed):
    """float32 CPU tensors with the magnitudes of tests/test_gpu_bpr_train.py: picked 0.7, att 0.5, fc1 0.4 / 0.1, fc2 0.5 / 0.1 randn"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s
    return dict(picked=mk(3 * b, p, r, s=0.7), att=mk(1, p, r, s=0.5) if mode == 'att' else None, fc1_w=mk(r, 2 * r, s=0.4),
                fc1_b=mk(r, s=0.1), fc2_w=mk(1, r, s=0.5), fc2_b=mk(1, s=0.1))


def _forward(x, att, fc1_w, fc1_b, fc2_w, fc2_b):
    """(channel weights a [3B, P] or None, fused [3B, R], z [B, 2, 2R], h [B, 2, R] before the relu, score gap d [B])"""
    n3, p, r = x.shape
    if att is None:
        a, fused = None, x.mean(dim=1)
    else:
        a = torch.softmax(torch.sum(x * att.view(1, p, r), dim=-1), dim=-1)
        fused = torch.sum(x * a.unsqueeze(-1), dim=1)
    rows = fused.view(-1, 3, r)
    z = torch.stack([torch.cat([rows[:, 0], rows[:, 1 + e]], dim=-1) for e in range(2)], dim=1)
    h = z @ fc1_w.t() + fc1_b
    s = (torch.relu(h) @ fc2_w.t() + fc2_b).squeeze(-1)
    return a, fused, z, h, s[:, 0] - s[:, 1]


def head_reference(picked, att, fc1_w, fc1_b, fc2_w, fc2_b, dtype, wrong=None):
    """dict of numpy arrays in `dtype` (float32: the peer, float64: the truth):

        loss [1]                        -sum_b log(sigmoid(pos_b - neg_b)), unclamped
        d_<input>                       torch autograd's gradient of the loss for every input that is not None
        gap [B]                         pos_b - neg_b
        zx  [2B, 3R + 4]   row 2b + e = [fused user | fused item_e | relu(hidden_e) | 1 0 0 0]
        dhx [2B, R + 4]    row 2b + e = [(hidden_e > 0) ds_e fc2_w | ds_e | 0 0 0],  ds_0 = g = -(1 - sigmoid(gap)), ds_1 = -g
        dsc [3B, ceil4(P)] row 3b + j = a_p (dF_j . S_p - sum_q a_q dF_j . S_q), 0 for p >= P   (None without att)
        grad_rows [3B, P R]             a_p dF_j + dsc_p att_p  ('mean': dF_j / P)

    wrong: a defect planted in the raw outputs, for tests/test_bpr_head_cpu.py to show that the comparisons notice it:
    'ds_sign' (ds_1 = +g), 'dsc_no_sum' (dsc without its sum term), 'dsc_rotated' (dsc[:, p] taken from channel p + 1),
    'zx_swapped' (item before user), 'dhx_pad' (the first pad column of dhx repeats ds)."""
    leaves = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v is not None else None)
              for k, v in zip(KEYS, (picked, att, fc1_w, fc1_b, fc2_w, fc2_b))}
    a, fused, z, h, d = _forward(*[leaves[k] for k in KEYS])
    loss = -d.sigmoid().log().sum()
    loss.backward()
    out = {'loss': loss.detach().reshape(1), 'gap': d.detach()}
    out.update({'d_' + k: (v.grad if v is not None else None) for k, v in leaves.items()})
    with torch.no_grad():
        x, w1, w2 = leaves['picked'], leaves['fc1_w'], leaves['fc2_w']
        n3, p, r = x.shape
        b = n3 // 3
        g = -(1.0 - torch.sigmoid(d))
        ds = torch.stack([g, g if wrong == 'ds_sign' else -g], dim=1)                    # [B, 2]
        dh = (h > 0).to(dtype) * ds.unsqueeze(-1) * w2.view(1, 1, r)                     # [B, 2, R]
        zeros = torch.zeros((b, 2, 3), dtype=dtype)
        halves = (z[..., r:], z[..., :r]) if wrong == 'zx_swapped' else (z[..., :r], z[..., r:])
        out['zx'] = torch.cat(halves + (torch.relu(h), torch.ones((b, 2, 1), dtype=dtype), zeros), dim=-1).reshape(2 * b, 3 * r + 4)
        pad = ds.unsqueeze(-1) * torch.tensor([1.0, 0.0, 0.0], dtype=dtype) if wrong == 'dhx_pad' else zeros
        out['dhx'] = torch.cat([dh, ds.unsqueeze(-1), pad], dim=-1).reshape(2 * b, r + 4)
        dz = dh @ w1                                                                     # [B, 2, 2R]
        df = torch.stack([dz[:, 0, :r] + dz[:, 1, :r], dz[:, 0, r:], dz[:, 1, r:]], dim=1).reshape(n3, 1, r)
        if a is None:
            out['dsc'] = None
            out['grad_rows'] = (df / p).expand(n3, p, r).reshape(n3, p * r)
        else:
            dot = (df * x).sum(-1)                                                       # [3B, P]
            dsc = a * (dot - (a * dot).sum(-1, keepdim=True))
            shown = a * dot if wrong == 'dsc_no_sum' else torch.roll(dsc, -1, dims=1) if wrong == 'dsc_rotated' else dsc
            out['dsc'] = torch.cat([shown, torch.zeros((n3, ceil4(p) - p), dtype=dtype)], dim=1)
            out['grad_rows'] = (a.unsqueeze(-1) * df + dsc.unsqueeze(-1) * leaves['att'].view(1, p, r)).reshape(n3, p * r)
    return {k: (v.detach().numpy() if v is not None else None) for k, v in out.items()}


def gate_margin(picked, att, fc1_w, fc1_b, fc2_w, fc2_b, ulps=GATE_ULPS):
    """bool [B]: the triples with a float64 hidden pre-activation h_k (of either score) so close to the relu gate that float32 may
    see its sign otherwise:  |h_k| <= ulps 2^-24 (|z| . |w1_k| + |b1_k|).  A flip changes a whole dhx row and with it the
    triple's grad_rows and dsc rows, so these triples leave the comparisons of those three outputs (not of zx or the loss)."""
    t = [v.detach().double() if v is not None else None for v in (picked, att, fc1_w, fc1_b, fc2_w, fc2_b)]
    _, _, z, h, _ = _forward(*t)
    bound = ulps * helpers.EPS32 * (z.abs() @ t[2].abs().t() + t[3].abs())
    return (h.abs() <= bound).any(dim=-1).any(dim=-1).numpy()


def exclusion_cap(b):
    """triples a cell of b triples may exclude"""
    return 1 if b < 200 else int(EXCLUDE_SHARE * b)


# ------------------------------------------------------------------------------------------------------------
# HEAD_CELLS: (id, B, P, R, mode, seed).  bpr_train_kernel<R4> is instantiated per R4 = R / 4 = 1..8 and branches on att;
# P: 1 = a softmax of one term, 3 = P4 of 4 with one pad column of dsc, 4 = no pad, 9 = the headline count.  One B per
# (R4, P), the same for both modes, rotated through 1, 63, 64, 65 (around kTB = 64) and 257 (five workgroups, the last with one
# triple), so that every B meets both modes and an odd R4 (test_bpr_head_cpu.py asserts it).  Then the limits P <= 64,
# P R <= 1024, R <= 32, and the route's own cap of 5461 triples (ROWS_SCATTER_MAX / 3) at the headline shape.
# Seeds: 1000 B + 10 P + R (+ 1 for 'mean') unless SEEDS names another; tests/test_bpr_head_cpu.py holds every cell to the
# exclusion cap, to at least one kept triple, and to HEAD_NEAR_ULPS.
# ------------------------------------------------------------------------------------------------------------
HEAD_BATCHES = (1, 63, 64, 65, 257)
HEAD_PS = (1, 3, 4, 9)
HEAD_P_NAMES = {1: 'one_term', 3: 'one_pad', 4: 'no_pad', 9: 'headline'}
HEAD_LIMITS = [(64, 16, 65, 'P64xR16_cols1024'), (32, 32, 63, 'P32xR32_cols1024'), (64, 4, 257, 'P64xR4_max_channels')]
HEAD_CAP = (5461, 9, 16)
MODES = ('att', 'mean')
# the formula's seed puts triple 5240 within 8 ulps of a gate.  The choice holds for head_inputs as written and torch's CPU
# generator stream: change either and test_bpr_head_cpu.py names the cells that need a seed chosen again
SEEDS = {'route_cap-mean-B5461-P9-R16': 5461096}
# the wrapper's parameter gradients sum over EVERY triple, the excluded ones too: no cell may hold a pre-activation within this
# many float32 ulps (of |z| . |w1_k| + |b1_k|) of the gate, where the kernel's own rounding (about sqrt(2R) / 2 ulps of a 2R-term
# product sum, below 1 in these units) could turn it
HEAD_NEAR_ULPS = 8.0


def _head_cells():
    cells = []

    def add(name, b, p, r, mode):
        cid = '%s-%s-B%d-P%d-R%d' % (name, mode, b, p, r)
        cells.append((cid, b, p, r, mode, SEEDS.get(cid, 1000 * b + 10 * p + r + (mode == 'mean'))))

    for r4 in range(1, 9):
        for k, p in enumerate(HEAD_PS):
            b = HEAD_BATCHES[((r4 - 1) * len(HEAD_PS) + k) % len(HEAD_BATCHES)]
            for mode in MODES:
                add('R4_%d-%s' % (r4, HEAD_P_NAMES[p]), b, p, 4 * r4, mode)
    for p, r, b, name in HEAD_LIMITS:
        for mode in MODES:
            add('limit_' + name, b, p, r, mode)
    for mode in MODES:
        add('route_cap', HEAD_CAP[0], HEAD_CAP[1], HEAD_CAP[2], mode)
    return cells


HEAD_CELLS = _head_cells()
HEAD_IDS = [c[0] for c in HEAD_CELLS]
# the cells of test_fused_rows_are_the_bits_of_pea_fuse: every (R4, mode) at P = 9, and the three limit shapes
FUSE_CELLS = [c for c in HEAD_CELLS if ('headline' in c[0] or c[0].startswith('limit_'))]
_CASES = {}


def head_case(cid):
    """(inputs, float32 peer, float64 truth, flagged triples) of a cell, computed once"""
    if cid not in _CASES:
        _, b, p, r, mode, seed = HEAD_CELLS[HEAD_IDS.index(cid)]
        inp = head_inputs(b, p, r, mode, seed)
        args = [inp[k] for k in KEYS]
        _CASES[cid] = (inp, head_reference(*args, torch.float32), head_reference(*args, torch.float64), gate_margin(*args))
    return _CASES[cid]


def kept_rows(flagged, rows_per_triple):
    """bool mask over the rows of an output with `rows_per_triple` rows per triple: the rows of the triples that are not flagged"""
    return np.repeat(~np.asarray(flagged, bool), rows_per_triple)


def assert_head_close(got, peer, truth, flagged, what='', keys=RAW + ('loss',), report=None):
    """helpers.assert_fp32_close at its defaults for every output named in `keys`: dhx, dsc and grad_rows on the triples
    gate_margin keeps, everything else whole.  report: a dict that receives {key: (row ulps against float64, deciding tier)}."""
    assert int(np.sum(flagged)) <= exclusion_cap(len(flagged)), '%s: %d of %d triples excluded' % (what, int(np.sum(flagged)), len(flagged))
    for k in keys:
        if truth[k] is None:
            assert got[k] is None, k
            continue
        g, p, t = (np.asarray(a[k]) for a in (got, peer, truth))
        assert g.shape == t.shape, (what, k, g.shape, t.shape)
        if k in PER_TRIPLE:
            keep = kept_rows(flagged, PER_TRIPLE[k])
            g, p, t = g[keep], p[keep], t[keep]
        if g.size == 0:
            continue
        assert np.isfinite(g).all(), '%s: %s is not finite' % (what, k)
        if report is not None:
            report[k] = (helpers.row_ulps(g.reshape(-1, g.shape[-1]), t.reshape(-1, t.shape[-1])) if np.abs(t).max() > 0 else 0.0,
                         helpers.fp32_tier(g, p, t))
        helpers.assert_fp32_close(g, p, t, what='%s %s' % (what, k))


# ------------------------------------------------------------------------------------------------------------
# pea_rows_scatter_sum
# ------------------------------------------------------------------------------------------------------------
SCATTER_BUCKETS = 2048                                   # rows_scatter.hip: kBuckets
SCATTER_MAX = 16384                                      # rows_scatter.hip: kSortMax
SCATTER_RUNS = {1: (1, 31, 32, 33, 64, 65, 200),         # V = 1 (W <= 256): NB = 32 rows per trip of the run loop
                4: (1, 7, 8, 9, 16, 17, 100)}            # V = 4 (W > 256):  NB = 8
SCATTER_ROWS = 4200                                      # table rows of the constructed cases: past the third id of a bucket
# (P, R, n % 4): W = 4 and 256 (the last V = 1), 260 (the first V = 4), 768, 1024 (the maximum)
SCATTER_CASES = [(1, 4, 1), (16, 16, 2), (13, 20, 3), (24, 32, 1), (64, 16, 2)]
SCATTER_IDS = ['W%d_%dx%d' % (p * r, p, r) for p, r, _ in SCATTER_CASES]


def scatter_width_class(w):
    """V of scatter_runs_kernel<V>: float4 columns per lane"""
    return 1 if w <= 256 else 4


def scatter_ids(width_class, num_rows, n_mod4=1, seed=0):
    """(ids int64 [n], {run length: node}) for scatter_runs_kernel<width_class>: one node per run length of SCATTER_RUNS (NB - 1,
    NB, NB + 1, 2 NB, 2 NB + 1 and a long run), the positions of all runs interleaved by one permutation, so that a run's
    positions are not contiguous and their order matters.  Three nodes share an LDS bucket of the sort (a, a + 2048, a + 4096),
    one node is the table's last row; ids -1, num_rows and 2^40 are skipped ones.  Padded with -1 to n % 4 == n_mod4."""
    runs = SCATTER_RUNS[width_class]
    a = 37
    assert num_rows > 2 * SCATTER_BUCKETS + a + 1
    nodes = [a, num_rows - 1, a + SCATTER_BUCKETS, 5, a + 2 * SCATTER_BUCKETS, 2 * SCATTER_BUCKETS - 1, 300]
    assert len(set(nodes)) == len(runs) and max(nodes) < num_rows
    ids = [node for node, length in zip(nodes, runs) for _ in range(length)] + [-1, num_rows, 2 ** 40, -1, num_rows + 7]
    while len(ids) % 4 != n_mod4:
        ids.append(-1)
    ids = np.asarray(ids, np.int64)
    ids = ids[np.random.default_rng(100 * width_class + seed).permutation(ids.size)]
    return ids, dict(zip(runs, nodes))


def scatter_reference(ids, src, P, R, cols, dst0, wrong=None):
    """(float32 [num_rows, ld], float64 total) of pea_rows_scatter_sum on a table that holds dst0: for every id in [0, num_rows) the
    rows src[k] of its positions k, added in float32 one after the other in increasing k, stored at the channels' columns
    (channel c of the source at cols[c] .. cols[c] + R); rows and columns nobody writes keep dst0's value.
    wrong = ('drop_last', node): the node's last position is left out; ('swap', node, j): the rows of its positions j and j + 1 of
    the run are added in swapped order."""
    num_rows = dst0.shape[0]
    src = np.asarray(src, np.float32)
    want = np.array(dst0, np.float32)
    want64 = want.astype(np.float64)
    valid = np.flatnonzero((ids >= 0) & (ids < num_rows))
    order = valid[np.argsort(ids[valid], kind='stable')]                    # by id, a node's positions in increasing k
    starts = np.flatnonzero(np.concatenate([[True], ids[order][1:] != ids[order][:-1]])) if order.size else []
    for pos in np.split(order, starts[1:]) if order.size else []:
        i = int(ids[pos[0]])
        if wrong is not None and wrong[1] == i:
            if wrong[0] == 'drop_last':
                pos = pos[:-1]
            else:
                j = wrong[2]
                pos = np.concatenate([pos[:j], pos[[j + 1, j]], pos[j + 2:]])
        acc = src[pos[0]].copy()
        for q in pos[1:]:
            acc = acc + src[q]
        assert acc.dtype == np.float32
        tot = src[pos].astype(np.float64).sum(axis=0)
        for c in range(P):
            want[i, cols[c]:cols[c] + R] = acc[c * R:(c + 1) * R]
            want64[i, cols[c]:cols[c] + R] = tot[c * R:(c + 1) * R]
    return want, want64


def scatter_case(p, r, n_mod4):
    """(ids, run length -> node, src [n, W] float32 as a column slice of a wider buffer, cols, dst0 [SCATTER_ROWS, W + 4] of 7.0)"""
    w = p * r
    ids, nodes = scatter_ids(scatter_width_class(w), SCATTER_ROWS, n_mod4)
    rng = np.random.default_rng(1000 * p + r)
    wide = rng.standard_normal((ids.size, w + 8)).astype(np.float32)
    perm = rng.permutation(p)
    cols = [int(perm[q]) * r for q in range(p)]
    return ids, nodes, wide[:, 4:4 + w], cols, np.full((SCATTER_ROWS, w + 4), 7.0, np.float32)


def scatter_f64_bound(want64):
    """the float64 bound of tests/test_gpu_bpr_train.py's scatter test"""
    return 1e-5 * max(1.0, float(np.abs(want64).max()))


def scatter_limit_case(kind):
    """(ids [16384], src [16384, 16], num_rows) at the sort's limit: 'one_node' owns every position, 'distinct' = 16384 nodes, eight
    ids in every bucket, 'skipped' = nothing to add"""
    rng = np.random.default_rng(77)
    src = rng.standard_normal((SCATTER_MAX, 16)).astype(np.float32)
    if kind == 'one_node':
        return np.full(SCATTER_MAX, 2, np.int64), src, 3
    if kind == 'distinct':
        return rng.permutation(SCATTER_MAX).astype(np.int64), src, SCATTER_MAX
    ids = np.where(np.arange(SCATTER_MAX) % 3 == 0, -1, np.where(np.arange(SCATTER_MAX) % 3 == 1, 50, 2 ** 40)).astype(np.int64)
    return ids, src, 50
