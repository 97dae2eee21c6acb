"""Helper (not collected): restatements for the metapath2vec tests.

  * both walk kinds of csrc/walk.hip in numpy, on top of oracle.philox.philox4x32_10 and a CSR (rowptr, col);
  * the skip-gram loss of the reference (models/metapath2vec.py:147-172) in torch, on the reference's window layout
    (:117-121), at float32 or float64, with the means over the valid pairs;
  * a toy heterogeneous graph in one global id space.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.philox import MASK, philox4x32_10                        # noqa: E402

EPS = 1e-15


def _words(n_walks, t, seed, offset):
    rows = np.arange(n_walks, dtype=np.uint64)
    w, _, _, _ = philox4x32_10(rows & MASK, rows >> np.uint64(32), np.full(n_walks, t, dtype=np.uint64),
                               np.full(n_walks, offset, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    return w


def metapath_walks(csrs, relations, starts, walk_length, seed, offset, num_nodes):
    """(walks int64 [n, L + 1], [walks that met a dead end, bad starts]); csrs[r] = (rowptr, col) of relation r: the row of a
    node holds the nodes a step from it may go to."""
    starts = np.asarray(starts, dtype=np.int64)
    n = starts.shape[0]
    walks = np.full((n, walk_length + 1), -1, dtype=np.int64)
    ok = (starts >= 0) & (starts < num_nodes)
    walks[ok, 0] = starts[ok]
    alive = ok.copy()
    dead = 0
    for t in range(1, walk_length + 1):
        rowptr, col = (np.asarray(a, dtype=np.int64) for a in csrs[relations[(t - 1) % len(relations)]])
        cur = np.where(alive, walks[:, t - 1], 0)
        beg, deg = rowptr[cur], rowptr[cur + 1] - rowptr[cur]
        w = _words(n, t, seed, offset)
        stop = alive & (deg == 0)
        dead += int(stop.sum())
        alive &= deg > 0
        slot = beg + ((w * deg.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        walks[alive, t] = col[slot[alive]]
    return walks, [dead, int((~ok).sum())]


def uniform_walks(block_lo, block_n, starts, walk_length, seed, offset):
    starts = np.asarray(starts, dtype=np.int64)
    n = starts.shape[0]
    walks = np.empty((n, walk_length + 1), dtype=np.int64)
    walks[:, 0] = starts
    for t in range(1, walk_length + 1):
        s = (t - 1) % len(block_lo)
        w = _words(n, t, seed, offset)
        walks[:, t] = block_lo[s] + ((w * np.uint64(block_n[s])) >> np.uint64(32)).astype(np.int64)
    return walks


def windows(rw, context_size):
    """the reference's slicing of whole walks (models/metapath2vec.py:117-121)"""
    rw = np.asarray(rw)
    return np.concatenate([rw[:, j:j + context_size] for j in range(rw.shape[1] - context_size + 1)], axis=0)


def skipgram_loss(weight, pos_win, neg_win, dtype):
    """(loss, pos, neg, d loss / d weight [N, D], valid pairs per side) of the reference's loss on window rows [M, C] (int64
    numpy), computed by torch autograd in `dtype`; a pair with an id outside [0, N) is skipped, the means run over the valid
    pairs, a side without one gives 0."""
    import torch
    w = torch.from_numpy(np.asarray(weight)).to(dtype).requires_grad_(True)
    n = w.shape[0]
    sides, counts = [], []
    for win, positive in ((pos_win, True), (neg_win, False)):
        win = torch.from_numpy(np.asarray(win, dtype=np.int64).reshape(-1, np.asarray(pos_win if positive else neg_win).shape[-1]))
        if win.shape[0] == 0:
            sides.append(w.sum() * 0)
            counts.append(0)
            continue
        start, rest = win[:, :1], win[:, 1:]
        valid = (start >= 0) & (start < n) & (rest >= 0) & (rest < n)
        h_start = w[start.clamp(0, n - 1)]
        h_rest = w[rest.clamp(0, n - 1)]
        out = (h_start * h_rest).sum(dim=-1)
        sig = torch.sigmoid(out)
        term = -torch.log((sig if positive else 1 - sig) + EPS)
        cnt = int(valid.sum())
        sides.append((term * valid).sum() / max(cnt, 1))
        counts.append(cnt)
    loss = sides[0] + sides[1]
    loss.backward()
    return (np.array([loss.item(), sides[0].item(), sides[1].item()], dtype=np.float64), w.grad.numpy().astype(np.float64),
            counts)


def toy_hin(seed=7, n_user=40, n_item=30, n_genre=5):
    """users, items and genres in one global id space (in that order).  Random user2item and genre2item edges, some doubled;
    genre 0 is a hub (every item that has a genre has it); the last two items have no genre, the last item no user either,
    and the last user has no item.  Returns a dict: types, num_nodes_dict, type_accs, num_nodes, edge_index_dict (numpy int64
    [2, E] per (source type, name, target type), both directions) and the metapath user -> item -> genre -> item -> user."""
    rng = np.random.default_rng(seed)
    u0, i0, g0 = 0, n_user, n_user + n_item
    users = rng.integers(0, n_user - 1, size=160)                      # the last user stays without an item
    items = rng.integers(0, n_item - 1, size=160)                      # the last item stays without a user
    u2i = np.stack([u0 + users, i0 + items])
    u2i = np.concatenate([u2i, u2i[:, :25]], axis=1)                   # doubled edges
    gi = np.arange(n_item - 2)                                         # the last two items stay without a genre
    g2i = np.stack([np.full(gi.size, g0), i0 + gi])                    # the hub genre
    extra = np.stack([g0 + rng.integers(1, n_genre, size=40), i0 + rng.integers(0, n_item - 2, size=40)])
    g2i = np.concatenate([g2i, extra, extra[:, :8]], axis=1)
    u2i, g2i = u2i.astype(np.int64), g2i.astype(np.int64)
    eid = {('uid', 'has watched', 'iid'): u2i, ('iid', 'has been watched by', 'uid'): np.ascontiguousarray(u2i[::-1]),
           ('genre', 'as the genre of', 'iid'): g2i, ('iid', 'has the genre', 'genre'): np.ascontiguousarray(g2i[::-1])}
    metapath = [('uid', 'has watched', 'iid'), ('iid', 'has the genre', 'genre'), ('genre', 'as the genre of', 'iid'),
                ('iid', 'has been watched by', 'uid')]
    return dict(types=['uid', 'iid', 'genre'], num_nodes_dict={'uid': n_user, 'iid': n_item, 'genre': n_genre},
                type_accs={'uid': u0, 'iid': i0, 'genre': g0}, num_nodes=n_user + n_item + n_genre, edge_index_dict=eid,
                metapath=metapath)


def csr_of(edge_index, num_nodes):
    """(rowptr, col) whose row of node a holds b for every edge (a, b), in edge order: what a walk from edge_index[0] to
    edge_index[1] steps over (the plan's CSR of the flipped COO)"""
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    order = np.argsort(src, kind='stable')
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=num_nodes))]).astype(np.int64)
    return rowptr, dst[order].astype(np.int64)


WALK_SEED = (5 << 32) | 2024          # the seed the GPU comparison uses
