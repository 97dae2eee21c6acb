"""The streams of the on-device KG triple sampler (include/peahip_sample.h) restated in numpy over oracle/philox.py: the keyed
bijection perm, the negative-tail draw with its rejection rule, and the sampled table.  Imports nothing from the product.
A helper: not collected."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.philox import philox4x32_10                                # noqa: E402

TAG_DRAW, TAG_SHUFFLE = 1 << 8, 2 << 8
MAX_ATTEMPTS = 64
MASK32 = np.uint64(0xFFFFFFFF)


def half_bits(n):
    b = max(int(n - 1).bit_length(), 1)
    return max((b + 1) // 2, 1)


def feistel_pass(x, hb, seed, offset):
    """one pass of the 4-round network on a uint64 array of values below 2^(2 hb)"""
    m = np.uint64((1 << hb) - 1)
    sh = np.uint64(hb)
    left, right = x >> sh, x & m
    for j in range(4):
        f = philox4x32_10(right, np.full(x.shape, j, dtype=np.uint64), np.full(x.shape, TAG_SHUFFLE, dtype=np.uint64),
                          np.full(x.shape, offset, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)[0] & m
        left, right = right, left ^ f
    return (left << sh) | right


def perm(n, seed=0, offset=0, return_passes=False):
    """perm(e) for e = 0 .. n - 1 (int64 [n]); with return_passes also the passes each e needed"""
    hb = half_bits(n)
    y = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    passes = np.zeros(n, dtype=np.int64)
    while todo.any():
        idx = np.nonzero(todo)[0]
        y[idx] = feistel_pass(y[idx], hb, seed, offset)
        passes[idx] += 1
        todo[idx] = y[idx] >= np.uint64(n)
    out = y.astype(np.int64)
    return (out, passes) if return_passes else out


def segment_of_rows(seg_ptr):
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    return np.repeat(np.arange(seg_ptr.size - 1, dtype=np.int64), np.diff(seg_ptr))


def known_keys(heads, tails, seg_ptr, num_nodes):
    """the sorted, distinct keys ((s N) + h) N + t of the store's triples"""
    s = segment_of_rows(seg_ptr)
    return np.unique((s * num_nodes + np.asarray(heads, dtype=np.int64)) * num_nodes + np.asarray(tails, dtype=np.int64))


def sample(heads, tails, seg_ptr, seg_rel, seg_lo, seg_n, num_nodes, keys=None, seed=0, offset=0, shuffle=False):
    """(int64 [E, 4] rows (h, t+, t-, relation id), rows whose attempts ran out, bool [E] which store rows those are).
    keys: the sorted key table (filtered draws) or None."""
    heads, tails = np.asarray(heads, dtype=np.int64), np.asarray(tails, dtype=np.int64)
    seg_rel, seg_lo, seg_n = (np.asarray(a, dtype=np.int64) for a in (seg_rel, seg_lo, seg_n))
    n = heads.size
    s = segment_of_rows(seg_ptr)
    assert s.size == n
    rows = np.arange(n, dtype=np.uint64)
    lo, span = seg_lo[s], seg_n[s].astype(np.uint64)
    neg = lo.copy()
    todo = np.ones(n, dtype=bool)
    if keys is not None and len(keys) == 0:
        keys = None
    for attempt in range(MAX_ATTEMPTS):
        idx = np.nonzero(todo)[0]
        if idx.size == 0:
            break
        r = rows[idx]
        w = philox4x32_10(r & MASK32, r >> np.uint64(32), np.full(r.shape, attempt | TAG_DRAW, dtype=np.uint64),
                          np.full(r.shape, offset, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)[0]
        t_neg = lo[idx] + ((w * span[idx]) >> np.uint64(32)).astype(np.int64)
        neg[idx] = t_neg
        if keys is None:
            todo[idx] = False
        else:
            key = (s[idx] * num_nodes + heads[idx]) * num_nodes + t_neg
            pos = np.searchsorted(keys, key)
            known = (pos < keys.size) & (keys[np.minimum(pos, keys.size - 1)] == key)
            todo[idx] = known | (t_neg == tails[idx])
    table = np.stack([heads, tails, neg, seg_rel[s]], axis=1) if n else np.zeros((0, 4), dtype=np.int64)
    if shuffle and n:
        out = np.empty_like(table)
        out[perm(n, seed, offset)] = table
        table = out
    return table, int(todo.sum()), todo
