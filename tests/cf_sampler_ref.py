"""The streams of the on-device CF epoch sampler (include/peahip_cf_sample.h) restated in numpy over oracle/philox.py: the
negative item with its rejection rule (oracle.philox.sample_negatives word for word, kept here so that the BCE numbering can
share it), the six entity columns from one Philox call per row, and the shuffle (perm of tests/kg_sampler_ref.py).  Imports
nothing from the product.  A helper: not collected."""
import numpy as np

from kg_sampler_ref import MASK32, MAX_ATTEMPTS, perm, philox4x32_10

TAG_ENTITY = 3 << 8
BPR, BCE = 0, 1


def csr_of(lists):
    """(ptr int64 [n + 1], ids int64 [nnz]) of a list of lists"""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    ids = np.asarray([v for l in lists for v in l], dtype=np.int64)
    return ptr, ids


def seen_keys(pos_u, pos_i, item_lo, num_items):
    """the sorted, distinct keys u * num_items + (i+ - item_lo)"""
    return np.unique(np.asarray(pos_u, dtype=np.int64) * num_items + (np.asarray(pos_i, dtype=np.int64) - item_lo))


def draw_negatives(users, item_lo, num_items, keys, seed, offset, live):
    """negative j of user users[j], j = 0 .. len(users) - 1: (int64 ids, bool which ran out).  Rows outside `live` draw nothing
    and keep item_lo."""
    n = users.size
    rows = np.arange(n, dtype=np.uint64)
    neg = np.full(n, item_lo, dtype=np.int64)
    todo = live.copy()
    if keys is not None and len(keys) == 0:
        keys = None
    for attempt in range(MAX_ATTEMPTS):
        idx = np.nonzero(todo)[0]
        if idx.size == 0:
            break
        r = rows[idx]
        w = philox4x32_10(r & MASK32, r >> np.uint64(32), np.full(r.shape, attempt, dtype=np.uint64),
                          np.full(r.shape, offset, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)[0]
        d = ((w * np.uint64(num_items)) >> np.uint64(32)).astype(np.int64)
        neg[idx] = item_lo + d
        if keys is None:
            todo[idx] = False
        else:
            key = users[idx] * num_items + d
            pos = np.searchsorted(keys, key)
            todo[idx] = (pos < keys.size) & (keys[np.minimum(pos, keys.size - 1)] == key)
    return neg, todo


def entity_triple(ptr, ids, owner, w_pos, w_neg, block_lo, block_n, live):
    """(e+, e-, mask) int64 [n, 3] of every row: owner [n] indexes the CSR (ptr, ids), w_pos / w_neg uint64 [n] the two words"""
    n = owner.size
    out = np.zeros((n, 3), dtype=np.int64)
    own = np.where(live, owner, 0)
    a, b = ptr[own], ptr[own + 1]
    length = np.where(live, b - a, 0)
    has = length > 0
    pick = a[has] + ((w_pos[has] * length[has].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    e = ids[pick]
    blk = np.maximum(np.searchsorted(block_lo, e, side='right') - 1, 0)
    out[has, 0] = e
    out[has, 1] = block_lo[blk] + ((w_neg[has] * block_n[blk].astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    out[has, 2] = 1
    return out


def sample(pos_u, pos_i, k, mode, item_lo, num_items, user_lo, num_users, keys=None, entity=None, seed=0, offset=0, shuffle=False):
    """(int64 table, rows whose attempts ran out, bad rows, bool [negatives] which negatives ran out).  entity: None or
    (item_ptr, item_ids, user_ptr, user_ids, block_lo, block_n); keys: the sorted key table ('unseen') or None."""
    pos_u, pos_i = np.asarray(pos_u, dtype=np.int64), np.asarray(pos_i, dtype=np.int64)
    n_pos = pos_u.size
    assert mode in (BPR, BCE) and not (mode == BCE and entity is not None)
    u = np.repeat(pos_u, k)
    u_ok = (u >= user_lo) & (u < user_lo + num_users)
    if mode == BPR:
        ip = np.repeat(pos_i, k)
        live = u_ok & (ip >= item_lo) & (ip < item_lo + num_items)
        if entity is not None:
            item_ptr, item_ids, user_ptr, user_ids, block_lo, block_n = (np.asarray(a, dtype=np.int64) for a in entity)
            for ptr, ids, owner in ((item_ptr, item_ids, ip - item_lo), (user_ptr, user_ids, u - user_lo)):
                own = np.where(live, owner, 0)
                live &= (ptr[own] >= 0) & (ptr[own] <= ptr[own + 1]) & (ptr[own + 1] <= ids.size)
        neg, out_of = draw_negatives(u, item_lo, num_items, keys, seed, offset, live)
        cols = [u, ip, neg]
        if entity is not None:
            r = np.arange(u.size, dtype=np.uint64)
            e = philox4x32_10(r & MASK32, r >> np.uint64(32), np.full(r.shape, TAG_ENTITY, dtype=np.uint64),
                              np.full(r.shape, offset, dtype=np.uint64), seed & 0xFFFFFFFF, seed >> 32)
            item_cols = entity_triple(item_ptr, item_ids, ip - item_lo, e[0], e[1], block_lo, block_n, live)
            user_cols = entity_triple(user_ptr, user_ids, u - user_lo, e[2], e[3], block_lo, block_n, live)
            cols += list(item_cols.T) + list(user_cols.T)
        table = np.stack(cols, axis=1) if u.size else np.zeros((0, len(cols)), dtype=np.int64)
        bad = int((~live).sum())
    else:
        pos_ok = (pos_u >= user_lo) & (pos_u < user_lo + num_users) & (pos_i >= item_lo) & (pos_i < item_lo + num_items)
        neg, out_of = draw_negatives(u, item_lo, num_items, keys, seed, offset, u_ok)
        table = np.concatenate([np.stack([pos_u, pos_i, np.ones(n_pos, dtype=np.int64)], axis=1),
                                np.stack([u, neg, np.zeros(u.size, dtype=np.int64)], axis=1)])
        bad = int((~pos_ok).sum() + (~u_ok).sum())
    if shuffle and table.shape[0]:
        out = np.empty_like(table)
        out[perm(table.shape[0], seed, offset)] = table
        table = out
    return table, int(out_of.sum()), bad, out_of


# ---------------------------------------------------------------- the datasets the two test files share
class EntityDataset:
    """The construction of tests/test_sampling_metrics.py::_entity_dataset (oracle/make_golden.py::entity_fake_dataset), rebuilt:
    40 users, 70 items, the unique pairs of 600 draws, blocks genre 5 and tid 9; item lists of 0..3 entities over both blocks,
    user lists of 0..2 tags."""

    def __init__(self, seed=13, n_user=40, n_item=70, e=600):
        rng = np.random.default_rng(seed)
        self.type_accs = {'uid': 0, 'iid': n_user}
        self.num_uids, self.num_iids = n_user, n_item
        u = rng.integers(0, n_user, size=e)
        i = n_user + rng.integers(0, n_item, size=e)
        pairs = np.unique(np.stack([u, i]), axis=1)
        self.edge_index_nps = {'user2item': pairs.astype(np.float64)}
        self.cf_loss_type, self.entity_aware = 'BPR', True
        self.num_negative_samples, self.sampling_strategy = 4, 'random'
        rng = np.random.default_rng(seed + 100)
        base = n_user + n_item
        self.type_accs.update({'genre': base, 'tid': base + 5})
        self.num_genres, self.num_tids = 5, 9
        self.nid2e_dict = {base + k: ('genre', k) for k in range(5)}
        self.nid2e_dict.update({base + 5 + k: ('tid', k) for k in range(9)})
        self.iid_feat_nids = [[int(base + v) for v in rng.integers(0, 14, size=int(rng.integers(0, 4)))] for _ in range(n_item)]
        self.uid_feat_nids = [[int(base + 5 + v) for v in rng.integers(0, 9, size=int(rng.integers(0, 3)))] for _ in range(n_user)]


class SmallDataset:
    """15 users (0..14), 20 items (15..34), blocks genre 5 (35..39), tid 9 (40..48) and year 1 (49: a block of one node).
    Item 0 has a list of 300 entries (duplicates), the others lists of 0, 1, 2 or 3; users have 0, 1 or 2 tags, or the year.
    user2item: n_pos pairs drawn with repetition; full_user: user 0 is also paired with every item."""

    def __init__(self, n_pos, k=1, loss='BPR', strategy='random', entity_aware=False, seed=0, full_user=False):
        rng = np.random.default_rng(seed)
        self.type_accs = {'uid': 0, 'iid': 15, 'genre': 35, 'tid': 40, 'year': 49}
        self.num_uids, self.num_iids, self.num_genres, self.num_tids, self.num_years = 15, 20, 5, 9, 1
        self.num_nodes = 50
        pairs = np.stack([rng.integers(0, 15, n_pos), rng.integers(15, 35, n_pos)])
        if full_user:
            pairs[0, pairs[0] == 0] = 1
            pairs = np.concatenate([np.stack([np.zeros(20, dtype=np.int64), np.arange(15, 35)]), pairs], axis=1)[:, :max(n_pos, 20)]
        self.edge_index_nps = {'user2item': pairs.astype(np.float64)}
        self.cf_loss_type, self.sampling_strategy, self.entity_aware = loss, strategy, entity_aware
        self.num_negative_samples = k
        self.nid2e_dict = {35 + j: ('genre', j) for j in range(5)}
        self.nid2e_dict.update({40 + j: ('tid', j) for j in range(9)})
        self.nid2e_dict[49] = ('year', 0)
        self.iid_feat_nids = [[int(v) for v in rng.integers(35, 50, size=300)]]
        self.iid_feat_nids += [[int(v) for v in rng.integers(35, 50, size=j % 4)] for j in range(1, 20)]
        self.uid_feat_nids = [[49] if j == 7 else [int(v) for v in rng.integers(40, 49, size=j % 3)] for j in range(15)]

    def positives(self):
        e = self.edge_index_nps['user2item'].astype(np.int64)
        return e[0], e[1]

    def entity_tables(self):
        """what sample() takes as `entity`: the CSR pairs and the blocks of every sized type, ascending"""
        blocks = sorted((lo, getattr(self, 'num_%ss' % t)) for t, lo in self.type_accs.items())
        return csr_of(self.iid_feat_nids) + csr_of(self.uid_feat_nids) + (np.array([b[0] for b in blocks]),
                                                                          np.array([b[1] for b in blocks]))


def sample_dataset(ds, seed, offset=0, shuffle=False):
    """sample() with every argument taken from a dataset object, as utils.device_cf_negative_sampling takes them"""
    e = ds.edge_index_nps['user2item'].astype(np.int64)
    lo, n = ds.type_accs['iid'], ds.num_iids
    keys = seen_keys(e[0], e[1], lo, n) if ds.sampling_strategy == 'unseen' else None
    entity = None
    if ds.entity_aware:
        blocks = sorted((b, getattr(ds, 'num_%ss' % t)) for t, b in ds.type_accs.items())
        entity = csr_of(ds.iid_feat_nids) + csr_of(ds.uid_feat_nids) + (np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks]))
    return sample(e[0], e[1], ds.num_negative_samples, BPR if ds.cf_loss_type == 'BPR' else BCE, lo, n, ds.type_accs['uid'],
                  ds.num_uids, keys=keys, entity=entity, seed=seed, offset=offset, shuffle=shuffle)
