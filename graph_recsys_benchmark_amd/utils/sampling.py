"""Host-side samplers with the reference's exact RNG call sequence, so sampled ids are BIT-EXACT given the same
seeds (`random.seed / np.random.seed / torch.manual_seed`, reference solvers.py:123-127) and the same call order.

    cf_negative_sampling   graph_recsys_benchmark/datasets/movielens.py:879-997 (BPR branch :920-940, BCE branch :886-917, shuffle :994-997)
                           (Yelp twin: datasets/yelp.py:746-760)
    kg_negative_sampling   graph_recsys_benchmark/datasets/movielens.py:861-877 (the KG quadruples CFKG trains on)
    generate_candidates    graph_recsys_benchmark/solvers.py:21-31
    entity_aware_row       graph_recsys_benchmark/datasets/movielens.py:1147-1181 (the six entity columns of a row)

They stay on the host on purpose: numpy's legacy RandomState stream and Python's `random` are version-frozen, a
device-side Philox stream would not reproduce the reference's ids.

    device_negative_sampling   the ADDITIONAL device-side sampler: same strategies and output
                               layout, its own Philox4x32-10 stream (csrc/sampler.hip); never a replacement for the
                               bit-exact path above.
    device_kg_negative_sampling   its KG twin (csrc/kg_sampler.hip): the (h, t+, t-, rel) table of kg_negative_sampling from
                               one launch over a kg_triple_store, the epoch shuffle a keyed bijection inside that launch;
                               device_shuffle_rows applies the same bijection to any int64 table.
    device_cf_negative_sampling   the CF epoch table from one launch (csrc/cf_sampler.hip): the BPR rows of device_negative_sampling,
                               the BCE rows NFM trains on, or the nine-column entity-aware rows over an entity_store, the epoch
                               shuffle inside the launch.
"""
import random as rd

import numpy as np
import torch


def cf_negative_sampling(dataset):
    """BPR training triples: every positive (u, i+) repeated `num_negative_samples` times + one sampled negative
    column, then a torch.randperm shuffle.  Sets dataset.train_data / train_data_length like the reference and
    returns the int64 [M*neg, 3] tensor."""
    if dataset.cf_loss_type == 'BCE':
        return _cf_negative_sampling_bce(dataset)
    if dataset.cf_loss_type != 'BPR':
        raise NotImplementedError('only the BPR and BCE branches are on the accelerated path')
    pos = dataset.edge_index_nps['user2item'].T
    num_interactions = pos.shape[0]
    k = dataset.num_negative_samples
    train_data_np = np.repeat(pos, repeats=k, axis=0)
    if dataset.sampling_strategy == 'random':
        lo = dataset.type_accs['iid']
        neg = np.random.randint(low=lo, high=lo + dataset.num_iids, size=(num_interactions * k, 1))
    elif dataset.sampling_strategy == 'unseen':
        parts = []
        for u_nid in pos[:, 0]:
            pool = dataset.test_pos_unid_inid_map[u_nid] + dataset.neg_unid_inid_map[u_nid]
            parts.append(np.array(rd.choices(pool, k=k), dtype=np.int64).reshape(-1, 1))
        neg = np.vstack(parts)
    else:
        raise NotImplementedError
    train_data_np = np.hstack([train_data_np, neg])
    if getattr(dataset, 'entity_aware', False) and not hasattr(dataset, 'iid_feat_nids'):
        # the reference builds the per-item / per-user entity lists here from its processed CSV files
        # (datasets/movielens.py:941-991): dataset ETL, outside the accelerated path.  Without them the six
        # entity columns __getitem__ appends (see entity_aware_row) cannot be drawn, and a model with
        # entity_aware=True would index columns 3..8 of a 3-column batch.
        raise NotImplementedError('entity_aware=True needs dataset.iid_feat_nids / uid_feat_nids / nid2e_dict '
                                  '(built by the reference\'s dataset preprocessing); attach them to the dataset')
    train_data_t = torch.from_numpy(train_data_np).long()
    shuffle_idx = torch.randperm(train_data_t.shape[0])
    dataset.train_data = train_data_t[shuffle_idx]
    dataset.train_data_length = train_data_t.shape[0]
    return dataset.train_data


def _cf_negative_sampling_bce(dataset):
    """The BCE branch (datasets/movielens.py:886-917), what NFM trains on: every positive (u, i+, 1), then
    `num_negative_samples` rows (u, sampled item, 0) per positive, then the shared torch.randperm shuffle: int64
    [M (1 + neg), 3].  'random': ONE np.random.randint over all negatives; 'unseen': one np.random.choice per positive over the
    user's held-out and never-seen items -- numpy's stream here, where the BPR branch draws with Python's `random`."""
    pos = dataset.edge_index_nps['user2item'].T
    num_interactions = pos.shape[0]
    k = dataset.num_negative_samples
    pos_samples_np = np.hstack([pos, np.ones((num_interactions, 1))])
    users = np.repeat(pos_samples_np[:, 0].reshape(-1, 1), repeats=k, axis=0)
    if dataset.sampling_strategy == 'random':
        lo = dataset.type_accs['iid']
        neg = np.random.randint(low=lo, high=lo + dataset.num_iids, size=(num_interactions * k, 1))
    elif dataset.sampling_strategy == 'unseen':
        parts = []
        for u_nid in pos_samples_np[:, 0]:
            pool = dataset.test_pos_unid_inid_map[u_nid] + dataset.neg_unid_inid_map[u_nid]
            parts.append(np.random.choice(pool, size=(k, 1)))
        neg = np.vstack(parts)
    else:
        raise NotImplementedError
    neg_samples_np = np.hstack([users, neg, np.zeros((num_interactions * k, 1))])
    train_data_t = torch.from_numpy(np.vstack([pos_samples_np, neg_samples_np])).long()
    shuffle_idx = torch.randperm(train_data_t.shape[0])
    dataset.train_data = train_data_t[shuffle_idx]
    dataset.train_data_length = train_data_t.shape[0]
    return dataset.train_data


def kg_negative_sampling(dataset):
    """KG training quadruples: every edge of every relation of dataset.edge_index_nps as (h, t+), one uniformly drawn node as
    the negative tail (ONE np.random.randint over all edges) and the relation's edge_type_dict id, then a torch.randperm
    shuffle.  Sets dataset.train_data / train_data_length like the reference and returns the int64 [E, 4] tensor
    (h, t+, t-, rel).  A dataset without edge_type_dict gets the types the reference's dataset builds: enumerate over the keys
    of edge_index_nps (datasets/movielens.py:329)."""
    type_of = getattr(dataset, 'edge_type_dict', None)
    if type_of is None:
        type_of = {name: k for k, name in enumerate(dataset.edge_index_nps.keys())}
    pairs = [(edge_index, np.ones((edge_index.shape[1], 1)) * type_of[edge_type])
             for edge_type, edge_index in dataset.edge_index_nps.items()]
    pos_np = np.hstack([p[0] for p in pairs]).T
    r_np = np.vstack([p[1] for p in pairs])
    neg_t_np = np.random.randint(low=0, high=dataset.num_nodes, size=(pos_np.shape[0], 1))
    train_data_t = torch.from_numpy(np.hstack([pos_np, neg_t_np, r_np])).long()
    shuffle_idx = torch.randperm(train_data_t.shape[0])
    dataset.train_data = train_data_t[shuffle_idx]
    dataset.train_data_length = train_data_t.shape[0]
    return dataset.train_data


def entity_aware_row(dataset, train_data_t):
    """One training row as the reference's Dataset.__getitem__ returns it (datasets/movielens.py:1147-1181): with
    dataset.entity_aware the (u, i+, i-) row gets six more columns -- positive / negative entity of the item, mask,
    positive / negative entity of the user, mask -- drawn with Python's `random` in the reference's call order (bit-exact
    when called from the seeded main process; the reference's DataLoader workers make its own stream irreproducible,
    SURVEY.md appendix C.10).  `train_data_t`: int64 [3] tensor = dataset.train_data[idx]."""
    if not getattr(dataset, 'entity_aware', False):
        return train_data_t
    out = []
    for col, feats_of, acc in ((1, dataset.iid_feat_nids, dataset.type_accs['iid']),
                               (0, dataset.uid_feat_nids, dataset.type_accs['uid'])):
        nid = int(train_data_t[col])
        feat_nids = feats_of[int(nid - acc)]
        if len(feat_nids) == 0:
            out += [0, 0, 0]
        else:
            pos_entity = rd.choice(feat_nids)
            entity_type = dataset.nid2e_dict[pos_entity][0]
            lower = dataset.type_accs.get(entity_type)
            upper = lower + getattr(dataset, 'num_' + entity_type + 's')
            out += [pos_entity, rd.choice(range(lower, upper)), 1]
    return torch.cat([train_data_t, torch.tensor(out, dtype=torch.long)], dim=-1)


def generate_candidates(dataset, u_nid, num_neg_candidates=99):
    """(positives, negatives) for one test user: the held-out positives and `num_neg_candidates` negatives drawn
    WITH replacement by np.random.choice (reference solvers.py:28-29)."""
    pos_i_nids = dataset.test_pos_unid_inid_map[u_nid]
    neg_i_nids = list(np.random.choice(dataset.neg_unid_inid_map[u_nid], size=(num_neg_candidates,)))
    return pos_i_nids, neg_i_nids


def device_negative_sampling(dataset, seed, epoch=0, device='cuda', shuffle=True):
    """BPR triples sampled ON THE GPU: int64 [M * num_negative_samples, 3] CUDA tensor (u, i+, i-), optionally shuffled
    with torch.randperm on the device.  'random': uniform items; 'unseen': uniform over the items the user has no
    training interaction with (the pool the reference draws from, datasets/movielens.py:929-937).  `epoch` selects an
    independent stream per call (the Philox counter's fourth word)."""
    from .. import _lib
    lib = _lib.require_device()
    if dataset.cf_loss_type != 'BPR':
        raise NotImplementedError('only the BPR branch is on the accelerated path')
    pos = torch.as_tensor(dataset.edge_index_nps['user2item']).to(device=device, dtype=torch.int64)
    pos_u, pos_i = pos[0].contiguous(), pos[1].contiguous()
    k = int(dataset.num_negative_samples)
    lo, n_items = int(dataset.type_accs['iid']), int(dataset.num_iids)
    keys = None
    if dataset.sampling_strategy == 'unseen':
        keys = torch.unique(pos_u * n_items + (pos_i - lo))        # ascending
    elif dataset.sampling_strategy != 'random':
        raise NotImplementedError
    out = torch.empty((pos_u.numel() * k, 3), dtype=torch.int64, device=device)
    exhausted = torch.zeros(1, dtype=torch.int32, device=device)
    _lib.check(lib.pea_sample_negatives(pos_u.numel(), k, _lib.ptr(pos_u), _lib.ptr(pos_i), lo, n_items, _lib.ptr(keys),
                                        0 if keys is None else keys.numel(), int(seed) & (2 ** 64 - 1),
                                        int(epoch) & 0xFFFFFFFF, _lib.ptr(out), out.stride(0), _lib.ptr(exhausted),
                                        _lib.current_stream()))
    n_exhausted = int(exhausted.item())
    if n_exhausted:
        # 'unseen': 64 rejection attempts all hit seen items (a user who has rated nearly every item); the row keeps
        # a seen item as its negative.  Loud, because such a row is a false negative.
        import warnings
        warnings.warn('device_negative_sampling: %d of %d negatives are seen items (rejection sampling exhausted)'
                      % (n_exhausted, out.shape[0]), RuntimeWarning)
    dataset.negatives_exhausted = n_exhausted
    if shuffle:
        out = out[torch.randperm(out.shape[0], device=device)]
    dataset.train_data, dataset.train_data_length = out, out.shape[0]
    return out


# ---- the KG twin: on-device triple sampler with the epoch shuffle inside the launch (csrc/kg_sampler.hip,
# ---- include/peahip_sample.h).  An addition next to kg_negative_sampling above, never its replacement: its ids are its own.
class KGTripleStore:
    """Every KG triple of a dataset, laid out for pea_kg_sample: heads / tails int64 [E] in the order kg_negative_sampling
    stacks them (relation by relation, in the order of dataset.edge_index_nps), and one segment per relation: seg_ptr
    [S + 1], seg_rel [S] (the relation's edge_type_dict id), and the node block (seg_lo, seg_n) [S] its typed negatives are
    drawn from.  `host` holds the numpy copies of the four tables."""

    def __init__(self, heads, tails, seg_ptr, seg_rel, seg_lo, seg_n, num_nodes, device):
        self.num_nodes, self.device = int(num_nodes), torch.device(device)
        self.host = {'seg_ptr': seg_ptr, 'seg_rel': seg_rel, 'seg_lo': seg_lo, 'seg_n': seg_n}
        to = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64)).to(self.device)
        self.heads, self.tails = to(heads), to(tails)
        self.device = self.heads.device                                # with its index: 'cuda' became 'cuda:0'
        self.seg_ptr, self.seg_rel, self.seg_lo, self.seg_n = to(seg_ptr), to(seg_rel), to(seg_lo), to(seg_n)
        s = len(seg_rel)
        self.any_lo, self.any_n = to(np.zeros(s)), to(np.full(s, self.num_nodes))       # strategy 'random': any node
        self._keys = None

    @property
    def num_triples(self):
        return int(self.heads.numel())

    @property
    def num_segments(self):
        return int(self.seg_rel.numel())

    def segment_of_rows(self):
        """int64 [E]: the segment index of every store row"""
        counts = self.seg_ptr[1:] - self.seg_ptr[:-1]
        return torch.repeat_interleave(torch.arange(self.num_segments, device=self.device), counts)

    def rows(self):
        """int64 [E, 3]: (h, t+, relation id) of every store row, in store order"""
        return torch.stack([self.heads, self.tails, self.seg_rel[self.segment_of_rows()]], dim=1)

    def keys(self):
        """The sorted table of known triples, ((s N) + h) N + t, built once (torch.unique on the store's device)"""
        if self._keys is None:
            n = self.num_nodes
            self._keys = torch.unique((self.segment_of_rows() * n + self.heads) * n + self.tails)
        return self._keys


def _default_tail_blocks(dataset, names, tails_of):
    """{relation: (lo, n)}: the node-type block of dataset.type_accs that holds the relation's tails; a block ends where the
    next one starts (the last at num_nodes).  A relation without triples draws from every node."""
    starts = np.asarray(sorted(set(int(v) for v in dataset.type_accs.values())) + [int(dataset.num_nodes)], dtype=np.int64)
    blocks = {}
    for name in names:
        t = tails_of[name]
        if t.size == 0:
            blocks[name] = (0, int(dataset.num_nodes))
            continue
        k = int(np.searchsorted(starts, int(t.min()), side='right')) - 1
        if k < 0 or k >= starts.size - 1:
            raise ValueError('kg_triple_store: tails of %r lie outside every node-type block' % name)
        blocks[name] = (int(starts[k]), int(starts[k + 1] - starts[k]))
    return blocks


def kg_triple_store(dataset, device='cuda', tail_blocks=None):
    """The KGTripleStore of a dataset, built once per dataset: relations in the order of dataset.edge_index_nps, relation ids
    from edge_type_dict (or enumerated, as kg_negative_sampling does).  tail_blocks = {relation: (lo, n)} names the node block
    a relation's typed negatives come from; by default the dataset.type_accs block its tails lie in.  A relation whose tails
    leave their block raises ValueError, as do more than 1024 relations and ids outside [0, num_nodes)."""
    from .. import _lib
    type_of = getattr(dataset, 'edge_type_dict', None)
    if type_of is None:
        type_of = {name: k for k, name in enumerate(dataset.edge_index_nps.keys())}
    names = list(dataset.edge_index_nps.keys())
    n = int(dataset.num_nodes)
    if not 1 <= len(names) <= _lib.KG_MAX_SEGMENTS:
        raise ValueError('kg_triple_store: %d relations (1..%d)' % (len(names), _lib.KG_MAX_SEGMENTS))
    if not 1 <= n < 2 ** 32:
        raise ValueError('kg_triple_store: num_nodes %d outside [1, 2^32)' % n)
    edges = {name: np.asarray(dataset.edge_index_nps[name]).astype(np.int64).reshape(2, -1) for name in names}
    tails_of = {name: edges[name][1] for name in names}
    if tail_blocks is None:
        tail_blocks = _default_tail_blocks(dataset, names, tails_of)
    seg_ptr = np.zeros(len(names) + 1, dtype=np.int64)
    seg_rel, seg_lo, seg_n = (np.zeros(len(names), dtype=np.int64) for _ in range(3))
    for s, name in enumerate(names):
        lo, cnt = (int(v) for v in tail_blocks[name])
        e = edges[name]
        if not (0 <= lo and 1 <= cnt and lo + cnt <= n):
            raise ValueError('kg_triple_store: tail block (%d, %d) of %r is not inside [0, %d)' % (lo, cnt, name, n))
        if e.size and (e.min() < 0 or e.max() >= n):
            raise ValueError('kg_triple_store: a node id of %r is outside [0, %d)' % (name, n))
        if e.size and (e[1].min() < lo or e[1].max() >= lo + cnt):
            raise ValueError('kg_triple_store: tails of %r leave their block [%d, %d)' % (name, lo, lo + cnt))
        seg_ptr[s + 1] = seg_ptr[s] + e.shape[1]
        seg_rel[s], seg_lo[s], seg_n[s] = int(type_of[name]), lo, cnt
    heads = np.concatenate([edges[name][0] for name in names])
    tails = np.concatenate([edges[name][1] for name in names])
    return KGTripleStore(heads, tails, seg_ptr, seg_rel, seg_lo, seg_n, n, device)


def _store_of(dataset_or_store, device):
    if isinstance(dataset_or_store, KGTripleStore):
        return dataset_or_store
    store = getattr(dataset_or_store, 'kg_store', None)
    if not isinstance(store, KGTripleStore) or store.device != torch.empty(0, device=device).device:
        store = kg_triple_store(dataset_or_store, device)
        dataset_or_store.kg_store = store
    return store


def device_kg_negative_sampling(dataset_or_store, seed, epoch=0, device='cuda', strategy='random', filtered=False, shuffle=True):
    """KG quadruples sampled ON THE GPU: int64 [E, 4] CUDA tensor (h, t+, t-, relation id), the columns kg_loss of CFKG, KGAT
    and KGCN reads, from one launch of csrc/kg_sampler.hip -- the epoch shuffle included (a keyed bijection of the row index:
    no randperm, no second table).  strategy 'random': t- uniform over all nodes, the reference's distribution
    (datasets/movielens.py:861-877); 'typed': uniform over the node block of the relation's tails.  filtered: a draw equal to
    t+ or completing a known triple of the relation is redrawn (up to 64 times; the store caches the key table).  `epoch`
    is the Philox counter's fourth word: an independent draw and shuffle per epoch.  Takes a dataset (its store is built
    on first use and kept at dataset.kg_store) or a kg_triple_store; sets train_data, train_data_length and
    negatives_exhausted on it."""
    from .. import _lib
    if strategy not in ('random', 'typed'):
        raise NotImplementedError('strategy %r (random or typed)' % (strategy,))
    if not isinstance(dataset_or_store, KGTripleStore):
        _lib.require_device()
    store = _store_of(dataset_or_store, device)
    # what the launch cannot check for itself (the tables are device memory): the host copies answer for them
    host = store.host
    if (np.diff(host['seg_ptr']) < 0).any() or host['seg_ptr'][0] != 0 or host['seg_ptr'][-1] != store.num_triples:
        raise ValueError('kg triple store: seg_ptr must rise from 0 to the number of triples')
    if (host['seg_n'] < 1).any() or (host['seg_n'] >= 2 ** 32).any():
        raise ValueError('kg triple store: a seg_n is outside [1, 2^32)')
    lib = _lib.require_device()
    lo, cnt = (store.seg_lo, store.seg_n) if strategy == 'typed' else (store.any_lo, store.any_n)
    keys = store.keys() if filtered and store.num_triples else None
    out = torch.empty((store.num_triples, 4), dtype=torch.int64, device=store.device)
    exhausted = torch.zeros(1, dtype=torch.int32, device=store.device)
    _lib.check(lib.pea_kg_sample(store.num_triples, _lib.ptr(store.heads), _lib.ptr(store.tails), store.num_segments,
                                 _lib.ptr(store.seg_ptr), _lib.ptr(store.seg_rel), _lib.ptr(lo), _lib.ptr(cnt), store.num_nodes,
                                 _lib.ptr(keys), 0 if keys is None else keys.numel(), int(seed) & (2 ** 64 - 1),
                                 int(epoch) & 0xFFFFFFFF, int(bool(shuffle)), _lib.ptr(out),
                                 out.stride(0), _lib.ptr(exhausted), _lib.current_stream()))
    n_exhausted = int(exhausted.item())
    if n_exhausted:
        # 64 rejection attempts all hit known triples (a head linked to nearly its whole block): the row keeps a known tail
        # as its negative.  Loud, because such a row is a false negative.
        import warnings
        warnings.warn('device_kg_negative_sampling: %d of %d negatives are known triples (rejection sampling exhausted)'
                      % (n_exhausted, out.shape[0]), RuntimeWarning)
    for target in {id(dataset_or_store): dataset_or_store, id(store): store}.values():
        target.negatives_exhausted = n_exhausted
        target.train_data, target.train_data_length = out, out.shape[0]
    return out


def device_shuffle_rows(rows, seed, epoch=0):
    """A shuffled copy of a contiguous int64 [n, w] CUDA tensor (w in 1..16): out[perm(i)] = rows[i] with the keyed bijection
    of csrc/kg_sampler.hip, one launch, no randperm and no index tensor.  The shuffle the device BPR triples
    (device_negative_sampling(..., shuffle=False)) and HeRec's labelled rows can opt into."""
    from .. import _lib
    lib = _lib.require_device()
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 2 and rows.is_contiguous()):
        raise ValueError('device_shuffle_rows: a contiguous int64 [n, w] CUDA tensor expected')
    if not 1 <= rows.shape[1] <= _lib.PERMUTE_MAX_WIDTH:
        raise ValueError('device_shuffle_rows: %d columns (1..%d)' % (rows.shape[1], _lib.PERMUTE_MAX_WIDTH))
    out = torch.empty_like(rows)
    _lib.check(lib.pea_permute_rows(rows.shape[0], rows.shape[1], _lib.ptr(rows), rows.stride(0), _lib.ptr(out), out.stride(0),
                                    int(seed) & (2 ** 64 - 1), int(epoch) & 0xFFFFFFFF, _lib.current_stream()))
    return out


# ---- the CF epoch table from one launch (csrc/cf_sampler.hip, include/peahip_cf_sample.h): BPR, BCE and entity-aware rows.  An
# ---- addition next to cf_negative_sampling / entity_aware_row / device_negative_sampling above, never their replacement.
_NO_ENTITY_LISTS = ('entity_aware=True needs dataset.iid_feat_nids / uid_feat_nids / nid2e_dict '
                    '(built by the reference\'s dataset preprocessing); attach them to the dataset')


class EntityStore:
    """The entity lists of a dataset laid out for pea_cf_sample: CSR (item_ptr [num_iids + 1], item_ent) and (user_ptr
    [num_uids + 1], user_ent) of the entity node ids of every item and user, and the node-type blocks (block_lo ascending,
    block_n) an entity's negative is drawn from.  `host` holds the numpy copies of the six tables."""

    def __init__(self, item_ptr, item_ent, user_ptr, user_ent, block_lo, block_n, block_types, device):
        self.host = {'item_ptr': item_ptr, 'item_ent': item_ent, 'user_ptr': user_ptr, 'user_ent': user_ent,
                     'block_lo': block_lo, 'block_n': block_n}
        self.block_types = list(block_types)
        self.nnz_i, self.nnz_u = int(item_ent.size), int(user_ent.size)
        # an empty list table still gets a word, so that its pointer is not null (all four tables are given, or none)
        to = lambda a: torch.as_tensor(np.ascontiguousarray(a if a.size else np.zeros(1), dtype=np.int64)).to(device)
        self.item_ptr, self.item_ent, self.user_ptr, self.user_ent = to(item_ptr), to(item_ent), to(user_ptr), to(user_ent)
        self.block_lo, self.block_n = to(block_lo), to(block_n)
        self.device = self.item_ptr.device

    @property
    def num_blocks(self):
        return int(self.host['block_lo'].size)


def _csr_of_lists(lists, n, what):
    if len(lists) != n:
        raise ValueError('entity_store: %s has %d lists for %d owners' % (what, len(lists), n))
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    ids = np.fromiter((v for l in lists for v in l), dtype=np.int64, count=int(ptr[-1]))
    return ptr, ids


def entity_store(dataset, device='cuda'):
    """The EntityStore of a dataset, built once and kept at dataset.entity_store, from the reference's attributes
    (datasets/movielens.py:941-991): iid_feat_nids / uid_feat_nids (one list of entity node ids per item / user), nid2e_dict
    (node id -> (type, ...)), type_accs and num_<type>s.  Checks on the host what the launch cannot: every listed id lies in
    the block [type_accs[t], type_accs[t] + num_<t>s) of its nid2e_dict type, the blocks are disjoint (kept ascending) and at
    most 64.  ValueError otherwise; NotImplementedError when the lists are absent."""
    from .. import _lib
    want = torch.empty(0, device=device).device
    store = getattr(dataset, 'entity_store', None)
    if isinstance(store, EntityStore) and store.device == want:
        return store
    if not all(hasattr(dataset, a) for a in ('iid_feat_nids', 'uid_feat_nids', 'nid2e_dict')):
        raise NotImplementedError(_NO_ENTITY_LISTS)
    item_ptr, item_ent = _csr_of_lists(dataset.iid_feat_nids, int(dataset.num_iids), 'iid_feat_nids')
    user_ptr, user_ent = _csr_of_lists(dataset.uid_feat_nids, int(dataset.num_uids), 'uid_feat_nids')
    if max(item_ent.size, user_ent.size) >= 2 ** 32:
        raise ValueError('entity_store: 2^32 or more list entries')
    # the blocks of every node type the dataset sizes (num_<type>s), ascending
    blocks = sorted((int(lo), int(getattr(dataset, 'num_%ss' % t)), t) for t, lo in dataset.type_accs.items()
                    if hasattr(dataset, 'num_%ss' % t))
    if not 1 <= len(blocks) <= _lib.CF_MAX_BLOCKS:
        raise ValueError('entity_store: %d node-type blocks (1..%d)' % (len(blocks), _lib.CF_MAX_BLOCKS))
    for k, (lo, cnt, t) in enumerate(blocks):
        if lo < 0 or not 1 <= cnt < 2 ** 32:
            raise ValueError('entity_store: block (%d, %d) of %r' % (lo, cnt, t))
        if k and lo < blocks[k - 1][0] + blocks[k - 1][1]:
            raise ValueError('entity_store: the blocks of %r and %r overlap' % (blocks[k - 1][2], t))
    span = {t: (lo, lo + cnt) for lo, cnt, t in blocks}
    for e in np.unique(np.concatenate([item_ent, user_ent])).tolist():
        entry = dataset.nid2e_dict.get(e)
        if entry is None or entry[0] not in span:
            raise ValueError('entity_store: entity %d has no sized node type in nid2e_dict' % e)
        lo, hi = span[entry[0]]
        if not lo <= e < hi:
            raise ValueError('entity_store: entity %d lies outside the block [%d, %d) of its type %r' % (e, lo, hi, entry[0]))
    store = EntityStore(item_ptr, item_ent, user_ptr, user_ent, np.asarray([b[0] for b in blocks], dtype=np.int64),
                        np.asarray([b[1] for b in blocks], dtype=np.int64), [b[2] for b in blocks], device)
    dataset.entity_store = store
    return store


def device_cf_negative_sampling(dataset, seed, epoch=0, device='cuda', shuffle=True):
    """The CF training table of an epoch sampled ON THE GPU by one launch of csrc/cf_sampler.hip, the epoch shuffle included (a
    keyed bijection of the row index: no randperm, no second table); int64 CUDA tensor.
        cf_loss_type 'BPR'                 [M k, 3]        (u, i+, i-): unshuffled, bitwise device_negative_sampling(shuffle=False)
        'BPR' with dataset.entity_aware    [M k, 9]        + (e+, e-, mask_i, f+, f-, mask_u), the columns entity_aware_row appends,
                                                           over entity_store(dataset)
        'BCE'                              [M (1 + k), 3]  (u, i+, 1) for every positive, then (u, i-, 0) k per positive
    sampling_strategy 'random': uniform items; 'unseen': uniform over the items the user has no training interaction with (64
    rejection attempts; a row they do not suffice for keeps a seen item, is counted in negatives_exhausted and warned about).
    `epoch` is the Philox counter's fourth word: an independent draw and shuffle per epoch.  Sets train_data,
    train_data_length and negatives_exhausted; a user or item id outside its block raises ValueError."""
    from .. import _lib
    mode = {'BPR': _lib.CF_BPR, 'BCE': _lib.CF_BCE}.get(dataset.cf_loss_type)
    if mode is None:
        raise NotImplementedError('only the BPR and BCE branches are on the accelerated path')
    if dataset.sampling_strategy not in ('random', 'unseen'):
        raise NotImplementedError('sampling_strategy %r (random or unseen)' % (dataset.sampling_strategy,))
    ent = bool(getattr(dataset, 'entity_aware', False))
    if ent and mode == _lib.CF_BCE:
        raise NotImplementedError('entity-aware rows exist in the BPR branch only (datasets/movielens.py:941-991)')
    store = entity_store(dataset, device) if ent else None
    lib = _lib.require_device()
    pos = torch.as_tensor(dataset.edge_index_nps['user2item']).to(device=device, dtype=torch.int64)
    pos_u, pos_i = pos[0].contiguous(), pos[1].contiguous()
    k = int(dataset.num_negative_samples)
    lo, n_items = int(dataset.type_accs['iid']), int(dataset.num_iids)
    u_lo, n_users = int(dataset.type_accs['uid']), int(dataset.num_uids)
    keys = torch.unique(pos_u * n_items + (pos_i - lo)) if dataset.sampling_strategy == 'unseen' else None       # ascending
    n_pos = pos_u.numel()
    out = torch.empty((n_pos * (k + 1 if mode == _lib.CF_BCE else k), 9 if ent else 3), dtype=torch.int64, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)              # exhausted, bad rows: one host read for both
    tables = [None, None, 0, None, None, 0, 0, None, None] if store is None else [
        _lib.ptr(store.item_ptr), _lib.ptr(store.item_ent), store.nnz_i, _lib.ptr(store.user_ptr), _lib.ptr(store.user_ent),
        store.nnz_u, store.num_blocks, _lib.ptr(store.block_lo), _lib.ptr(store.block_n)]
    _lib.check(lib.pea_cf_sample(n_pos, k, mode, _lib.ptr(pos_u), _lib.ptr(pos_i), lo, n_items, u_lo, n_users, _lib.ptr(keys),
                                 0 if keys is None else keys.numel(), *tables, int(seed) & (2 ** 64 - 1),
                                 int(epoch) & 0xFFFFFFFF, int(bool(shuffle)), _lib.ptr(out), out.stride(0), _lib.ptr(counts),
                                 _lib.ptr(counts[1:]), _lib.current_stream()))
    n_exhausted, n_bad = (int(v) for v in counts.tolist())
    if n_bad:
        raise ValueError('device_cf_negative_sampling: %d of %d rows carry a user or item id outside its block (or an entity '
                         'list outside its table)' % (n_bad, out.shape[0]))
    if n_exhausted:
        # 'unseen': 64 rejection attempts all hit seen items (a user who has rated nearly every item); the row keeps
        # a seen item as its negative.  Loud, because such a row is a false negative.
        import warnings
        warnings.warn('device_cf_negative_sampling: %d of %d negatives are seen items (rejection sampling exhausted)'
                      % (n_exhausted, out.shape[0]), RuntimeWarning)
    dataset.negatives_exhausted = n_exhausted
    dataset.train_data, dataset.train_data_length = out, out.shape[0]
    return out
