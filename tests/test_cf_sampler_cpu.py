"""CPU: the on-device CF epoch sampler without a device -- the numpy restatement of its streams (tests/cf_sampler_ref.py: the
entity columns have the properties of utils.entity_aware_row, the BCE rows the reference's layout, 'unseen' draws hit no
training pair), the seventh header (include/peahip_cf_sample.h) against _lib.CF_SAMPLE_SIGNATURES and the library's exports,
every argument error of the entry point (returned before anything is launched), utils.entity_store's checks and
SyntheticHIN.entity_lists."""
import os
import re

import numpy as np
import pytest

import cf_sampler_ref as ref
from graph_recsys_benchmark_amd import _lib
from graph_recsys_benchmark_amd.utils import SyntheticHIN, device_cf_negative_sampling, entity_store
from test_cfkg_cpu import case_id, ctypes_width, fake, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
# Any seed serves the coverage test below: a member of a list of 3 is missed by 40 rows with probability (2 / 3)^40 < 1e-7.
# This one has a non-zero high word, and the restatement was run with it: every such member is drawn.
SEED = (7 << 32) | 2020


# ---------------------------------------------------------------- the entity columns
@pytest.fixture(scope='module')
def entity_rows():
    ds = ref.EntityDataset()
    table, exhausted, bad, _ = ref.sample_dataset(ds, SEED, offset=3)
    assert exhausted == 0 and bad == 0 and table.dtype == np.int64
    return ds, table


def test_entity_columns_have_the_properties_of_entity_aware_row(entity_rows):
    ds, table = entity_rows
    pos = ds.edge_index_nps['user2item'].astype(np.int64)
    assert table.shape == (pos.shape[1] * 4, 9)
    assert np.array_equal(table[:, 0], np.repeat(pos[0], 4)) and np.array_equal(table[:, 1], np.repeat(pos[1], 4))
    seen_empty = seen_full = 0
    for row in table.tolist():
        for owner, feats_of, cols in ((row[1] - ds.type_accs['iid'], ds.iid_feat_nids, row[3:6]),
                                      (row[0] - ds.type_accs['uid'], ds.uid_feat_nids, row[6:9])):
            feats = feats_of[owner]
            if not feats:
                assert cols == [0, 0, 0]
                seen_empty += 1
                continue
            e_pos, e_neg, mask = cols
            assert mask == 1 and e_pos in feats
            lower = ds.type_accs[ds.nid2e_dict[e_pos][0]]
            assert lower <= e_neg < lower + getattr(ds, 'num_' + ds.nid2e_dict[e_pos][0] + 's')
            seen_full += 1
    assert seen_empty > 100 and seen_full > 1000                      # both branches were walked


def test_every_member_of_a_short_list_is_drawn(entity_rows):
    ds, table = entity_rows
    checked = 0
    for col, first, lo, feats_of in ((1, 3, ds.type_accs['iid'], ds.iid_feat_nids), (0, 6, ds.type_accs['uid'], ds.uid_feat_nids)):
        for owner, feats in enumerate(feats_of):
            rows = table[table[:, col] == lo + owner]
            if 1 <= len(feats) <= 3 and rows.shape[0] >= 40:
                assert set(rows[:, first].tolist()) == set(feats), (col, owner)
                checked += 1
    assert checked >= 30
    assert len(np.unique(table[table[:, 5] == 1, 4])) == 14          # and the negatives reach every entity of both blocks


def test_epochs_and_seeds_give_other_entity_draws(entity_rows):
    ds, table = entity_rows
    again, _, _, _ = ref.sample_dataset(ds, SEED, offset=3)
    other, _, _, _ = ref.sample_dataset(ds, SEED, offset=4)
    assert np.array_equal(again, table) and np.array_equal(other[:, :2], table[:, :2])
    assert (other[:, 2] != table[:, 2]).mean() > 0.9 and (other[:, 4] != table[:, 4]).mean() > 0.4
    shuffled, _, _, _ = ref.sample_dataset(ds, SEED, offset=3, shuffle=True)
    assert np.array_equal(shuffled[ref.perm(table.shape[0], SEED, 3)], table)


# ---------------------------------------------------------------- the BCE rows and the negatives
@pytest.mark.parametrize('strategy', ['random', 'unseen'])
def test_bce_layout(strategy):
    ds = ref.SmallDataset(100, k=4, loss='BCE', strategy=strategy, seed=1)
    u, i = ds.positives()
    table, exhausted, bad, _ = ref.sample_dataset(ds, SEED, offset=1)
    assert table.shape == (500, 3) and exhausted == 0 and bad == 0
    assert np.array_equal(table[:100], np.stack([u, i, np.ones(100, dtype=np.int64)], axis=1))
    assert np.array_equal(table[100:, 0], np.repeat(u, 4)) and (table[100:, 2] == 0).all()
    assert ((table[100:, 1] >= 15) & (table[100:, 1] < 35)).all() and len(np.unique(table[100:, 1])) == 20
    # negative j draws with counter j, whatever the loss: the BPR table of the same positives has the same negatives
    ds.cf_loss_type = 'BPR'
    bpr, _, _, _ = ref.sample_dataset(ds, SEED, offset=1)
    assert np.array_equal(bpr[:, 2], table[100:, 1]) and np.array_equal(bpr[:, 0], table[100:, 0])


@pytest.mark.parametrize('loss', ['BPR', 'BCE'])
def test_unseen_negatives_hit_no_training_pair(loss):
    ds = ref.SmallDataset(120, k=4, loss=loss, strategy='unseen', seed=2)
    u, i = ds.positives()
    keys = ref.seen_keys(u, i, 15, 20)
    table, exhausted, _, _ = ref.sample_dataset(ds, SEED)
    neg_u, neg_i = (table[:, 0], table[:, 2]) if loss == 'BPR' else (table[120:, 0], table[120:, 1])
    assert exhausted == 0 and not np.isin(neg_u * 20 + (neg_i - 15), keys).any()
    ds.sampling_strategy = 'random'
    plain, _, _, _ = ref.sample_dataset(ds, SEED)
    plain_i = plain[:, 2] if loss == 'BPR' else plain[120:, 1]
    hit = np.isin(neg_u * 20 + (plain_i - 15), keys)
    assert hit.any() and np.array_equal(neg_i[~hit], plain_i[~hit])   # the plain stream does hit; the other rows kept their first draw


@pytest.mark.parametrize('loss', ['BPR', 'BCE'])
def test_a_user_who_has_seen_every_item_exhausts_exactly_its_rows(loss):
    ds = ref.SmallDataset(100, k=4, loss=loss, strategy='unseen', seed=3, full_user=True)
    u, _ = ds.positives()
    table, exhausted, bad, which = ref.sample_dataset(ds, SEED)
    want = np.repeat(u, 4) == 0
    assert want.sum() == 80 and exhausted == 80 and bad == 0 and np.array_equal(which, want)
    neg = table[:, 2] if loss == 'BPR' else table[u.size:, 1]
    assert ((neg >= 15) & (neg < 35)).all()


def test_ids_outside_their_block_are_bad_rows_and_draw_nothing():
    ds = ref.SmallDataset(50, k=2, entity_aware=True, seed=4)
    ds.edge_index_nps['user2item'][1, 7] = 35                          # one past the item block
    ds.edge_index_nps['user2item'][0, 9] = 15                          # one past the user block
    table, _, bad, _ = ref.sample_dataset(ds, SEED)
    assert bad == 4
    for r in (14, 15, 18, 19):
        assert table[r, 2] == 15 and (table[r, 3:] == 0).all()
    ds.cf_loss_type, ds.entity_aware = 'BCE', False
    assert ref.sample_dataset(ds, SEED)[2] == 2 + 2                    # the two positives, and the two negatives of the bad user


# ---------------------------------------------------------------- the seventh header
def test_seventh_header_matches_its_ctypes_table():
    protos = prototypes('peahip_cf_sample.h')
    assert sorted(protos) == sorted(_lib.CF_SAMPLE_SIGNATURES) == ['pea_cf_sample']
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.CF_SAMPLE_SIGNATURES[name]
        assert len(argtypes) == len(params) == 28
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    tables = (_lib.SIGNATURES, _lib.KGE_SIGNATURES, _lib.EVAL_SIGNATURES, _lib.SAMPLE_SIGNATURES, _lib.FM_SIGNATURES,
              _lib.FM_EVAL_SIGNATURES)
    assert len(_lib.SIGNATURES) == 112
    assert not set().union(*[set(t) for t in tables]) & set(_lib.CF_SAMPLE_SIGNATURES)
    headers = ('peahip.h', 'peahip_kge.h', 'peahip_eval.h', 'peahip_sample.h', 'peahip_fm.h', 'peahip_fm_eval.h')
    assert not set().union(*[set(prototypes(h)) for h in headers]) & set(protos)
    text = open(os.path.join(ROOT, 'include', 'peahip_cf_sample.h')).read()
    for name, value in (('PEA_CF_MAX_BLOCKS', _lib.CF_MAX_BLOCKS), ('PEA_CF_BPR', _lib.CF_BPR), ('PEA_CF_BCE', _lib.CF_BCE)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), text), name
    assert _lib.CF_MAX_BLOCKS == 64


# ---------------------------------------------------------------- argument errors
ENT = dict(item_ptr=fake(), item_ent=fake(), user_ptr=fake(), user_ent=fake(), n_blocks=3, block_lo=fake(), block_n=fake(), ld_out=9)


def sample_call(**over):
    a = dict(n=100, k=4, mode=0, pos_u=fake(), pos_i=fake(), item_lo=15, num_items=20, user_lo=0, num_users=15, keys=None, n_keys=0,
             item_ptr=None, item_ent=None, nnz_i=10, user_ptr=None, user_ent=None, nnz_u=10, n_blocks=0, block_lo=None,
             block_n=None, seed=1, offset=0, shuffle=1, out=fake(), ld_out=3, exhausted=fake(), bad_rows=fake(), stream=None)
    a.update(over)
    return _lib.load().pea_cf_sample(a['n'], a['k'], a['mode'], a['pos_u'], a['pos_i'], a['item_lo'], a['num_items'], a['user_lo'],
                                     a['num_users'], a['keys'], a['n_keys'], a['item_ptr'], a['item_ent'], a['nnz_i'], a['user_ptr'],
                                     a['user_ent'], a['nnz_u'], a['n_blocks'], a['block_lo'], a['block_n'], a['seed'], a['offset'],
                                     a['shuffle'], a['out'], a['ld_out'], a['exhausted'], a['bad_rows'], a['stream'])


BAD = [dict(pos_u=None), dict(pos_i=None), dict(out=None), dict(exhausted=None), dict(bad_rows=None),
       dict(k=0), dict(k=-1), dict(mode=2), dict(mode=-1), dict(ld_out=2), dict(ld_out=0), dict(ENT, ld_out=8),
       dict(num_items=0), dict(num_items=1 << 32), dict(num_items=-3), dict(num_users=0), dict(num_users=1 << 32),
       dict(item_lo=-1), dict(user_lo=-1),
       dict(ENT, n_blocks=0), dict(ENT, n_blocks=65), dict(ENT, n_blocks=-1), dict(ENT, block_lo=None), dict(ENT, block_n=None),
       dict(ENT, item_ptr=None), dict(ENT, item_ent=None), dict(ENT, user_ptr=None), dict(ENT, user_ent=None),
       dict(item_ptr=fake()), dict(user_ent=fake()), dict(ENT, user_ptr=None, user_ent=None),
       dict(ENT, mode=1), dict(ENT, nnz_i=-1), dict(ENT, nnz_u=1 << 32),
       dict(n_keys=7), dict(n_keys=-1, keys=fake()),
       dict(keys=fake(), n_keys=5, user_lo=1 << 40, num_items=1 << 23),          # 2^40 * 2^23 == 2^63
       dict(n=-1), dict(shuffle=2), dict(shuffle=-1),
       dict(n=1 << 39, k=1), dict(n=1 << 37, k=3, mode=1), dict(n=1 << 62, k=1 << 30)]            # more rows than the grid holds


@pytest.mark.parametrize('over', BAD, ids=[case_id(o) + ('#%d' % i) for i, o in enumerate(BAD)])
def test_argument_errors_need_no_device(over):
    assert sample_call(**over) == ERR_ARG
    assert _lib.last_error()


def test_nothing_to_do_is_ok_without_a_device():
    assert sample_call(n=0) == 0 and sample_call(n=0, mode=1) == 0 and sample_call(n=0, **ENT) == 0
    assert sample_call(n=0, pos_u=None, pos_i=None, out=None, exhausted=None, bad_rows=None) == 0
    assert sample_call(n=0, keys=fake(), n_keys=5, user_lo=(1 << 40) - 15, num_users=14, num_items=1 << 23) == 0      # below 2^63


# ---------------------------------------------------------------- the host layers
def test_entity_store_tables():
    ds = ref.SmallDataset(10)
    store = entity_store(ds, device='cpu')
    assert ds.entity_store is store and entity_store(ds, device='cpu') is store       # built once
    item_ptr, item_ent, user_ptr, user_ent, block_lo, block_n = ds.entity_tables()
    for name, want in (('item_ptr', item_ptr), ('item_ent', item_ent), ('user_ptr', user_ptr), ('user_ent', user_ent),
                       ('block_lo', block_lo), ('block_n', block_n)):
        assert store.host[name].dtype == np.int64 and np.array_equal(store.host[name], want), name
        assert np.array_equal(getattr(store, name).numpy(), want), name
    assert store.block_types == ['uid', 'iid', 'genre', 'tid', 'year'] and store.num_blocks == 5
    assert (store.nnz_i, store.nnz_u) == (item_ent.size, user_ent.size) and item_ptr[1] == 300
    ds = ref.SmallDataset(10)
    ds.uid_feat_nids = [[] for _ in range(15)]                         # no user entity at all: the table still has an address
    store = entity_store(ds, device='cpu')
    assert store.nnz_u == 0 and store.user_ent.numel() == 1 and store.host['user_ent'].size == 0


def test_entity_store_refusals():
    def broken(change):
        ds = ref.SmallDataset(10)
        change(ds)
        return ds

    def without_lists(ds):
        del ds.iid_feat_nids

    def without_dict(ds):
        del ds.nid2e_dict

    with pytest.raises(NotImplementedError, match='entity_aware=True needs dataset.iid_feat_nids'):
        entity_store(broken(without_lists), device='cpu')
    with pytest.raises(NotImplementedError):
        entity_store(broken(without_dict), device='cpu')
    cases = {
        'an entity outside the block of its type': lambda ds: ds.iid_feat_nids[3].append(40) or ds.nid2e_dict.update({40: ('genre', 5)}),
        'an entity one past the last block': lambda ds: ds.uid_feat_nids[2].append(50) or ds.nid2e_dict.update({50: ('year', 1)}),
        'an entity nid2e_dict does not know': lambda ds: ds.iid_feat_nids[0].append(77),
        'an entity of a type without a size': lambda ds: ds.nid2e_dict.update({49: ('decade', 0)}),
        'overlapping blocks': lambda ds: setattr(ds, 'num_genres', 6),
        'an empty block': lambda ds: setattr(ds, 'num_years', 0),
        'a list short': lambda ds: ds.uid_feat_nids.pop(),
        'too many blocks': lambda ds: [ds.type_accs.update({'t%d' % j: 100 + j}) or setattr(ds, 'num_t%ds' % j, 1) for j in range(60)],
    }
    for what, change in cases.items():
        with pytest.raises(ValueError):
            entity_store(broken(change), device='cpu')
            pytest.fail('accepted: ' + what)
    ds = broken(lambda ds: [ds.type_accs.update({'t%d' % j: 100 + j}) or setattr(ds, 'num_t%ds' % j, 1) for j in range(59)])
    assert entity_store(ds, device='cpu').num_blocks == 64             # 64 blocks are still taken


def test_device_cf_negative_sampling_refuses_before_it_needs_a_device():
    for change in (dict(cf_loss_type='WARP'), dict(sampling_strategy='popular'), dict(cf_loss_type='BCE', entity_aware=True)):
        ds = ref.SmallDataset(10)
        for name, value in change.items():
            setattr(ds, name, value)
        with pytest.raises(NotImplementedError):
            device_cf_negative_sampling(ds, seed=1, device='cpu')
    ds = ref.SmallDataset(10, entity_aware=True)
    del ds.uid_feat_nids
    with pytest.raises(NotImplementedError, match='entity_aware=True needs'):
        device_cf_negative_sampling(ds, seed=1, device='cpu')


def test_synthetic_entity_lists():
    ds = SyntheticHIN('ml_small')
    items, users = ds.entity_lists()
    assert items is ds.iid_feat_nids and users is ds.uid_feat_nids and len(items) == ds.num_iids and len(users) == ds.num_uids
    rel = ds.edge_index_nps
    to_item = [n for n in rel if n.endswith('2item') and n != 'user2item']
    to_user = [n for n in rel if n.endswith('2user')]
    assert len(to_item) == 6 and to_user == ['tag2user']
    assert sum(len(l) for l in items) == sum(rel[n].shape[1] for n in to_item)
    assert sum(len(l) for l in users) == sum(rel[n].shape[1] for n in to_user)
    year = range(ds.type_accs['year'], ds.type_accs['year'] + ds.num_years)
    assert all(sum(e in year for e in l) == 1 for l in items)          # every item has its year
    # relation by relation, each in edge order: item 5's list against a plain loop
    want = [int(s) for n in to_item for s, d in rel[n].T if int(d) == ds.type_accs['iid'] + 5]
    assert items[5] == want and len(want) >= 1
    assert ds.num_genres == 19 and ds.num_tids == 42 and ds.num_uids == 608
    assert set(ds.nid2e_dict) == set(range(ds.type_accs['genre'], ds.num_nodes))
    assert all(ds.type_accs[t] + j == e for e, (t, j) in ds.nid2e_dict.items())
    store = entity_store(ds, device='cpu')                             # and the lists pass the store's checks
    assert store.nnz_i == sum(len(l) for l in items) and store.num_blocks == 8
    before = ([list(l) for l in items], [list(l) for l in users], dict(ds.nid2e_dict))
    again = ds.entity_lists()
    assert again[0] is items and again[1] is users and (items, users, ds.nid2e_dict) == before
