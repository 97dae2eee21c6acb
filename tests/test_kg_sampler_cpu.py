"""CPU: the on-device KG triple sampler without a device -- the numpy restatement of its streams (tests/kg_sampler_ref.py: the
keyed bijection is a permutation, the rows have the store's columns, filtered draws complete no known triple), the fourth
header (include/peahip_sample.h) against _lib.SAMPLE_SIGNATURES and the library's exports, every argument error of the two
entry points (returned before anything is launched), and kg_triple_store against the reference-recorded table of
tests/golden/cfkg_small.npz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cfkg_ref
import kg_sampler_ref as ref
from graph_recsys_benchmark_amd import _lib
from graph_recsys_benchmark_amd.utils import device_kg_negative_sampling, kg_triple_store
from test_cfkg_cpu import case_id, ctypes_width, fake, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SEED = (7 << 32) | 2020


# ---------------------------------------------------------------- the shuffle
@pytest.mark.parametrize('ns', [range(1, 300), (4096, 4097), (65536, 65537)], ids=['1..299', '4096,4097', '65536,65537'])
def test_perm_is_a_permutation(ns):
    for n in ns:
        p = ref.perm(n, SEED, 3)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n)), n


def test_offsets_and_seeds_give_different_permutations():
    a, b, c = ref.perm(4097, SEED, 0), ref.perm(4097, SEED, 1), ref.perm(4097, SEED + 1, 0)
    assert (a != b).mean() > 0.99 and (a != c).mean() > 0.99
    assert np.array_equal(a, ref.perm(4097, SEED, 0))
    assert (a != np.arange(4097)).mean() > 0.99


def test_walk_length():
    """2^(2 hb) < 4 n, so a pass lands below n with probability above 1 / 4: the mean walk is at most 4 passes"""
    for n in (257, 4097, 65537):
        _, passes = ref.perm(n, SEED, 3, return_passes=True)
        assert passes.min() >= 1 and passes.mean() <= 4.0, n
        assert (1 << (2 * ref.half_bits(n))) < 4 * n or n < 3


# ---------------------------------------------------------------- the draws
def small_graph(seed=0, full_head=False):
    """3 relations over 40 nodes (users 0..14, items 15..34, attributes 35..39), 200 triples; full_head: user 0 is linked to
    every item as well.  Returns (heads, tails, seg_ptr, seg_rel, typed seg_lo, typed seg_n, N)."""
    rng = np.random.default_rng(seed)
    u2i = np.stack([rng.integers(0, 15, 120), rng.integers(15, 35, 120)])
    if full_head:
        u2i[0, u2i[0] == 0] = 1
        u2i = np.concatenate([np.stack([np.zeros(20, dtype=np.int64), np.arange(15, 35)]), u2i[:, :100]], axis=1)
    a2i = np.stack([rng.integers(35, 40, 50), rng.integers(15, 35, 50)])
    a2u = np.stack([rng.integers(35, 40, 30), rng.integers(0, 15, 30)])
    parts = [u2i, a2i, a2u]
    heads, tails = (np.concatenate([p[k] for p in parts]).astype(np.int64) for k in (0, 1))
    seg_ptr = np.cumsum([0] + [p.shape[1] for p in parts])
    return heads, tails, seg_ptr, np.array([4, 0, 2]), np.array([15, 15, 0]), np.array([20, 20, 15]), 40


def test_rows_have_the_store_columns():
    heads, tails, seg_ptr, seg_rel, lo, cnt, n = small_graph()
    assert heads.size == 200
    rel = seg_rel[ref.segment_of_rows(seg_ptr)]
    for strategy, (s_lo, s_n) in {'random': (np.zeros(3, dtype=np.int64), np.full(3, n)), 'typed': (lo, cnt)}.items():
        rows, exhausted, _ = ref.sample(heads, tails, seg_ptr, seg_rel, s_lo, s_n, n, seed=SEED, offset=3)
        assert exhausted == 0 and rows.dtype == np.int64 and rows.shape == (200, 4)
        assert np.array_equal(rows[:, 0], heads) and np.array_equal(rows[:, 1], tails) and np.array_equal(rows[:, 3], rel)
        seg = ref.segment_of_rows(seg_ptr)
        assert ((rows[:, 2] >= s_lo[seg]) & (rows[:, 2] < s_lo[seg] + s_n[seg])).all(), strategy
        shuffled, _, _ = ref.sample(heads, tails, seg_ptr, seg_rel, s_lo, s_n, n, seed=SEED, offset=3, shuffle=True)
        assert np.array_equal(shuffled[ref.perm(200, SEED, 3)], rows)
    typed, _, _ = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, n, seed=SEED, offset=3)
    assert len(np.unique(typed[:120, 2])) > 10                       # and it does draw: not one id


@pytest.mark.parametrize('strategy', ['random', 'typed'])
def test_filtered_draws_complete_no_known_triple(strategy):
    heads, tails, seg_ptr, seg_rel, lo, cnt, n = small_graph()
    if strategy == 'random':
        lo, cnt = np.zeros(3, dtype=np.int64), np.full(3, n)
    keys = ref.known_keys(heads, tails, seg_ptr, n)
    rows, exhausted, _ = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, n, keys=keys, seed=SEED, offset=3)
    assert exhausted == 0
    seg = ref.segment_of_rows(seg_ptr)
    assert not (rows[:, 2] == rows[:, 1]).any()
    assert not np.isin((seg * n + rows[:, 0]) * n + rows[:, 2], keys).any()
    plain, _, _ = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, n, seed=SEED, offset=3)
    hit = np.isin((seg * n + plain[:, 0]) * n + plain[:, 2], keys)
    assert hit.any() and np.array_equal(rows[~hit], plain[~hit])   # the unfiltered stream does hit; the other rows kept their first draw


def test_a_head_linked_to_its_whole_block_exhausts_exactly_its_rows():
    heads, tails, seg_ptr, seg_rel, lo, cnt, n = small_graph(full_head=True)
    keys = ref.known_keys(heads, tails, seg_ptr, n)
    rows, exhausted, which = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, n, keys=keys, seed=SEED, offset=3)
    want = (heads == 0) & (ref.segment_of_rows(seg_ptr) == 0)
    assert want.sum() == 20 and exhausted == 20 and np.array_equal(which, want)
    assert ((rows[want, 2] >= 15) & (rows[want, 2] < 35)).all()


# ---------------------------------------------------------------- the fourth header
def test_fourth_header_matches_its_ctypes_table():
    protos = prototypes('peahip_sample.h')
    assert sorted(protos) == sorted(_lib.SAMPLE_SIGNATURES) == ['pea_kg_sample', 'pea_permute_rows']
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.SAMPLE_SIGNATURES[name]
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    others = set(prototypes('peahip.h')) | set(prototypes('peahip_kge.h')) | set(prototypes('peahip_eval.h'))
    assert not others & set(protos)
    assert not (set(_lib.SIGNATURES) | set(_lib.KGE_SIGNATURES) | set(_lib.EVAL_SIGNATURES)) & set(_lib.SAMPLE_SIGNATURES)
    text = open(os.path.join(ROOT, 'include', 'peahip_sample.h')).read()
    for name, value in (('PEA_KG_MAX_SEGMENTS', _lib.KG_MAX_SEGMENTS), ('PEA_PERMUTE_MAX_WIDTH', _lib.PERMUTE_MAX_WIDTH)):
        assert re.search(r'#define\s+%s\s+%d\b' % (name, value), text), name


# ---------------------------------------------------------------- argument errors
def sample_call(**over):
    a = dict(n=100, heads=fake(), tails=fake(), n_seg=3, seg_ptr=fake(), seg_rel=fake(), seg_lo=fake(), seg_n=fake(), num_nodes=50,
             keys=None, n_keys=0, seed=1, offset=0, shuffle=1, out=fake(), ld_out=4, exhausted=fake(), stream=None)
    a.update(over)
    return _lib.load().pea_kg_sample(a['n'], a['heads'], a['tails'], a['n_seg'], a['seg_ptr'], a['seg_rel'], a['seg_lo'], a['seg_n'],
                                     a['num_nodes'], a['keys'], a['n_keys'], a['seed'], a['offset'], a['shuffle'], a['out'],
                                     a['ld_out'], a['exhausted'], a['stream'])


BAD_SAMPLE = [dict(heads=None), dict(tails=None), dict(seg_ptr=None), dict(seg_rel=None), dict(seg_lo=None), dict(seg_n=None),
              dict(out=None), dict(exhausted=None), dict(ld_out=3), dict(ld_out=0), dict(n_seg=0), dict(n_seg=1025), dict(n_seg=-1),
              dict(num_nodes=0), dict(num_nodes=1 << 32), dict(num_nodes=-5), dict(n_keys=7), dict(n_keys=-1, keys=fake()),
              dict(n_seg=1024, num_nodes=(1 << 32) - 1, keys=fake(), n_keys=5),          # 2^10 * (2^32 - 1)^2 >= 2^63
              dict(n_seg=2, num_nodes=(1 << 31), keys=fake(), n_keys=5),                 # 2 * 2^62 == 2^63
              dict(n=-1), dict(shuffle=2), dict(shuffle=-1)]


@pytest.mark.parametrize('over', BAD_SAMPLE, ids=[case_id(o) + ('#%d' % i) for i, o in enumerate(BAD_SAMPLE)])
def test_kg_sample_argument_errors_need_no_device(over):
    assert sample_call(**over) == ERR_ARG
    assert _lib.last_error()


def permute_call(**over):
    buf = fake(1 << 16)
    a = dict(n=100, width=3, src=buf, ld_in=3, out=C.c_void_p(buf.value + 4096), ld_out=4, seed=1, offset=0, stream=None)
    a.update(over)
    return _lib.load().pea_permute_rows(a['n'], a['width'], a['src'], a['ld_in'], a['out'], a['ld_out'], a['seed'], a['offset'],
                                        a['stream'])


BAD_PERMUTE = [dict(src=None), dict(out=None), dict(width=0), dict(width=17), dict(width=-1), dict(ld_in=2), dict(ld_out=2),
               dict(n=-1), dict(n=1000)]        # the last: 1000 rows of stride 3 run into out, 4096 bytes on


@pytest.mark.parametrize('over', BAD_PERMUTE, ids=[case_id(o) + ('#%d' % i) for i, o in enumerate(BAD_PERMUTE)])
def test_permute_rows_argument_errors_need_no_device(over):
    assert permute_call(**over) == ERR_ARG
    assert _lib.last_error()


def test_permute_rows_refuses_the_same_table_in_place():
    buf = fake()
    assert permute_call(src=buf, out=buf) == ERR_ARG


def test_nothing_to_do_is_ok_without_a_device():
    assert sample_call(n=0) == 0 and sample_call(n=0, heads=None, tails=None, out=None, exhausted=None) == 0
    assert permute_call(n=0) == 0 and permute_call(n=0, src=None, out=None) == 0
    assert sample_call(n_seg=1023, num_nodes=(1 << 26), keys=fake(), n_keys=5, n=0) == 0     # 1023 * 2^52 < 2^63


# ---------------------------------------------------------------- the triple store
@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'cfkg_small.npz'))


def golden_dataset(z):
    names = [str(n) for n in z['kg.relations']]
    return cfkg_ref.FakeDataset(int(z['kg.num_nodes']), 1, 0, {n: z['kg.edge.' + n] for n in names})


def test_triple_store_has_the_rows_of_the_reference_table(golden):
    ds = golden_dataset(golden)
    store = kg_triple_store(ds, device='cpu')
    want = golden['kg.train_data_sorted'][:, [0, 1, 3]]               # the reference's table minus its negative column
    got = store.rows().numpy()
    assert got.dtype == np.int64 and store.num_triples == int(golden['kg.train_data_length'])
    assert np.array_equal(cfkg_ref.sorted_rows(got), cfkg_ref.sorted_rows(want))
    # store order: relation by relation in the order of edge_index_nps, each relation's edges in their own order
    names = list(ds.edge_index_nps)
    assert np.array_equal(store.host['seg_ptr'], np.cumsum([0] + [ds.edge_index_nps[n].shape[1] for n in names]))
    assert np.array_equal(store.host['seg_rel'], [ds.edge_type_dict[n] for n in names])
    assert np.array_equal(got[:, :2], np.hstack([ds.edge_index_nps[n] for n in names]).T.astype(np.int64))
    del ds.edge_type_dict                                              # typed by position, as kg_negative_sampling types them
    assert np.array_equal(kg_triple_store(ds, device='cpu').rows().numpy(), got)
    # one node type: the default block of every relation is the whole node range
    assert np.array_equal(store.host['seg_lo'], np.zeros(len(names))) and np.array_equal(store.host['seg_n'], np.full(len(names), ds.num_nodes))


def test_triple_store_blocks_and_refusals():
    ds = cfkg_ref.sampling_dataset()                                   # users 0..29, items 30..74, others 75..86
    ds.type_accs = {'uid': 0, 'iid': 30, 'other': 75}
    store = kg_triple_store(ds, device='cpu')
    assert store.host['seg_lo'].tolist() == [30, 30, 0] and store.host['seg_n'].tolist() == [45, 45, 30]
    keys = store.keys().numpy()
    assert np.array_equal(keys, ref.known_keys(store.heads.numpy(), store.tails.numpy(), store.host['seg_ptr'], ds.num_nodes))
    with pytest.raises(ValueError):
        kg_triple_store(ds, device='cpu', tail_blocks={'user2item': (30, 10), 'attr2item': (30, 45), 'attr2user': (0, 30)})
    ds.edge_index_nps['empty'] = np.zeros((2, 0))
    ds.edge_type_dict['empty'] = 3
    with_empty = kg_triple_store(ds, device='cpu')
    assert with_empty.host['seg_ptr'].tolist()[-2:] == [215, 215] and with_empty.num_segments == 4
    # what the launch cannot check (the tables are device memory) the host call checks first, without a device
    with_empty.host['seg_n'] = np.array([45, 45, 30, 0])
    with pytest.raises(ValueError):
        device_kg_negative_sampling(with_empty, seed=1)
    with_empty.host['seg_n'] = np.array([45, 45, 30, 1])
    with_empty.host['seg_ptr'] = np.array([0, 150, 140, 215, 215])
    with pytest.raises(ValueError):
        device_kg_negative_sampling(with_empty, seed=1)
    with pytest.raises(NotImplementedError):
        device_kg_negative_sampling(with_empty, seed=1, strategy='unseen')
