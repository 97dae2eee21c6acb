"""GPU: the on-device KG triple sampler and row shuffle (csrc/kg_sampler.hip, include/peahip_sample.h) against the numpy
restatement of their streams (tests/kg_sampler_ref.py) bit for bit, the properties the draws must have, and the table feeding
kg_loss of CFKG and KGAT and solvers.kg_epoch without a copy."""
import warnings

import numpy as np
import pytest
import torch

import kg_sampler_ref as ref
from graph_recsys_benchmark_amd import _lib, solvers
from graph_recsys_benchmark_amd.models import CFKGRecsysModel, KGATRecsysModel
from graph_recsys_benchmark_amd.utils import (SyntheticHIN, device_kg_negative_sampling, device_shuffle_rows, kg_graph_input,
                                              kg_triple_store)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED, EPOCH = (7 << 32) | 2020, 3          # a seed with a non-zero high word
NODES, BLOCK = 200, 50                     # four node blocks of 50


class Graph:
    """the dataset attributes kg_triple_store reads"""

    def __init__(self, num_nodes, relations, type_ids):
        self.num_nodes, self.type_accs = num_nodes, {'uid': 0}
        self.edge_index_nps = relations
        self.edge_type_dict = type_ids


def random_graph(n_triples, n_seg, seed):
    """n_triples over n_seg relations.  With 64 segments the first, a middle and the last one are empty (and, when the
    triples are few, others too); with 3, one of those three, chosen by the seed.  Tails of relation s lie in block s % 4;
    relation ids are not the segment indices.  Returns (Graph, tail_blocks)."""
    rng = np.random.default_rng(seed)
    ends = (0, n_seg // 2, n_seg - 1)
    empty = set(ends) if n_seg >= 8 else {ends[seed % 3]} if n_seg >= 3 else set()
    live = [s for s in range(n_seg) if s not in empty]
    cuts = np.sort(rng.integers(0, n_triples + 1, size=len(live) - 1))
    sizes = dict(zip(live, np.diff(np.concatenate([[0], cuts, [n_triples]]))))
    rel, blocks, types = {}, {}, {}
    for s in range(n_seg):
        e = int(sizes.get(s, 0))
        lo = BLOCK * (s % 4)
        name = 'rel%d' % s
        rel[name] = np.stack([rng.integers(0, NODES, e), rng.integers(lo, lo + BLOCK, e)]).astype(np.float64)
        blocks[name], types[name] = (lo, BLOCK), (5 * s + 2) % 97
    return Graph(NODES, rel, types), blocks


def host_tables(store, strategy):
    h = store.host
    lo, cnt = (h['seg_lo'], h['seg_n']) if strategy == 'typed' else (np.zeros_like(h['seg_lo']), np.full_like(h['seg_n'], store.num_nodes))
    return store.heads.cpu().numpy(), store.tails.cpu().numpy(), h['seg_ptr'], h['seg_rel'], lo, cnt


def raw_sample(store, strategy, filtered, shuffle, ld_out=4):
    """pea_kg_sample itself, into a table of any row stride with a stale count in *exhausted: (rows, exhausted)"""
    lo, cnt = (store.seg_lo, store.seg_n) if strategy == 'typed' else (store.any_lo, store.any_n)
    keys = store.keys() if filtered else None
    out = torch.full((store.num_triples, ld_out), -1, dtype=torch.int64, device=DEV)
    ex = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    _lib.check(_lib.require_device().pea_kg_sample(
        store.num_triples, _lib.ptr(store.heads), _lib.ptr(store.tails), store.num_segments, _lib.ptr(store.seg_ptr),
        _lib.ptr(store.seg_rel), _lib.ptr(lo), _lib.ptr(cnt), store.num_nodes, _lib.ptr(keys), 0 if keys is None else keys.numel(),
        SEED, EPOCH, shuffle, _lib.ptr(out), ld_out, _lib.ptr(ex), _lib.current_stream()))
    return out.cpu().numpy(), int(ex.item())


MODES = [('random', False), ('typed', False), ('typed', True), ('random', True)]


@pytest.mark.parametrize('n_seg', [1, 3, 64])
@pytest.mark.parametrize('n_triples', [1, 2, 3, 17, 255, 256, 257, 4097])
def test_bit_equal_to_the_restatement(n_triples, n_seg):
    graph, blocks = random_graph(n_triples, n_seg, seed=n_triples + n_seg)
    store = kg_triple_store(graph, DEV, tail_blocks=blocks)
    assert store.num_triples == n_triples and store.num_segments == n_seg
    for strategy, filtered in MODES:
        heads, tails, seg_ptr, seg_rel, lo, cnt = host_tables(store, strategy)
        keys = ref.known_keys(heads, tails, seg_ptr, NODES) if filtered else None
        want, want_ex, _ = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, NODES, keys=keys, seed=SEED, offset=EPOCH)
        want_sh, _, _ = ref.sample(heads, tails, seg_ptr, seg_rel, lo, cnt, NODES, keys=keys, seed=SEED, offset=EPOCH, shuffle=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)          # dense small graphs do exhaust: counted below
            got = device_kg_negative_sampling(store, SEED, epoch=EPOCH, strategy=strategy, filtered=filtered, shuffle=False)
            assert store.negatives_exhausted == want_ex and store.train_data is got and store.train_data_length == n_triples
            got_sh = device_kg_negative_sampling(store, SEED, epoch=EPOCH, strategy=strategy, filtered=filtered)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (n_triples, 4)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(got_sh.cpu().numpy(), want_sh)
        rows, ex = raw_sample(store, strategy, filtered, 1, ld_out=6)           # a wider table: columns 4.. are left alone
        np.testing.assert_array_equal(rows[:, :4], want_sh)
        assert ex == want_ex and (rows[:, 4:] == -1).all()
        view = lambda a: np.sort(np.ascontiguousarray(a).view('i8,i8,i8,i8'), axis=0)
        np.testing.assert_array_equal(view(want_sh), view(want))                 # the same multiset of rows
        if filtered:
            seg = ref.segment_of_rows(seg_ptr)
            known = np.isin((seg * NODES + want[:, 0]) * NODES + want[:, 2], keys)
            assert known.sum() <= want_ex                                          # only exhausted rows keep a known tail


@pytest.mark.parametrize('n', [1, 2, 17, 256, 257, 4097])
def test_permute_rows_width_1_is_perm(n):
    rows = torch.arange(n, dtype=torch.int64, device=DEV).view(n, 1)
    out = device_shuffle_rows(rows, SEED, epoch=EPOCH).cpu().numpy().reshape(-1)
    p = ref.perm(n, SEED, EPOCH)
    np.testing.assert_array_equal(out[p], np.arange(n))                # out[perm(i)] = i
    assert torch.equal(rows.view(-1), torch.arange(n, device=DEV))     # the input is left alone


@pytest.mark.parametrize('width,ld_in,ld_out', [(3, 5, 4), (16, 17, 20), (16, 16, 16)])
def test_permute_rows_moves_whole_rows(width, ld_in, ld_out):
    n = 1000
    g = torch.Generator().manual_seed(width)
    src = torch.randint(0, 1 << 40, (n, ld_in), generator=g, dtype=torch.int64).to(DEV)
    out = torch.full((n, ld_out), -1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.require_device().pea_permute_rows(n, width, _lib.ptr(src), ld_in, _lib.ptr(out), ld_out, SEED, EPOCH,
                                                      _lib.current_stream()))
    p = torch.from_numpy(ref.perm(n, SEED, EPOCH)).to(DEV)
    assert torch.equal(out[p, :width], src[:, :width])
    assert bool((out[:, width:] == -1).all())                          # nothing between the rows is touched
    if ld_in == width:
        assert torch.equal(device_shuffle_rows(src, SEED, epoch=EPOCH), out)


def one_head_store(linked, n_rows):
    """head 0 linked to the first `linked` nodes of the block [1000, 1050), the triples repeated to n_rows"""
    tails = 1000 + np.arange(n_rows) % linked
    graph = Graph(1050, {'r': np.stack([np.zeros(n_rows), tails]).astype(np.float64)}, {'r': 0})
    return kg_triple_store(graph, DEV, tail_blocks={'r': (1000, 50)})


def test_distribution():
    store = one_head_store(10, 100000)
    out = device_kg_negative_sampling(store, 99, strategy='typed', filtered=True).cpu().numpy()
    assert store.negatives_exhausted == 0
    neg = out[:, 2] - 1000
    assert neg.min() >= 10 and neg.max() < 50
    counts = np.bincount(neg, minlength=50)[10:]
    expect = 100000 / 40.0
    assert np.abs(counts - expect).max() < 6 * np.sqrt(expect)        # uniform over the 40 free nodes


def test_exhaustion_warns_and_stays_in_the_block():
    store = one_head_store(50, 100)
    with pytest.warns(RuntimeWarning):
        out = device_kg_negative_sampling(store, 1, strategy='typed', filtered=True)
    assert store.negatives_exhausted == 100                            # every row is flagged
    assert bool(((out[:, 2] >= 1000) & (out[:, 2] < 1050)).all())


def test_refusals_raise():
    store = one_head_store(10, 64)
    lib = _lib.require_device()
    out = torch.empty((64, 4), dtype=torch.int64, device=DEV)
    ex = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = lambda **o: [o.get('n', 64), _lib.ptr(store.heads), _lib.ptr(store.tails), o.get('n_seg', 1), _lib.ptr(store.seg_ptr),
                        _lib.ptr(store.seg_rel), _lib.ptr(store.seg_lo), _lib.ptr(store.seg_n), o.get('num_nodes', 1050), None,
                        o.get('n_keys', 0), 1, 0, o.get('shuffle', 1), _lib.ptr(out), o.get('ld_out', 4), _lib.ptr(ex),
                        _lib.current_stream()]
    for bad in (dict(ld_out=3), dict(n_seg=0), dict(n_seg=1025), dict(num_nodes=0), dict(n_keys=4), dict(shuffle=5)):
        with pytest.raises(_lib.PeaError):
            _lib.check(lib.pea_kg_sample(*args(**bad)))
    with pytest.raises(_lib.PeaError):                                 # in place
        _lib.check(lib.pea_permute_rows(64, 4, _lib.ptr(out), 4, _lib.ptr(out), 4, 1, 0, _lib.current_stream()))
    with pytest.raises(ValueError):
        device_shuffle_rows(torch.zeros((4, 17), dtype=torch.int64, device=DEV), 1)
    with pytest.raises(ValueError):
        device_shuffle_rows(torch.zeros((4, 4), dtype=torch.int32, device=DEV), 1)


def test_identical_calls_give_identical_bytes():
    graph, blocks = random_graph(4097, 3, seed=5)
    store = kg_triple_store(graph, DEV, tail_blocks=blocks)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        a = device_kg_negative_sampling(store, SEED, epoch=1, strategy='typed', filtered=True)
        b = device_kg_negative_sampling(store, SEED, epoch=1, strategy='typed', filtered=True)
        c = device_kg_negative_sampling(store, SEED, epoch=2, strategy='typed', filtered=True)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    assert not torch.equal(a, c) and float((a[:, :2] != c[:, :2]).any(dim=1).float().mean()) > 0.9    # another epoch: another order


# ---------------------------------------------------------------- the table feeds the models
@pytest.fixture(scope='module')
def hin():
    ds = SyntheticHIN('ml_small', scale=0.1)
    ds.num_edge_types = len(ds.edge_index_nps)
    return ds


def check_table(ds, table):
    n_edges = sum(e.shape[1] for e in ds.edge_index_nps.values())
    assert tuple(table.shape) == (n_edges, 4) and table.is_cuda and table.is_contiguous()
    assert ds.train_data is table and ds.train_data_length == n_edges and ds.negatives_exhausted == 0
    assert int(table[:, 3].max()) == len(ds.edge_index_nps) - 1 and int(table[:, :3].max()) < ds.num_nodes


def is_view(batch, table, first_row):
    return batch.data_ptr() == table.data_ptr() + first_row * table.stride(0) * 8 and batch.is_contiguous()


def test_table_feeds_cfkg_without_a_copy(hin):
    torch.manual_seed(4)
    model = CFKGRecsysModel(dataset=hin, emb_dim=16).to(DEV)
    with torch.no_grad():
        model.x.mul_(6.0)
        model.r.mul_(6.0)
    table = device_kg_negative_sampling(hin, SEED, epoch=EPOCH, strategy='typed')
    check_table(hin, table)
    model.train()
    for first in (0, 512):
        batch = table[first:first + 512]
        assert is_view(batch, table, first) and model._native_ok(batch)
        loss = model.kg_loss(batch)
        assert 'Cfkg' in type(loss.grad_fn).__name__
        want = model._kg_loss_torch(batch)
        np.testing.assert_allclose(float(loss.detach()), float(want.detach()), rtol=1e-4)
    loss.backward()
    assert model.x.grad is not None and bool(torch.isfinite(model.x.grad).all())


def test_table_feeds_kgat_native_kg_without_a_copy(hin):
    torch.manual_seed(4)

    class Model(KGATRecsysModel):
        def update_graph_input(self, dataset):
            return kg_graph_input(dataset, DEV)

    model = Model(dataset=hin, emb_dim=16, hidden_size=16, dropout=0.0, native_train=False, native_kg=True).to(DEV)
    device_kg_negative_sampling(hin, SEED, epoch=EPOCH + 1)
    store = hin.kg_store
    table = device_kg_negative_sampling(hin, SEED, epoch=EPOCH)
    assert hin.kg_store is store                                       # built once per dataset
    check_table(hin, table)
    model.train()
    batch = table[256:768]
    assert is_view(batch, table, 256)
    loss = model.kg_loss(batch)
    assert 'Transr' in type(loss.grad_fn).__name__
    model.native_kg = False
    np.testing.assert_allclose(float(loss.detach()), float(model.kg_loss(batch).detach()), rtol=1e-4)


def test_kg_epoch_is_the_hand_written_loop(hin):
    table = device_kg_negative_sampling(hin, SEED, epoch=EPOCH, strategy='typed')
    steps, bs = 21, 256
    table = table[:(steps - 1) * bs + 100]                             # the 21st batch is short and is included

    def fresh():
        torch.manual_seed(4)
        model = CFKGRecsysModel(dataset=hin, emb_dim=16).to(DEV)
        with torch.no_grad():
            model.x.mul_(6.0)
            model.r.mul_(6.0)
        return model.train(), torch.optim.Adam(model.parameters(), lr=1e-2)

    model, opt = fresh()
    losses = []
    for k in range(steps):                                             # the reference driver's loop: one host read per step
        batch = table[k * bs:(k + 1) * bs]
        opt.zero_grad()
        loss = model.kg_loss(batch)
        loss.backward()
        opt.step()
        losses.append(loss.detach().cpu().item())
    want = float(np.mean(losses))
    assert len(losses) == steps and losses[19] < losses[0]            # two full batches: the loop does train
    other, opt2 = fresh()
    got = solvers.kg_epoch(other, opt2, table, bs)
    assert isinstance(got, float) and abs(got - want) <= 1e-6 * abs(want)
    for a, b in zip(model.parameters(), other.parameters()):
        assert torch.equal(a, b)
    third, opt3 = fresh()
    head = solvers.kg_epoch(third, opt3, table, bs, max_steps=5)
    assert abs(head - float(np.mean(losses[:5]))) <= 1e-6 * abs(head)
