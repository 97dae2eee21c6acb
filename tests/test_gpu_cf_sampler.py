"""GPU: the on-device CF epoch sampler (csrc/cf_sampler.hip, include/peahip_cf_sample.h) against the numpy restatement of its
streams (tests/cf_sampler_ref.py) bit for bit, against the two launches it composes (pea_sample_negatives, pea_permute_rows),
and the table feeding an entity-aware PEAGAT through solvers.cf_epoch.  Integers only: every comparison is equality."""
import warnings

import numpy as np
import pytest
import torch

import cf_sampler_ref as ref
from graph_recsys_benchmark_amd import _lib, models, pea_solver_bpr, solvers
from graph_recsys_benchmark_amd.utils import (SyntheticHIN, device_cf_negative_sampling, device_negative_sampling, device_shuffle_rows,
                                              entity_store, update_pea_graph_input)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEED, EPOCH = (7 << 32) | 2020, 3          # a seed with a non-zero high word
FORMS = [('BPR', False), ('BPR', True), ('BCE', False)]          # (loss, entity columns)


def device_table(ds, shuffle, epoch=EPOCH):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)               # dense small datasets do exhaust: counted by the caller
        return device_cf_negative_sampling(ds, SEED, epoch=epoch, device=DEV, shuffle=shuffle)


# rows = n_pos k (BPR) or n_pos (1 + k) (BCE): 1 and 2 (hb = 1), the workgroup edge 255 / 256 / 257 in either form, and k = 4
SHAPES = [(1, 1), (2, 1), (255, 1), (256, 1), (257, 1), (1, 4), (64, 4), (65, 4), (51, 4), (128, 1)]


@pytest.mark.parametrize('strategy', ['random', 'unseen'])
@pytest.mark.parametrize('n_pos,k', SHAPES)
def test_bit_equal_to_the_restatement(n_pos, k, strategy):
    for loss, ent in FORMS:
        ds = ref.SmallDataset(n_pos, k=k, loss=loss, strategy=strategy, entity_aware=ent, seed=n_pos + k)
        n_rows = n_pos * (k + 1 if loss == 'BCE' else k)
        want, want_ex, bad, _ = ref.sample_dataset(ds, SEED, offset=EPOCH)
        want_sh, _, _, _ = ref.sample_dataset(ds, SEED, offset=EPOCH, shuffle=True)
        assert bad == 0 and want.shape == (n_rows, 9 if ent else 3)
        got = device_table(ds, False)
        assert ds.negatives_exhausted == want_ex and ds.train_data is got and ds.train_data_length == n_rows
        assert got.dtype == torch.int64 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == want.shape
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg='%s %s' % (loss, ent))
        got_sh = device_table(ds, True)
        np.testing.assert_array_equal(got_sh.cpu().numpy(), want_sh, err_msg='%s %s shuffled' % (loss, ent))
        # the shuffle is the row shuffle of pea_permute_rows, the negatives those of pea_sample_negatives
        assert torch.equal(got_sh, device_shuffle_rows(got, SEED, epoch=EPOCH))
        if loss == 'BPR':
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                plain = device_negative_sampling(ds, SEED, epoch=EPOCH, device=DEV, shuffle=False)
            assert torch.equal(got[:, :3], plain) and ds.negatives_exhausted == want_ex


def raw_sample(ds, shuffle, ld_out):
    """pea_cf_sample itself into a table of any row stride, with stale counts in the two counters: (rows, exhausted, bad rows)"""
    pos = torch.as_tensor(ds.edge_index_nps['user2item']).to(device=DEV, dtype=torch.int64)
    pos_u, pos_i = pos[0].contiguous(), pos[1].contiguous()
    k = ds.num_negative_samples
    store = entity_store(ds, DEV) if ds.entity_aware else None
    mode = _lib.CF_BCE if ds.cf_loss_type == 'BCE' else _lib.CF_BPR
    keys = torch.unique(pos_u * 20 + (pos_i - 15)) if ds.sampling_strategy == 'unseen' else None
    out = torch.full((pos_u.numel() * (k + 1 if mode else k), ld_out), -1, dtype=torch.int64, device=DEV)
    counts = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    tables = [None, None, 0, None, None, 0, 0, None, None] if store is None else [
        _lib.ptr(store.item_ptr), _lib.ptr(store.item_ent), store.nnz_i, _lib.ptr(store.user_ptr), _lib.ptr(store.user_ent),
        store.nnz_u, store.num_blocks, _lib.ptr(store.block_lo), _lib.ptr(store.block_n)]
    _lib.check(_lib.require_device().pea_cf_sample(
        pos_u.numel(), k, mode, _lib.ptr(pos_u), _lib.ptr(pos_i), 15, 20, 0, 15, _lib.ptr(keys), 0 if keys is None else keys.numel(),
        *tables, SEED, EPOCH, shuffle, _lib.ptr(out), ld_out, _lib.ptr(counts), _lib.ptr(counts[1:]), _lib.current_stream()))
    return out.cpu().numpy(), int(counts[0]), int(counts[1])


@pytest.mark.parametrize('loss,ent,ld_out', [('BPR', False, 5), ('BPR', True, 11), ('BCE', False, 4)])
def test_a_wider_table_keeps_its_spare_words(loss, ent, ld_out):
    ds = ref.SmallDataset(257, k=4, loss=loss, strategy='unseen', entity_aware=ent, seed=9)
    width = 9 if ent else 3
    for shuffle in (0, 1):
        want, want_ex, _, _ = ref.sample_dataset(ds, SEED, offset=EPOCH, shuffle=bool(shuffle))
        rows, ex, bad = raw_sample(ds, shuffle, ld_out)
        np.testing.assert_array_equal(rows[:, :width], want)
        assert (rows[:, width:] == -1).all() and ex == want_ex and bad == 0      # the counters were cleared first


def test_a_cycle_walk_across_the_square():
    """65,537 rows: hb = 9, the network permutes [0, 2^18) and is walked until it lands below 65,537"""
    ds = ref.SmallDataset(65537, k=1, entity_aware=True, seed=11)
    want, want_ex, _, _ = ref.sample_dataset(ds, SEED, offset=EPOCH, shuffle=True)
    got = device_table(ds, True)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert want_ex == 0 and ds.negatives_exhausted == 0
    ones = got[got[:, 5] == 1]
    assert len(torch.unique(ones[:, 3])) == 15 and len(torch.unique(ones[:, 4])) == 15     # every entity is drawn, either way


def test_epochs_differ_and_repeat():
    ds = ref.SmallDataset(257, k=4, strategy='unseen', entity_aware=True, seed=12)
    a, b, c = device_table(ds, True, epoch=1), device_table(ds, True, epoch=1), device_table(ds, True, epoch=2)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    assert not torch.equal(a, c) and float((a != c).any(dim=1).float().mean()) > 0.9
    a0, c0 = device_table(ds, False, epoch=1), device_table(ds, False, epoch=2)
    assert torch.equal(a0[:, :2], c0[:, :2]) and float((a0[:, 2] != c0[:, 2]).float().mean()) > 0.8
    assert float((a0[:, 3:] != c0[:, 3:]).any(dim=1).float().mean()) > 0.5


def test_exhaustion_warns():
    ds = ref.SmallDataset(100, k=4, strategy='unseen', seed=3, full_user=True)
    with pytest.warns(RuntimeWarning):
        out = device_cf_negative_sampling(ds, SEED, device=DEV, shuffle=False)
    assert ds.negatives_exhausted == 80
    assert bool(((out[:, 2] >= 15) & (out[:, 2] < 35)).all())


@pytest.mark.parametrize('loss,ent', FORMS)
def test_an_id_outside_its_block_is_a_bad_row(loss, ent):
    ds = ref.SmallDataset(300, k=2, loss=loss, entity_aware=ent, seed=4)
    ds.edge_index_nps['user2item'][1, 7] = 35                          # one past the item block
    want, _, bad, _ = ref.sample_dataset(ds, SEED, offset=EPOCH)
    rows, ex, got_bad = raw_sample(ds, 0, 9 if ent else 3)
    assert got_bad == bad == (1 if loss == 'BCE' else 2) and ex == 0
    np.testing.assert_array_equal(rows, want)                          # item_lo as the negative, zeros as the entity columns
    with pytest.raises(ValueError, match='outside its block'):
        device_cf_negative_sampling(ds, SEED, epoch=EPOCH, device=DEV)
    ds.edge_index_nps['user2item'][1, 7] = 34
    ds.edge_index_nps['user2item'][0, 299] = -1                        # and a user below its block
    assert raw_sample(ds, 1, 9 if ent else 3)[2] == (3 if loss == 'BCE' else 2)


# ---------------------------------------------------------------- the table feeds the entity-aware model
@pytest.fixture(scope='module')
def hin():
    ds = SyntheticHIN('ml_small', scale=0.05)
    ds.entity_lists()
    ds.cf_loss_type, ds.sampling_strategy, ds.entity_aware, ds.num_negative_samples = 'BPR', 'random', True, 4
    return ds


def fresh_model(ds):
    dataset_args = ds.dataset_args()
    train_args = {'device': torch.device('cuda', 0), 'num_metapaths': ds.spec['num_metapaths']}

    class Model(models.PEAGATRecsysModel):
        def update_graph_input(self, dataset):
            return update_pea_graph_input(dataset_args, train_args, ds)

    torch.manual_seed(2020)
    model = Model(**ds.model_args(kind='gat', entity_aware=True)).to(DEV)
    return model.train(), torch.optim.Adam(model.parameters(), lr=1e-3)


@pytest.fixture
def deterministic_index_add():
    """The backward of the entity regulariser adds its gradient rows into dx with torch's index_add_ (scoring._EntityReg), whose
    float atomics land in no fixed order when an entity id repeats in a batch; torch's deterministic mode gives it the sorted
    accumulation.  Both loops below run under it, so that a bitwise comparison of them means something."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def test_cf_epoch_is_the_hand_written_loop_on_entity_aware_rows(hin, deterministic_index_add):
    table = device_cf_negative_sampling(hin, SEED, epoch=EPOCH, device=DEV)
    n = hin.edge_index_nps['user2item'].shape[1] * 4
    assert tuple(table.shape) == (n, 9) and hin.train_data is table and hin.negatives_exhausted == 0
    assert int(table[:, :5].max()) < hin.num_nodes and int(table[:, 5].min()) == 1            # every item has its year
    steps, bs = 3, 512
    model, opt = fresh_model(hin)
    losses = []
    for k in range(steps):
        batch = table[k * bs:(k + 1) * bs]
        assert batch.data_ptr() == table.data_ptr() + k * bs * 72 and batch.is_contiguous()   # a view: no copy
        opt.zero_grad()
        loss = model.loss(batch)
        loss.backward()
        opt.step()
        losses.append(loss.detach().cpu().item())
    print('losses of the hand-written loop:', losses)
    assert all(np.isfinite(losses))
    other, opt2 = fresh_model(hin)
    got = solvers.cf_epoch(other, opt2, table, bs, max_steps=steps)
    # the mean of the hand-collected losses, reduced as cf_epoch reduces its device tensor (float64 mean of the float32 values)
    want = float(torch.tensor(losses, dtype=torch.float32, device=DEV).double().mean().item())
    print('cf_epoch mean %r, hand-written mean %r' % (got, want))
    assert isinstance(got, float) and got == want and abs(got - float(np.mean(losses))) <= 1e-12 * abs(got)
    for (name, a), b in zip(model.named_parameters(), other.parameters()):
        assert torch.equal(a, b), name
    masked = table[:bs].clone()
    masked[:, 3:] = 0                                                  # both masks off: each term is log sigmoid(0)
    with torch.no_grad():
        assert float(other.loss(table[:bs])) != float(other.loss(masked))                   # the entity columns do take part


def test_the_solver_trains_entity_aware_where_it_refused():
    ds = SyntheticHIN('ml_small', seed=2019, scale=0.05)
    res = pea_solver_bpr.main(['--model', 'PEAGAT', '--entity_aware', 'true', '--train_step', 'true', '--metapath_test', 'false',
                               '--eval_users', '16'], dataset=ds)
    assert np.isfinite(res['train_loss']) and res['train_loss'] > 0
    assert tuple(ds.train_data.shape) == (ds.edge_index_nps['user2item'].shape[1] * 4, 9) and hasattr(ds, 'entity_store')
    assert pea_solver_bpr.main.last_model.entity_aware
