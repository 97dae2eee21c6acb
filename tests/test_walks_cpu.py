"""CPU: the restated metapath2vec walks (tests/walk_ref.py) have the properties the device walks are compared against, the
window slicing is the reference's, and the new models / entry points exist with the reference's surface."""
import numpy as np
import pytest
import torch

import walk_ref


def _toy_csrs(hin):
    return [walk_ref.csr_of(hin['edge_index_dict'][keys], hin['num_nodes']) for keys in hin['metapath']]


def _toy_walks(walk_length=10, seed=walk_ref.WALK_SEED, offset=0):
    hin = walk_ref.toy_hin()
    starts = np.tile(np.arange(hin['num_nodes_dict']['uid']), 7)[:273]
    csrs = _toy_csrs(hin)
    walks, status = walk_ref.metapath_walks(csrs, [0, 1, 2, 3], starts, walk_length, seed, offset, hin['num_nodes'])
    return hin, csrs, starts, walks, status


def test_toy_hin_has_the_edge_cases():
    hin = walk_ref.toy_hin()
    eid, acc, cnt = hin['edge_index_dict'], hin['type_accs'], hin['num_nodes_dict']
    u2i, g2i = eid[('uid', 'has watched', 'iid')], eid[('genre', 'as the genre of', 'iid')]
    assert np.unique(u2i, axis=1).shape[1] < u2i.shape[1] and np.unique(g2i, axis=1).shape[1] < g2i.shape[1]   # doubled edges
    assert acc['iid'] + cnt['iid'] - 1 not in g2i[1] and acc['uid'] + cnt['uid'] - 1 not in u2i[0]
    per_genre = np.bincount(g2i[0] - acc['genre'], minlength=cnt['genre'])
    assert per_genre[0] >= 2 * per_genre[1:].max()                                                            # one hub genre


def test_restated_walks_follow_edges_and_stop_at_edgeless_nodes():
    hin, csrs, starts, walks, status = _toy_walks()
    assert (walks[:, 0] == starts).all()
    dead = 0
    for row in walks:
        for t in range(1, walks.shape[1]):
            rowptr, col = csrs[(t - 1) % 4]
            cur = row[t - 1]
            if cur < 0:
                assert row[t] == -1
                continue
            nbrs = col[rowptr[cur]:rowptr[cur + 1]]
            if nbrs.size == 0:
                assert row[t] == -1
                dead += 1
            else:
                assert row[t] in nbrs
    assert status == [dead, 0]


def test_toy_walks_complete_and_dead_end_often_enough():
    """the seed the GPU comparison uses: neither kind of walk may be rare, or that comparison checks nothing"""
    for length in (10, 3):
        _, _, _, walks, status = _toy_walks(length)
        complete = (walks[:, -1] >= 0).mean()
        assert complete >= 0.5, complete
        assert status[0] >= 0.05 * walks.shape[0], status
        assert status[0] == int((walks[:, -1] < 0).sum())


def test_restated_walks_depend_on_seed_and_offset_and_flag_bad_starts():
    _, csrs, starts, walks, _ = _toy_walks()
    hin = walk_ref.toy_hin()
    other_seed = walk_ref.metapath_walks(csrs, [0, 1, 2, 3], starts, 10, walk_ref.WALK_SEED + 1, 0, hin['num_nodes'])[0]
    other_off = walk_ref.metapath_walks(csrs, [0, 1, 2, 3], starts, 10, walk_ref.WALK_SEED, 1, hin['num_nodes'])[0]
    assert (walks != other_seed).any() and (walks != other_off).any()
    bad = starts.copy()
    bad[5] = hin['num_nodes']
    w2, status = walk_ref.metapath_walks(csrs, [0, 1, 2, 3], bad, 10, walk_ref.WALK_SEED, 0, hin['num_nodes'])
    assert status[1] == 1 and (w2[5] == -1).all()
    np.testing.assert_array_equal(np.delete(w2, 5, axis=0), np.delete(walks, 5, axis=0))       # rows are independent


def test_uniform_walks_stay_inside_their_blocks():
    lo, n = [40, 70, 40, 0], [30, 5, 30, 40]
    walks = walk_ref.uniform_walks(lo, n, np.arange(100) % 40, 10, 3, 1)
    for t in range(1, 11):
        s = (t - 1) % 4
        assert ((walks[:, t] >= lo[s]) & (walks[:, t] < lo[s] + n[s])).all()
    assert len(np.unique(walks[:, 1])) > 15


def _model(**kw):
    from graph_recsys_benchmark_amd.models import MetaPath2Vec
    hin = walk_ref.toy_hin()
    args = dict(edge_index_dict={k: torch.from_numpy(v) for k, v in hin['edge_index_dict'].items()}, embedding_dim=8,
                metapath=hin['metapath'], walk_length=6, context_size=3, num_nodes_dict=hin['num_nodes_dict'],
                types=hin['types'], type_accs=hin['type_accs'])
    args.update(kw)
    return MetaPath2Vec(**args), hin


def test_windows_is_the_references_slicing():
    model, _ = _model(walk_length=4, context_size=3)
    rw = torch.tensor([[0, 1, 2, 3, 4], [10, 11, 12, 13, -1]])
    want = torch.tensor([[0, 1, 2], [10, 11, 12], [1, 2, 3], [11, 12, 13], [2, 3, 4], [12, 13, -1]])
    assert torch.equal(model.windows(rw), want)
    np.testing.assert_array_equal(walk_ref.windows(rw.numpy(), 3), want.numpy())


def test_models_and_entry_points_exist_with_the_reference_surface():
    from graph_recsys_benchmark_amd import _lib, engine
    from graph_recsys_benchmark_amd.models import WalkBasedRecsysModel
    model, hin = _model(sparse=True)
    assert list(model.state_dict()) == ['embedding.weight']
    assert tuple(model.embedding.weight.shape) == (hin['num_nodes'], 8) and model.embedding.sparse
    assert repr(model) == 'MetaPath2Vec(%d, 8)' % hin['num_nodes']
    assert model('iid').shape == (30, 8) and model('genre', torch.tensor([1, 2])).shape == (2, 8)
    assert model.start == {'uid': 0, 'iid': 40, 'genre': 70} and model.end['genre'] == 75
    for name in ('loader', 'sample', 'pos_sample', 'neg_sample', 'loss', 'windows'):
        assert callable(getattr(model, name))
    rec = WalkBasedRecsysModel(embedding=model.embedding.weight, embedding_dim=8)
    assert sorted(rec.state_dict()) == ['fc1.bias', 'fc1.weight', 'fc2.bias', 'fc2.weight']
    assert not isinstance(rec.cached_repr, torch.nn.Parameter) and not rec.cached_repr.requires_grad
    assert rec.eval() is rec and not rec.training
    assert rec.predict(torch.tensor([0, 1]), torch.tensor([40, 41])).shape == (2, 1)
    for sym in ('pea_metapath_walks', 'pea_uniform_walks', 'pea_skipgram_supported', 'pea_skipgram_workspace_bytes',
                'pea_skipgram_train'):
        assert sym in _lib.SIGNATURES
    for fn in ('metapath_walks', 'uniform_walks', 'skipgram_supported', 'skipgram_loss'):
        assert callable(getattr(engine, fn))
    assert engine.skipgram_supported(64, 101, 7) and engine.skipgram_supported(128, 128, 16) and engine.skipgram_supported(4, 2, 2)
    assert not engine.skipgram_supported(6, 7, 7) and not engine.skipgram_supported(64, 6, 7)
    assert not engine.skipgram_supported(64, 20, 17) and not engine.skipgram_supported(64, 129, 7)


def test_torch_loss_agrees_with_the_restatement_and_skips_dead_ends():
    """the native=False composition (the timing yardstick) on whole walks against the restatement on the reference's windows"""
    model, hin = _model(native=False)
    rng = np.random.default_rng(0)
    pos = rng.integers(0, hin['num_nodes'], size=(6, 7))
    pos[2, 4:] = -1
    pos[4, :] = -1
    neg = rng.integers(0, hin['num_nodes'], size=(9, 7))
    loss = model.loss(torch.from_numpy(pos), torch.from_numpy(neg))
    loss.backward()
    want, grad, counts = walk_ref.skipgram_loss(model.embedding.weight.detach().numpy(), walk_ref.windows(pos, 3),
                                                walk_ref.windows(neg, 3), torch.float64)
    assert counts == [4 * 5 * 2 + 5, 9 * 5 * 2]       # four whole rows; row 2 keeps (0,1) (0,2) (1,2) (1,3) (2,3); row 4 nothing
    np.testing.assert_allclose(loss.item(), want[0], rtol=1e-5)
    np.testing.assert_allclose(model.embedding.weight.grad.numpy(), grad, rtol=1e-4, atol=1e-7)
    same = model.loss(model.windows(torch.from_numpy(pos)), model.windows(torch.from_numpy(neg)))
    np.testing.assert_allclose(same.item(), want[0], rtol=1e-5)


def test_constructor_assertions():
    hin = walk_ref.toy_hin()
    with pytest.raises(AssertionError):
        _model(metapath=hin['metapath'][:3])                       # not closed: uid ... genre -> iid
    with pytest.raises(AssertionError):
        _model(walk_length=2, context_size=3)
    with pytest.raises(AssertionError):
        _model(type_accs={'uid': 0, 'iid': 41, 'genre': 70})       # embedding row = global id does not hold
