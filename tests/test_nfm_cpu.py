"""CPU: NFM without a device -- NFMRecsysModel against the reference-recorded fixture tests/golden/nfm_small.npz
(tests/make_nfm_golden.py), the torch fold against the BN-eval composition, the ranking hooks against a brute-force
restatement, the fifth header against _lib.FM_SIGNATURES, every argument error (returned before anything is launched), the
supported shapes, the BCE sampling branch against a numpy recomputation, and the float32 headroom of every GPU training case
(tests/nfm_ref.py: TRAIN_CASES)."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import nfm_ref
from graph_recsys_benchmark_amd import _lib, engine
from graph_recsys_benchmark_amd.models import MFRecsysModel, NFMRecsysModel
from graph_recsys_benchmark_amd.utils import cf_negative_sampling
from helpers import EPS32, assert_fp32_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NOMEM = -1, -4
N_USER, N_ITEM, E, H = 60, 90, 20, 24


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'nfm_small.npz'))


def model_of(z, prefix='sd.', **kw):
    model = NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=E, hidden_size=H, dropout=0, **kw)
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)})
    return model


def batch_of(z):
    return torch.from_numpy(np.stack([z['uid'], z['iid'], z['label']], axis=1))


# ---------------------------------------------------------------- the model against the fixture
def test_state_dict_keys_are_the_reference_layout(golden):
    model = NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=E, hidden_size=H, dropout=0.3)
    want = [k[3:] for k in golden.files if k.startswith('sd.')]
    assert sorted(model.state_dict().keys()) == sorted(want)
    assert sorted(want) == sorted(list(nfm_ref.STATE_KEYS.values()) + ['emb.fm.1.num_batches_tracked', 'emb.mlp.mlp.1.num_batches_tracked'])
    assert isinstance(model, MFRecsysModel) and model.emb.fm[2].p == 0.3 and model.emb.mlp.mlp[3].p == 0.3
    assert tuple(model.emb.mlp.mlp[0].weight.shape) == (H, E)
    with pytest.raises(NotImplementedError):
        model.shard(0, 2)


def test_training_step_reproduces_the_fixture(golden):
    model = model_of(golden).train()
    batch = batch_of(golden)
    loss = model.loss(batch)
    loss.backward()
    np.testing.assert_allclose(loss.detach().numpy(), golden['loss'], rtol=1e-6, atol=0)
    with torch.no_grad():
        pred = model_of(golden).train().predict(batch[:, 0], batch[:, 1])
    np.testing.assert_allclose(pred.numpy(), golden['pred'], rtol=1e-6, atol=1e-7)
    for name, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), golden['grad.' + name], rtol=1e-5, atol=1e-8, err_msg=name)
    for name, t in model.state_dict().items():
        np.testing.assert_allclose(t.numpy(), golden['sd1.' + name], rtol=1e-6, atol=1e-7, err_msg=name)
    assert int(model.state_dict()['emb.fm.1.num_batches_tracked']) == int(golden['sd1.emb.fm.1.num_batches_tracked'].reshape(-1)[0]) == 1


def test_eval_mode_reproduces_the_fixture(golden):
    model = model_of(golden, prefix='sd1.').eval()
    batch = batch_of(golden)
    with torch.no_grad():
        np.testing.assert_allclose(model.predict(batch[:, 0], batch[:, 1]).numpy(), golden['eval_pred'], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(model.loss(torch.from_numpy(golden['eval_block'])).numpy(), golden['eval_loss'], rtol=1e-6)
        # the fold scores what the BN-eval composition scores
        y = model._logits_torch(batch[:, 0], batch[:, 1])
        np.testing.assert_allclose(torch.sigmoid(y).numpy(), golden['eval_pred'], rtol=2e-6, atol=2e-7)


def test_mf_base_is_bce_with_logits():
    class Dot(MFRecsysModel):
        def _init(self, **kw):
            self.u, self.i = torch.nn.Embedding(5, 4), torch.nn.Embedding(7, 4)

        def reset_parameters(self):
            pass

        def forward(self, uid, iid):
            return (self.u(uid) * self.i(iid)).sum(dim=-1)

    m = Dot().train()
    batch = torch.tensor([[0, 1, 1], [2, 3, 0], [4, 6, 1]])
    want = torch.nn.functional.binary_cross_entropy_with_logits(m(batch[:, 0], batch[:, 1]), batch[:, 2].float())
    assert torch.equal(m.loss(batch), want)
    m.eval()
    block = torch.tensor([[1, 2, 3], [1, 2, 4], [1, 2, 5]])
    logits = torch.cat([m(block[:1, 0], block[:1, 1]), m(block[:, 0], block[:, 2])])
    want = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.tensor([1., 0., 0., 0.]))
    assert torch.equal(m.loss(block), want)


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize('e,h', [(4, 4), (20, 24), (36, 100)])
def test_torch_fold_is_the_bn_eval_composition(e, h):
    inp = nfm_ref.make_inputs(e, h, 50, seed=31, U=40, I=70)
    fold = engine.nfm_fold_torch(*nfm_ref.engine_args(inp), 40)
    want = nfm_ref.eval_logits(inp, torch.float64, inp['uid'], inp['iid'])
    x = fold.emb[inp['uid']] * fold.emb[40 + inp['iid']]
    got = ((fold.lin[inp['uid']] + fold.lin[40 + inp['iid']]) + fold.bias) + torch.relu(x @ fold.w.t() + fold.b) @ fold.w2
    assert float((got - want).abs().max()) < 1e-13
    assert tuple(fold.w.shape) == (h, e) and fold.num_users == 40 and fold.num_items == 70


# ---------------------------------------------------------------- the ranking hooks on the CPU
ACC_U, ACC_I = 3, 3 + N_USER


@pytest.fixture(scope='module')
def cpu_model(golden):
    model = model_of(golden, prefix='sd1.', acc_uids=ACC_U, acc_iids=ACC_I)
    with torch.no_grad():
        model.emb.embedding.embedding.weight[N_USER + 11] = model.emb.embedding.embedding.weight[N_USER + 10]      # two items that tie
        model.emb.linear.fc.weight[N_USER + 11] = model.emb.linear.fc.weight[N_USER + 10]
    return model.double().eval()


def brute_logit(model, u_nid, i_nid):
    sd = {k: v.double() for k, v in model.state_dict().items()}
    inp = {k: sd[key] for k, key in nfm_ref.STATE_KEYS.items()}
    inp['U'] = N_USER
    return float(nfm_ref.eval_logits(inp, torch.float64, torch.tensor([u_nid - ACC_U]), torch.tensor([i_nid - ACC_I]))[0])


def test_hooks_need_eval_mode(golden):
    model = model_of(golden)
    for call in (lambda: model.rank_eval(torch.tensor([3]), torch.tensor([[70, 71]])),
                 lambda: model.rank_full(torch.tensor([3]), torch.tensor([70]), (ACC_I, ACC_I + N_ITEM)),
                 lambda: model.recommend(torch.tensor([3]), 5, (ACC_I, ACC_I + N_ITEM))):
        with pytest.raises(RuntimeError):
            call()
    assert model.eval().cached_repr is model.folded.w and model.train().folded is None


def test_rank_eval_matches_brute_force(cpu_model):
    g = torch.Generator().manual_seed(3)
    unids = torch.randint(ACC_U, ACC_U + N_USER, (9,), generator=g)
    cand = torch.randint(ACC_I, ACC_I + N_ITEM, (9, 14), generator=g)
    cand[0, 0], cand[0, 1] = ACC_I + 10, ACC_I + 11                      # a tie with the positive counts on neither side
    pred, rank, auc, loss = cpu_model.rank_eval(unids, cand)
    y = np.array([[brute_logit(cpu_model, int(u), int(i)) for i in row] for u, row in zip(unids, cand)])
    np.testing.assert_allclose(pred.numpy(), 1 / (1 + np.exp(-y)), rtol=1e-12)
    got_y = torch.logit(pred).numpy()
    assert rank.dtype == torch.int32
    assert rank.tolist() == [(got_y[r, 1:] > got_y[r, 0]).sum() for r in range(9)]
    np.testing.assert_allclose(auc.numpy(), [(got_y[r, 1:] < got_y[r, 0]).sum() / 13 for r in range(9)], rtol=1e-6)
    assert (got_y[0, 1] == got_y[0, 0]) and rank[0] == (y[0, 2:] > y[0, 0]).sum()
    label = np.zeros_like(y)
    label[:, 0] = 1
    np.testing.assert_allclose(loss.numpy(), ((1 / (1 + np.exp(-y)) - label) ** 2).mean(axis=1), rtol=1e-12)


def test_rank_full_and_recommend_match_brute_force(cpu_model):
    unids = torch.tensor([ACC_U + 5, ACC_U + 0, ACC_U + 59, ACC_U + 5])
    pos = torch.tensor([ACC_I + 10, ACC_I + 3, ACC_I + 89, ACC_I + 40])
    lo, hi = ACC_I + 2, ACC_I + 80
    rowptr = torch.tensor([0, 3, 3, 5, 6])
    excl = torch.tensor([ACC_I + 4, ACC_I + 11, ACC_I + 85, ACC_I + 2, ACC_I + 79, ACC_I + 40])
    cpu_model.USER_CHUNK = 3                                               # two chunks: the exclusion rows follow their users
    rank, auc, pos_score = cpu_model.rank_full(unids, pos, (lo, hi), exclude=(rowptr, excl))
    items, scores = cpu_model.recommend(unids, 80, (lo, hi), exclude=(rowptr, excl))
    top5, _ = cpu_model.recommend(unids, 5, (lo, hi), exclude=(rowptr, excl))
    for q in range(4):
        gone = set(excl[rowptr[q]:rowptr[q + 1]].tolist())
        y = {i: brute_logit(cpu_model, int(unids[q]), i) for i in range(lo, hi)}
        yp = brute_logit(cpu_model, int(unids[q]), int(pos[q]))
        elig = [i for i in y if i not in gone and i != int(pos[q])]
        assert int(rank[q]) == sum(y[i] > yp for i in elig) and abs(float(pos_score[q]) - yp) < 1e-12
        assert abs(float(auc[q]) - sum(y[i] < yp for i in elig) / len(elig)) < 1e-6
        keep = sorted((i for i in y if i not in gone), key=lambda i: (-y[i], i))
        assert items[q, :len(keep)].tolist() == keep                       # score descending, id ascending
        assert (items[q, len(keep):] == -1).all() and torch.isinf(scores[q, len(keep):]).all() and items.shape == (4, 80)
        assert top5[q].tolist() == keep[:5]
    order = items[0].tolist()
    assert ACC_I + 11 not in order and ACC_I + 10 in order                 # of the tying pair, user 0 excludes one
    order = items[1, :78].tolist()
    assert order.index(ACC_I + 10) + 1 == order.index(ACC_I + 11)          # user 1 keeps both: the smaller id first


# ---------------------------------------------------------------- the fifth header
C_WIDTH = {'void': 'void', 'int': 'int', 'int64_t': 'int64', 'size_t': 'uint64', 'uint64_t': 'uint64', 'uint32_t': 'uint32',
           'float': 'float', 'double': 'double'}


def c_width(decl, is_param):
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = [w for w in decl.split() if w not in ('const', 'struct')]
    if is_param and len(words) > 1:
        words = words[:-1]                      # the parameter's name
    return C_WIDTH.get(' '.join(words), 'unknown C type: %s' % decl.strip())


def ctypes_width(t):
    if t is None:
        return 'void'
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return 'pointer'
    table = {C.c_int: 'int', C.c_int64: 'int64', C.c_size_t: 'uint64', C.c_uint64: 'uint64', C.c_uint32: 'uint32',
             C.c_float: 'float', C.c_double: 'double'}
    return table.get(t, 'unknown ctypes type: %r' % t)


def prototypes(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    protos = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w \*]*?)\b(pea_[a-z_0-9]+)\s*\(([^)]*)\)\s*;', text):
        params = [p for p in params.split(',') if p.strip() and p.strip() != 'void']
        assert name not in protos, 'declared twice: %s' % name
        protos[name] = (c_width(ret, False), [c_width(p, True) for p in params])
    return protos


def test_fifth_header_matches_its_ctypes_table():
    protos = prototypes('peahip_fm.h')
    assert sorted(protos) == sorted(_lib.FM_SIGNATURES) == ['pea_nfm_fold', 'pea_nfm_score', 'pea_nfm_supported', 'pea_nfm_train',
                                                            'pea_nfm_train_workspace_bytes']
    lib = _lib.load()
    for name, (ret, params) in sorted(protos.items()):
        restype, argtypes = _lib.FM_SIGNATURES[name]
        assert (ctypes_width(restype), [ctypes_width(t) for t in argtypes]) == (ret, params), name
        assert hasattr(lib, name), 'libpeahip.so lacks %s' % name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), '%s is not typed by load()' % name
    others = set()
    for header in ('peahip.h', 'peahip_kge.h', 'peahip_eval.h', 'peahip_sample.h'):
        others |= set(prototypes(header))
    assert not others & set(protos)
    assert not (set(_lib.SIGNATURES) | set(_lib.KGE_SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.SAMPLE_SIGNATURES)) & set(_lib.FM_SIGNATURES)
    text = open(os.path.join(ROOT, 'include', 'peahip_fm.h')).read()
    for name, value in (('PAIRS', _lib.NFM_PAIRS), ('ROWS', _lib.NFM_ROWS), ('RANGE', _lib.NFM_RANGE), ('MAX_BATCH', _lib.NFM_MAX_BATCH)):
        assert re.search(r'#define\s+PEA_NFM_%s\s+%d\b' % (name, value), text)
    assert 2 * _lib.NFM_MAX_BATCH == engine.ROWS_SCATTER_MAX


# ---------------------------------------------------------------- supported shapes, workspace, argument errors
WIDTHS = {0: 0, 4: 1, 6: 0, 20: 1, 36: 1, 100: 1, 128: 1, 132: 0, -4: 0}


def test_supported_table():
    lib = _lib.load()
    for e, e_ok in WIDTHS.items():
        for h, h_ok in WIDTHS.items():
            assert lib.pea_nfm_supported(e, h) == (e_ok and h_ok), (e, h)
            for b in (1, 2, 1000, 8192, 8193):
                assert (lib.pea_nfm_train_workspace_bytes(b, e, h) > 0) == bool(e_ok and h_ok and 2 <= b <= 8192), (b, e, h)
    assert engine.nfm_supported(64, 64, 8192) and not engine.nfm_supported(64, 64, 8193) and not engine.nfm_supported(64, 64, 1)
    assert engine.nfm_supported(64, 64) and not engine.nfm_supported(64, 66)
    sizes = [lib.pea_nfm_train_workspace_bytes(b, 64, 64) for b in (2, 16, 17, 1000, 4096, 8192)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


_keep = []


def fake(nbytes=4096, misalign=0):
    """A 16-byte aligned host address (+ misalign) that stands in for a device pointer: the calls below fail validation before
    they would read through it."""
    buf = C.create_string_buffer(nbytes + 32)
    _keep.append(buf)
    return C.c_void_p(((C.addressof(buf) + 15) & ~15) + misalign)


TRAIN_ORDER = ('B', 'E', 'H', 'U', 'I', 'emb', 'ld_emb', 'lin', 'bias0', 'bn1_w', 'bn1_b', 'bn1_mean', 'bn1_var', 'w1', 'b1', 'bn2_w',
               'bn2_b', 'bn2_mean', 'bn2_var', 'w2', 'b2', 'eps', 'momentum', 'update', 'uids', 'iids', 'labels', 'keep1', 'keep2',
               'scale', 'loss', 'pred', 'stats', 'dense', 'rows', 'pos', 'ws', 'ws_bytes', 'stream')


def train_call(**over):
    a = {k: fake() for k in TRAIN_ORDER}
    a.update(B=100, E=16, H=8, U=50, I=60, ld_emb=16, eps=1e-5, momentum=0.1, update=1, scale=1.25, ws_bytes=1 << 40, stream=None)
    a.update(over)
    return _lib.load().pea_nfm_train(*[a[k] for k in TRAIN_ORDER])


TRAIN_BAD = [dict(B=1), dict(B=0), dict(B=8193), dict(E=6), dict(E=132), dict(H=0), dict(H=130), dict(U=0), dict(I=0), dict(emb=None),
             dict(lin=None), dict(bias0=None), dict(w1=None), dict(b2=None), dict(uids=None), dict(iids=None), dict(labels=None),
             dict(loss=None), dict(pred=None), dict(stats=None), dict(ws=None), dict(ld_emb=12), dict(ld_emb=18),
             dict(emb=fake(misalign=4)), dict(w1=fake(misalign=8)), dict(stats=fake(misalign=4)), dict(dense=fake(misalign=4)),
             dict(rows=fake(misalign=8)), dict(keep1=None), dict(keep2=None), dict(scale=0.0), dict(dense=None), dict(rows=None),
             dict(bn1_mean=None), dict(bn2_var=None), dict(dense=None, rows=None)]


@pytest.mark.parametrize('idx', range(len(TRAIN_BAD)))
def test_train_argument_errors_need_no_device(idx):
    assert train_call(**TRAIN_BAD[idx]) == ERR_ARG, TRAIN_BAD[idx]
    assert _lib.last_error()


@pytest.mark.parametrize('grads', [True, False])
def test_train_short_workspace(grads):
    need = _lib.load().pea_nfm_train_workspace_bytes(100, 16, 8)
    none = {} if grads else dict(dense=None, rows=None, pos=None)
    assert train_call(ws_bytes=need - 1, **none) == ERR_NOMEM


SCORE_ORDER = ('mode', 'n', 'C', 'lo', 'E', 'H', 'U', 'I', 'emb', 'ld_emb', 'lin', 'wf', 'bf', 'w2', 'bias', 'uids', 'iids', 'logits', 'pred',
               'rank', 'auc', 'err', 'stream')


def score_call(**over):
    a = {k: fake() for k in SCORE_ORDER}
    a.update(mode=_lib.NFM_ROWS, n=10, C=5, lo=0, E=16, H=8, U=50, I=60, ld_emb=16, stream=None)
    a.update(over)
    return _lib.load().pea_nfm_score(*[a[k] for k in SCORE_ORDER])


SCORE_BAD = [dict(mode=3), dict(mode=-1), dict(n=-1), dict(E=6), dict(H=132), dict(U=0), dict(I=0), dict(emb=None), dict(lin=None),
             dict(wf=None), dict(bf=None), dict(w2=None), dict(bias=None), dict(uids=None), dict(iids=None), dict(err=None),
             dict(logits=None, pred=None, rank=None, auc=None), dict(C=0), dict(rank=None), dict(auc=None), dict(logits=None),
             dict(mode=_lib.NFM_PAIRS), dict(mode=_lib.NFM_RANGE), dict(mode=_lib.NFM_RANGE, rank=None, auc=None, lo=58),
             dict(mode=_lib.NFM_RANGE, rank=None, auc=None, lo=-1), dict(ld_emb=12), dict(emb=fake(misalign=4)), dict(wf=fake(misalign=8))]


@pytest.mark.parametrize('idx', range(len(SCORE_BAD)))
def test_score_argument_errors_need_no_device(idx):
    assert score_call(**SCORE_BAD[idx]) == ERR_ARG, SCORE_BAD[idx]
    assert _lib.last_error()


def test_fold_argument_errors_need_no_device():
    lib = _lib.load()
    good = [16, 8] + [fake() for _ in range(12)] + [1e-5] + [fake() for _ in range(3)] + [None]
    for k in list(range(2, 14)) + [15, 16, 17]:
        bad = list(good)
        bad[k] = None
        assert lib.pea_nfm_fold(*bad) == ERR_ARG, k
    assert lib.pea_nfm_fold(*([6] + good[1:])) == ERR_ARG and lib.pea_nfm_fold(*([16, 132] + good[2:])) == ERR_ARG


# ---------------------------------------------------------------- the BCE sampling branch
class ToyDataset:
    def __init__(self, strategy, seed=0):
        rng = np.random.RandomState(seed)
        self.cf_loss_type, self.sampling_strategy, self.num_negative_samples = 'BCE', strategy, 3
        self.type_accs, self.num_iids = {'uid': 0, 'iid': 12}, 30
        users = rng.randint(0, 12, size=41)
        self.edge_index_nps = {'user2item': np.stack([users, 12 + rng.randint(0, 30, size=41)]).astype(np.float64)}
        self.test_pos_unid_inid_map = {u: [12 + int(rng.randint(0, 30))] for u in range(12)}
        self.neg_unid_inid_map = {u: sorted((12 + rng.choice(30, size=9, replace=False)).tolist()) for u in range(12)}


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize('strategy', ['random', 'unseen'])
def test_bce_branch_matches_a_numpy_recomputation(strategy):
    ds = ToyDataset(strategy)
    seed_all(2019)
    got = cf_negative_sampling(ds)
    seed_all(2019)
    pos = ds.edge_index_nps['user2item'].T
    m, k = pos.shape[0], 3
    if strategy == 'random':
        neg = np.random.randint(low=12, high=42, size=(m * k, 1))
    else:
        neg = np.vstack([np.random.choice(ds.test_pos_unid_inid_map[u] + ds.neg_unid_inid_map[u], size=(k, 1)) for u in pos[:, 0]])
    rows = np.vstack([np.hstack([pos, np.ones((m, 1))]), np.hstack([np.repeat(pos[:, :1], k, axis=0), neg, np.zeros((m * k, 1))])])
    want = torch.from_numpy(rows).long()[torch.randperm(m * (1 + k))]
    assert got.dtype == torch.int64 and tuple(got.shape) == (m * (1 + k), 3) and torch.equal(got, want)
    assert ds.train_data is got and ds.train_data_length == m * (1 + k)
    assert int(got[:, 2].sum()) == m and set(got[:, 2].tolist()) == {0, 1}
    if strategy == 'unseen':
        for u, i, label in got.tolist():
            assert label == 1 or i in ds.test_pos_unid_inid_map[u] + ds.neg_unid_inid_map[u]


def test_other_loss_types_are_still_refused():
    ds = ToyDataset('random')
    ds.cf_loss_type = 'MSE'
    with pytest.raises(NotImplementedError):
        cf_negative_sampling(ds)


# ---------------------------------------------------------------- the float32 headroom of every GPU training case
@pytest.mark.parametrize('case', nfm_ref.TRAIN_CASES, ids=nfm_ref.case_id)
@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'p0.3'])
def test_float32_restatement_has_headroom(case, masked):
    """The float32 restatement, taken as the peer, must itself pass assert_fp32_close against the float64 truth on every
    output the GPU test compares, and no batch variance may come near the eps of the normalisation."""
    inp = nfm_ref.case_inputs(case)
    masks = nfm_ref.make_masks(inp, 0.3, case[3] + 100) if masked else None
    truth, peer = nfm_ref.run(inp, torch.float64, masks), nfm_ref.run(inp, torch.float32, masks)
    assert min(float(truth['var1'].min()), float(truth['var2'].min())) > 100 * nfm_ref.EPS
    for k in truth:
        assert_fp32_close(peer[k].numpy(), truth[k].numpy(), truth[k].numpy(), what=k)
    assert EPS32 < 1e-6
