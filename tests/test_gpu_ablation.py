"""GPU: the one-pass metapath ablation sweep (csrc/ablate.hip) against the per-mask entry points it replaces.

The contract is bitwise: variant v of pea_fuse_ablate / pea_model_forward_ablate / pea_rank_eval_multi equals pea_fuse /
pea_model_forward (masked_channel = v - 1) / pea_rank_eval on table v, so every comparison against those is torch.equal.
Against the reference's own fixtures (tests/golden) and the C oracle the project's fp32 bound applies (rtol 1e-5, atol 1e-6,
helpers.assert_fp32_close with a float64 truth)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import (GoldenCase, assert_fp32_close, build_model, f64_forward, golden_cases, model_from_golden, oracle_params,
                     random_hin, random_state_dict)
from graph_recsys_benchmark_amd import _lib, engine, solvers
from graph_recsys_benchmark_amd.utils import SyntheticHIN
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    return _lib.current_stream()


# ------------------------------------------------------------------------------------------------ pea_fuse_ablate
def _fuse_inputs(P, R, N, seed):
    """A stack wider than P * R (8 floats of padding per row, 4 in front) whose channels sit in a permuted column order."""
    g = torch.Generator().manual_seed(seed)
    ld = P * R + 8
    buf = torch.randn(N, ld, generator=g)
    perm = torch.randperm(P, generator=g).tolist()
    cols = [4 + perm[p] * R for p in range(P)]
    att = torch.randn(P, R, generator=g) * 0.3
    return buf.to(DEV), ld, cols, att.to(DEV)


def _pea_fuse(lib, N, P, R, buf, ld, cols_c, att, masked, mode):
    out = torch.empty((N, R), dtype=torch.float32, device=DEV)
    _lib.check(lib.pea_fuse(N, P, R, _lib.ptr(buf), ld, cols_c, _lib.ptr(att), masked, mode, _lib.ptr(out), _stream()))
    return out


def _pea_fuse_ablate(lib, N, P, R, buf, ld, cols_c, att, mode, want_att=True):
    # poisoned outputs: every element must be written
    tables = torch.full((P + 1, N, R), float('nan'), dtype=torch.float32, device=DEV)
    w = torch.full((N, P), float('nan'), dtype=torch.float32, device=DEV) if want_att else None
    _lib.check(lib.pea_fuse_ablate(N, P, R, _lib.ptr(buf), ld, cols_c, _lib.ptr(att), mode, _lib.ptr(tables), _lib.ptr(w),
                                   _stream()))
    return tables, w


@pytest.mark.parametrize('mode', ['att', 'mean'])
@pytest.mark.parametrize('R', [4, 16, 24, 64, 256])
@pytest.mark.parametrize('P', [1, 3, 9, 17, 64])
def test_fuse_ablate_is_bitwise_pea_fuse_per_mask(P, R, mode):
    """P = 1, the register-resident paths (3, 9), one past them (17) and kMaxChannels; R = one lane to 64 lanes per row,
    24 = a row that does not fill its lane group; N odd: the last workgroup is partial at every rows-per-workgroup."""
    lib = _lib.require_device()
    N = 1037
    buf, ld, cols, att = _fuse_inputs(P, R, N, seed=1000 * P + R)
    cols_c = (C.c_int * P)(*cols)
    m = _lib.FUSE_ATT if mode == 'att' else _lib.FUSE_MEAN
    tables, w = _pea_fuse_ablate(lib, N, P, R, buf, ld, cols_c, att, m)
    before = buf.clone()
    for v in range(P + 1):
        want = _pea_fuse(lib, N, P, R, buf, ld, cols_c, att, v - 1, m)
        assert torch.equal(tables[v], want), 'variant %d differs from pea_fuse(masked=%d)' % (v, v - 1)
    again, w2 = _pea_fuse_ablate(lib, N, P, R, buf, ld, cols_c, att, m)
    assert torch.equal(again, tables) and torch.equal(w2, w)            # reproducible
    assert torch.equal(buf, before)                                     # the stack is only read
    no_att, none = _pea_fuse_ablate(lib, N, P, R, buf, ld, cols_c, att, m, want_att=False)
    assert none is None and torch.equal(no_att, tables)
    # fusion weights of the unmasked variant
    stack = torch.stack([buf[:, c:c + R] for c in cols], dim=1).cpu()
    if mode == 'att':
        want32 = torch.softmax((stack * att.cpu()).sum(-1), dim=-1).numpy()
        truth = torch.softmax((stack.double() * att.cpu().double()).sum(-1), dim=-1).numpy()
    else:
        truth = np.full((N, P), 1.0 / P)
        want32 = truth.astype(np.float32)
    assert_fp32_close(_np(w), want32, truth, rtol=RTOL, atol=ATOL, what='out_att')
    assert np.abs(_np(w).astype(np.float64).sum(axis=1) - 1.0).max() <= RTOL + ATOL


def test_fuse_ablate_python_wrapper_and_argument_errors():
    lib = _lib.require_device()
    g = torch.Generator().manual_seed(3)
    stack = torch.randn(513, 5, 16, generator=g).to(DEV)
    att = (torch.randn(1, 5, 16, generator=g) * 0.3).to(DEV)
    cols_c = (C.c_int * 5)(*[p * 16 for p in range(5)])
    for mode, m in (('att', _lib.FUSE_ATT), ('mean', _lib.FUSE_MEAN)):
        tables, w = engine.fuse_ablate(stack, att, mode)
        assert tables.shape == (6, 513, 16) and w.shape == (513, 5)
        for v in range(6):
            assert torch.equal(tables[v], _pea_fuse(lib, 513, 5, 16, stack, 80, cols_c, att.view(5, 16), v - 1, m))
    out = torch.empty((6, 513, 16), device=DEV)
    bad_cols = (C.c_int * 5)(0, 16, 32, 48, 72)                         # last channel runs past the row
    assert lib.pea_fuse_ablate(513, 5, 16, _lib.ptr(stack), 80, bad_cols, _lib.ptr(att), 0, _lib.ptr(out), None, _stream()) == -1
    assert lib.pea_fuse_ablate(513, 65, 16, _lib.ptr(stack), 80, cols_c, _lib.ptr(att), 0, _lib.ptr(out), None, _stream()) == -1
    assert lib.pea_fuse_ablate(513, 5, 16, _lib.ptr(stack), 80, cols_c, None, 0, _lib.ptr(out), None, _stream()) == -1
    assert lib.pea_fuse_ablate(513, 5, 16, _lib.ptr(stack), 80, cols_c, _lib.ptr(att), 2, _lib.ptr(out), None, _stream()) == -1


# ------------------------------------------------------------------------------------------------ forward_ablate
def _assert_bitwise_the_eval_loop(model):
    """eval_ablation()'s tables against model.eval() / model.eval(p); returns the tables."""
    model.eval_ablation()
    tables, att = model.ablation_repr, model.ablation_att
    P = len(model.meta_path_steps)
    assert tables.shape[0] == P + 1 and att.shape == (tables.shape[1], P)
    assert model.cached_repr.data_ptr() == tables.data_ptr() and torch.equal(model.cached_repr, tables[0])   # a view
    assert not model.training
    model.eval()
    assert model.ablation_repr is None and model.ablation_att is None
    assert torch.equal(model.cached_repr, tables[0]), 'variant 0 differs from eval()'
    for p in range(P):
        model.eval(p)
        assert torch.equal(model.cached_repr, tables[1 + p]), 'variant %d differs from eval(%d)' % (1 + p, p)
    return tables, att


@pytest.mark.parametrize('name', golden_cases())
def test_forward_ablate_on_the_reference_fixtures(name):
    g = GoldenCase(name)
    model = model_from_golden(g)
    tables, att = _assert_bitwise_the_eval_loop(model)
    np.testing.assert_allclose(_np(tables[0]), g.out['repr'], rtol=RTOL, atol=ATOL)          # the reference's own output
    np.testing.assert_allclose(_np(tables[2]), g.out['repr_mask1'], rtol=RTOL, atol=ATOL)
    assert np.abs(_np(att).astype(np.float64).sum(axis=1) - 1.0).max() <= RTOL + ATOL
    model.eval_ablation(keep_att=False)
    assert model.ablation_att is None and torch.equal(model.ablation_repr, tables)
    model.train()
    assert model.ablation_repr is None


def test_golden_cases_cover_every_kind():
    assert {GoldenCase(n).kind for n in golden_cases()} == {'gat', 'gcn', 'sage'}


def _f64_fuse(stack64, att, mode, masked):
    s = np.array(stack64, dtype=np.float64)
    if masked is not None:
        s[:, masked] = 0.0
    if mode == 'mean':
        return s.mean(axis=1)
    t = torch.from_numpy(s)
    w = torch.softmax((t * torch.from_numpy(np.asarray(att, np.float64)).reshape(1, *s.shape[1:])).sum(-1), dim=-1)
    return (t * w.unsqueeze(-1)).sum(1).numpy()


def _wide_model(kind, aggr='att'):
    """emb = hidden = 64, 2-step channels: what the two-step inference schedule accepts.  Hub rows, multi-edges, self loops."""
    n, blocks, rel = random_hin(23, n_user=900, n_item=300, n_attr=25, e_u2i=9000, e_attr=1200)
    u2i, a2i = rel['u2i'], rel['a2i']
    flip = lambda e: np.ascontiguousarray(e[::-1])
    edges = [[u2i, flip(u2i)], [flip(u2i), u2i], [a2i, flip(u2i)], [flip(a2i), a2i], [u2i, flip(a2i)]]
    steps = [2] * len(edges)
    model = build_model(kind, n, edges, steps, 64, 64, 16, channel_aggr=aggr)
    model.load_state_dict(random_state_dict(model, 41))
    return model, edges, steps


def _kernel_names(fn):
    lib = _lib.load()
    lib.pea_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.pea_profile_enable(0)
    cap = 4096
    names, cnt = C.create_string_buffer(cap * 32), C.c_int()
    lib.pea_profile_read(cap, names, None, None, C.byref(cnt))
    return [names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode() for i in range(cnt.value)]


def _wide_case(kind, aggr, two_step):
    model, edges, steps = _wide_model(kind, aggr)
    names = _kernel_names(model.eval_ablation)
    assert ('mlp2_fused' in names) == two_step, names
    assert names.count('fuse_ablate') == 1 and 'fuse' not in names, names      # the fusion launch is REPLACED
    tables, _ = _assert_bitwise_the_eval_loop(model)
    sd, cps, hls = oracle_params(model, steps, kind)
    _, t_stack = f64_forward(kind, sd, edges, steps, 1, aggr)
    for v in range(len(steps) + 1):
        masked = v - 1 if v else None
        want = orc.pea_forward(kind, sd['x'], edges, cps, hls, att=sd.get('att'), channel_aggr=aggr, metapath_idx=masked)
        assert_fp32_close(_np(tables[v]), want, _f64_fuse(t_stack, sd.get('att'), aggr, masked), rtol=RTOL, atol=ATOL,
                          what='%s variant %d vs oracle' % (kind, v))


@pytest.mark.parametrize('aggr', ['att', 'mean'])
@pytest.mark.parametrize('kind', ['gat', 'gcn', 'sage'])
def test_forward_ablate_on_the_two_step_schedule(kind, aggr, monkeypatch):
    monkeypatch.setenv('PEA_FUSED2', '1')
    _wide_case(kind, aggr, two_step=True)


def levelwise_child():
    """Body of the child process of the test below (PEA_FUSED2=0 in its environment from the start)."""
    assert os.environ.get('PEA_FUSED2') == '0'
    for kind in ('gat', 'gcn', 'sage'):
        _wide_case(kind, 'att', two_step=False)
    _wide_case('gat', 'mean', two_step=False)
    for name in golden_cases():
        _assert_bitwise_the_eval_loop(model_from_golden(GoldenCase(name)))
    print('ABLATION-LEVELWISE-OK')


def test_forward_ablate_on_the_level_wise_schedule_in_a_fresh_process():
    """PEA_FUSED2=0 for the whole life of a process of its own: the same checks on the level-wise schedule."""
    env = dict(os.environ, PEA_FUSED2='0')
    code = ('import sys; sys.path[:0] = [%r, %r]; import test_gpu_ablation as t; t.levelwise_child()' % (HERE, ROOT))
    flags = ['-s'] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + ['-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and 'ABLATION-LEVELWISE-OK' in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


# ------------------------------------------------------------------------------------------------ rank_eval_multi
def _scorer(R, seed):
    torch.manual_seed(seed)
    fc1, fc2 = torch.nn.Linear(2 * R, R), torch.nn.Linear(R, 1)
    return [t.detach().to(DEV) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]


@pytest.mark.parametrize('R', [16, 8, 64])
@pytest.mark.parametrize('C_', [100, 201, 2])
@pytest.mark.parametrize('shared', [True, False])
def test_rank_eval_multi_is_bitwise_rank_eval_per_table(shared, C_, R):
    """C = 100 (the reference's 1 + 99: two wave passes), 1 + 200 (four: past the ids kept in registers), 2 (one negative);
    R = 16 (rows in registers) and the generic widths; U = 37 leaves the last workgroup partial."""
    V, N, U = 5, 700, 37
    g = torch.Generator().manual_seed(C_ + R)
    tables = torch.randn(V, N, R, generator=g).to(DEV)
    unids = torch.randint(0, N, (U,), generator=g).to(DEV)
    cand = torch.randint(0, N, (U, C_) if shared else (V, U, C_), generator=g).to(DEV)
    fc = _scorer(R, 5)
    scores, rank, auc, loss = engine.rank_eval_multi(tables, unids, cand, *fc)
    assert scores.shape == (V, U, C_) and rank.shape == (V, U) and rank.dtype == torch.int32
    for v in range(V):
        want = engine.rank_eval(tables[v], unids, cand if shared else cand[v], *fc)
        for got, w, what in zip((scores[v], rank[v], auc[v], loss[v]), want, ('scores', 'rank', 'auc', 'loss')):
            assert torch.equal(got, w), '%s of variant %d' % (what, v)
    again = engine.rank_eval_multi(tables, unids, cand, *fc)
    assert all(torch.equal(a, b) for a, b in zip(again, (scores, rank, auc, loss)))
    # a contiguous sub-range of the tables, passed as a slice
    sub = engine.rank_eval_multi(tables[1:4], unids, cand if shared else cand[1:4], *fc)
    assert all(torch.equal(a, b[1:4]) for a, b in zip(sub, (scores, rank, auc, loss)))
    # scores = NULL at the C level
    lib = _lib.load()
    rank2 = torch.full((V, U), -1, dtype=torch.int32, device=DEV)
    auc2, loss2 = torch.empty((V, U), device=DEV), torch.empty((V, U), device=DEV)
    rc = lib.pea_rank_eval_multi(V, U, C_, R, N, _lib.ptr(tables), _lib.ptr(unids), _lib.ptr(cand), 0 if shared else U * C_,
                                 _lib.ptr(fc[0]), _lib.ptr(fc[1]), _lib.ptr(fc[2]), _lib.ptr(fc[3]), None, _lib.ptr(rank2),
                                 _lib.ptr(auc2), _lib.ptr(loss2), _stream())
    assert rc == 0 and torch.equal(rank2, rank) and torch.equal(auc2, auc) and torch.equal(loss2, loss)


def test_rank_eval_multi_reports_ids_out_of_range():
    V, N, U, C_, R = 3, 200, 9, 100, 16
    g = torch.Generator().manual_seed(0)
    tables = torch.randn(V, N, R, generator=g).to(DEV)
    unids = torch.randint(0, N, (U,), generator=g).to(DEV)
    fc = _scorer(R, 1)
    for shared in (True, False):
        cand = torch.randint(0, N, (U, C_) if shared else (V, U, C_), generator=g).to(DEV)
        engine.rank_eval_multi(tables, unids, cand, *fc)
        bad_u = unids.clone()
        bad_u[4] = N
        with pytest.raises(IndexError):
            engine.rank_eval_multi(tables, bad_u, cand, *fc)
        for where, value in ((3, -1), (70, N), (C_ - 1, N + 5)):         # first pass, second pass, last column
            bad_c = cand.clone()
            bad_c.view(-1, C_)[-2, where] = value                        # per-variant block: in the LAST variant's rows
            with pytest.raises(IndexError):
                engine.rank_eval_multi(tables, unids, bad_c, *fc)
        engine.rank_eval_multi(tables, unids, cand, *fc)                 # the flag is re-armed
    with pytest.raises(ValueError):
        engine.rank_eval_multi(tables, unids, torch.zeros((2, U, C_), dtype=torch.int64, device=DEV), *fc)
    lib = _lib.load()
    cand = torch.zeros((U, C_), dtype=torch.int64, device=DEV)
    out = torch.empty((V, U), dtype=torch.int32, device=DEV)
    rc = lib.pea_rank_eval_multi(V, U, C_, R, N, _lib.ptr(tables), _lib.ptr(unids), _lib.ptr(cand), 7, _lib.ptr(fc[0]),
                                 _lib.ptr(fc[1]), _lib.ptr(fc[2]), _lib.ptr(fc[3]), None, _lib.ptr(out), None, None, _stream())
    assert rc == -1                                                       # a stride that is neither 0 nor U * C


# ------------------------------------------------------------------------------------------------ the sweep on ml-small
@pytest.fixture(scope='module')
def ml_small():
    ds = SyntheticHIN('ml_small', seed=2019)
    ds.eval_split()
    return ds


@pytest.fixture(scope='module')
def cli_runs(ml_small):
    from graph_recsys_benchmark_amd import pea_solver_bpr
    with_sweep = pea_solver_bpr.main(['--model', 'PEAGCN'], dataset=ml_small)
    repr_with = pea_solver_bpr.main.last_model.cached_repr.clone()
    without = pea_solver_bpr.main(['--model', 'PEAGCN', '--metapath_test', 'false'], dataset=ml_small)
    return with_sweep, repr_with, without, pea_solver_bpr.main.last_model


def _reference_order(model, ds, seed, variants):
    """The reference's loop: model.eval(metapath_idx) then metrics(), one after the other from one seed."""
    np.random.seed(seed)
    rows = []
    for v in variants:
        model.eval(v - 1 if v else None)
        rows.append(solvers.metrics(model, ds))
    return rows


def _assert_rows(got, want_rows):
    hr, ndcg, auc, loss = got
    assert hr.shape == (len(want_rows), 16) and ndcg.shape == (len(want_rows), 16)
    for k, (whr, wndcg, wauc, wloss) in enumerate(want_rows):
        np.testing.assert_array_equal(hr[k], whr)
        np.testing.assert_array_equal(ndcg[k], wndcg)
        np.testing.assert_allclose(auc[k], wauc[0], rtol=1e-6)
        np.testing.assert_allclose(loss[k], wloss[0], rtol=1e-6)


def test_metapath_ablation_equals_the_reference_loop(ml_small, cli_runs):
    model = cli_runs[3]
    P = len(model.meta_path_steps)
    want = _reference_order(model, ml_small, 77, range(P + 1))
    want_state = np.random.get_state()
    model.eval_ablation()
    np.random.seed(77)
    got = solvers.metapath_ablation(model, ml_small)
    state = np.random.get_state()
    assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    _assert_rows(got, want)
    assert len({tuple(r) for r in got[1]}) > 1                            # the masks do change the ranking
    # the metapaths alone (what the CLI runs after its own unmasked metrics), and a non-contiguous choice
    for variants in (range(1, P + 1), [0, 3, 5]):
        want = _reference_order(model, ml_small, 78, variants)
        model.eval_ablation()
        np.random.seed(78)
        _assert_rows(solvers.metapath_ablation(model, ml_small, variants=variants), want)
    # shared candidates: every variant ranked on the one draw
    model.eval_ablation()
    np.random.seed(79)
    hr, ndcg, auc, loss = solvers.metapath_ablation(model, ml_small, shared_candidates=True)
    np.random.seed(79)
    cand = torch.from_numpy(solvers.ablation_candidates(ml_small, 1, shared=True)).to(DEV)
    users = torch.as_tensor(list(ml_small.test_pos_unid_inid_map.keys()), device=DEV)
    for v in range(P + 1):
        _, rank, a, l = engine.rank_eval(model.ablation_repr[v], users, cand, model.fc1.weight, model.fc1.bias, model.fc2.weight,
                                         model.fc2.bias)
        whr, wndcg = solvers.metrics_from_ranks(rank.cpu().numpy())
        np.testing.assert_array_equal(hr[v], whr.mean(axis=0))
        np.testing.assert_array_equal(ndcg[v], wndcg.mean(axis=0))
        np.testing.assert_allclose(auc[v], a.double().mean().item(), rtol=1e-6)
        np.testing.assert_allclose(loss[v], l.double().mean().item(), rtol=1e-6)
    model.train()
    with pytest.raises(RuntimeError, match='eval_ablation'):
        solvers.metapath_ablation(model, ml_small)


def test_explain_and_the_eval_cache_readers(ml_small, cli_runs):
    model = cli_runs[3]
    P = len(model.meta_path_steps)
    rng = np.random.default_rng(4)
    u0, i0 = ml_small.type_accs['uid'], ml_small.type_accs['iid']
    unids = torch.from_numpy(rng.integers(u0, u0 + ml_small.num_uids, size=50)).to(DEV)
    inids = torch.from_numpy(rng.integers(i0, i0 + ml_small.num_iids, size=50)).to(DEV)
    item_range = (i0, i0 + ml_small.num_iids)
    model.eval()
    with pytest.raises(RuntimeError, match='eval_ablation'):
        model.explain(unids, inids)
    want_score = model.predict(unids, inids).view(-1).clone()
    want_rec = model.recommend(unids, 10, item_range)
    want_full = solvers.metrics_full_from_dataset(model, ml_small)
    np.random.seed(11)
    want_metrics = solvers.metrics(model, ml_small)
    want_without = []
    for p in range(P):
        model.eval(p)
        want_without.append(model.predict(unids, inids).view(-1).clone())
    model.eval_ablation()
    ex = model.explain(unids, inids)
    assert torch.equal(ex['score'], want_score) and torch.equal(model.predict(unids, inids).view(-1), want_score)
    assert ex['score_without'].shape == (50, P)
    for p in range(P):
        assert torch.equal(ex['score_without'][:, p], want_without[p]), p
    assert torch.equal(ex['att_user'], model.ablation_att[unids]) and torch.equal(ex['att_item'], model.ablation_att[inids])
    got_rec = model.recommend(unids, 10, item_range)
    assert torch.equal(got_rec[0], want_rec[0]) and torch.equal(got_rec[1], want_rec[1])
    for a, b in zip(solvers.metrics_full_from_dataset(model, ml_small), want_full):
        np.testing.assert_array_equal(a, b)
    np.random.seed(11)
    for a, b in zip(solvers.metrics(model, ml_small), want_metrics):
        np.testing.assert_array_equal(a, b)
    model.eval_ablation(keep_att=False)
    ex = model.explain(unids, inids)
    assert ex['att_user'] is None and ex['att_item'] is None and torch.equal(ex['score'], want_score)
    with pytest.raises(IndexError):
        model.explain(torch.tensor([model.x.shape[0]], device=DEV), inids[:1])


def test_cli_runs_the_sweep_and_keeps_every_existing_value(ml_small, cli_runs):
    with_sweep, repr_with, without, model = cli_runs
    assert 'metapath_test' not in without
    assert set(with_sweep) == set(without) | {'metapath_test'}
    for k, v in without.items():
        assert with_sweep[k] == v, k                                      # exactly, floats included
    model.eval()
    assert torch.equal(repr_with, model.cached_repr)                      # the table left cached: eval()'s bytes
    sweep = with_sweep['metapath_test']
    assert len(sweep) == 9 and [e['metapath_idx'] for e in sweep] == list(range(9))
    # reference order from the CLI's seed (2019 + 1): unmasked metrics first, then metapath 0 .. 8
    rows = _reference_order(model, ml_small, 2020, range(10))
    hr, ndcg, auc, loss = rows[0]
    assert without['HR@10'] == float(hr[5]) and without['NDCG@20'] == float(ndcg[15]) and without['AUC'] == float(auc[0])
    for p, e in enumerate(sweep):
        hr, ndcg, auc, loss = rows[1 + p]
        for name, k in (('5', 0), ('10', 5), ('20', 15)):
            assert e['HR@' + name] == float(hr[k]) and e['NDCG@' + name] == float(ndcg[k])
        np.testing.assert_allclose(e['AUC'], auc[0], rtol=1e-6)
        np.testing.assert_allclose(e['eval_loss'], loss[0], rtol=1e-6)
