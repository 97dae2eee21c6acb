"""GPU: the two-step schedule's dense kernels over every configuration their dispatch accepts, not only the presets.

csrc/mlp2.hip chains both layer transforms (inference, TRAIN and SAGE variants, instantiated for emb, hidden in {64, 128}),
csrc/mlp2_bwd.hip runs the first layer's backward data path (NQ = ceil(k / 8) k-chunks of product 1, k = repr_dim, SAGE
2 x repr_dim).  Here every (kind, emb, hidden) meets repr_dim values that hit each masked-store tail and each NQ, with more
channels than one LDS pass holds (an uneven last channel group wherever a pass holds more than one), GCN under both degree
sides, and both sides of the channel limits (P = 32 / 33 for the fused path, P * R = 1024 for the HIP training head).  The
truth is the CPU oracle and float64 torch (forward) or float64 autograd (training step); the level-wise schedule on the same
parameters is a second check."""
import numpy as np
import pytest
import torch

from helpers import assert_fp32_close, build_model, f64_forward, random_hin, random_state_dict
from test_gpu_backward import f64_loss_and_grads
from test_gpu_edge_cases import _check, _kernel_names_of_one_forward

pytestmark = pytest.mark.gpu

# channels per LDS pass of csrc/mlp2.hip (launch_mlp2_v: weight images that fit 160 KB - 2 KB), by (kind is SAGE, emb, hidden)
_PER_PASS = {(False, 64, 64): 6, (False, 64, 128): 3, (False, 128, 64): 3, (False, 128, 128): 1,
             (True, 64, 64): 3, (True, 64, 128): 1, (True, 128, 64): 2, (True, 128, 128): 1}
# channel counts that need more than one pass, with an uneven last group where a pass holds more than one channel
# (passes are evened out: 7 at 6 per pass runs 4 + 3, 5 at 3 per pass 3 + 2, 3 at 2 per pass 2 + 1)
_CHANNELS = {(False, 64, 64): 7, (False, 64, 128): 5, (False, 128, 64): 5, (False, 128, 128): 2,
             (True, 64, 64): 5, (True, 64, 128): 2, (True, 128, 64): 3, (True, 128, 128): 2}


def _groups(kind, emb, hidden, P):
    """The channel groups launch_mlp2_v forms for P channels."""
    most = _PER_PASS[(kind == 'sage', emb, hidden)]
    passes = -(-P // min(most, P))
    per = -(-P // passes)
    return [min(per, P - g * per) for g in range(passes)]


_GRAPH = []


def _graph():
    """One graph for the whole module: N = 1553 (not a multiple of 32), ~21 k edges.  Under u2i every user is a row without
    in-edges that has out-edges (mlp2_load's lone-row branch; GCN 'row': dinv^2 = 1 / (outdeg + 1) != 1), item i0 + 1 is rated
    by every user (1100 > kChunk = 512 kept edges: its chunks merge), a2i and u2i carry duplicated (multi-)edges, and u2i runs
    together with its reverse."""
    if not _GRAPH:
        n, blocks, rel = random_hin(61, n_user=1100, n_item=420, n_attr=30, e_u2i=18000, e_attr=1500)
        u2i, a2i = rel['u2i'], rel['a2i']
        rng = np.random.default_rng(61)
        extra = np.stack([rng.integers(*blocks['u'], 40), rng.integers(*blocks['i'], 40)])
        u2i = np.concatenate([u2i, extra, extra], axis=1).astype(np.int64)
        assert n % 32 != 0
        deg_in, deg_out = np.bincount(u2i[1], minlength=n), np.bincount(u2i[0], minlength=n)
        assert ((deg_in == 0) & (deg_out > 0)).sum() >= 1000 and deg_in.max() > 512
        flip = lambda e: np.ascontiguousarray(e[::-1])
        _GRAPH.extend([n, blocks, [[u2i, flip(u2i)], [flip(u2i), u2i], [a2i, flip(u2i)], [flip(a2i), a2i]]])
    return _GRAPH


def _edges(P):
    metapaths = _graph()[2]
    return [metapaths[p % len(metapaths)] for p in range(P)]


def _np(t):
    return t.detach().cpu().numpy()


def _forward_case(kind, emb, hidden, repr_dim, P, deg, monkeypatch, fused=True):
    """The two-step forward (fused=False: the level-wise path of a model the two-step schedule refuses) against the oracle
    and float64 (test_gpu_edge_cases._check); then against the level-wise schedule (PEA_FUSED2=0) on the same parameters."""
    n = _graph()[0]
    edges, steps = _edges(P), [2] * P
    monkeypatch.setenv('PEA_FUSED2', '1')
    model = _check(kind, n, edges, steps, emb, hidden, repr_dim, seed=P + repr_dim, gcn_deg_from=deg)
    names = _kernel_names_of_one_forward(model)
    assert ('mlp2_fused' in names) == fused, sorted(names)
    with torch.no_grad():
        _, stack = model.forward(return_stack=True)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    monkeypatch.setenv('PEA_FUSED2', '0')             # read when the engine is made: a fresh model
    ref = build_model(kind, n, edges, steps, emb, hidden, repr_dim, gcn_deg_from=deg, state_dict=sd)
    ref.eval()
    assert 'mlp2_fused' not in _kernel_names_of_one_forward(ref)
    with torch.no_grad():
        _, lw_stack = ref.forward(return_stack=True)
    _, t_stack = f64_forward(kind, {k: v.numpy() for k, v in sd.items()}, edges, steps, 1, 'att', gcn_deg_from=deg)
    assert_fp32_close(_np(stack), _np(lw_stack), t_stack, what='two-step vs level-wise stack')


def _forward_params():
    out = []
    for kind in ('gat', 'gcn', 'sage'):
        for emb in (64, 128):
            for hidden in (64, 128):
                for r in ((4, 12, 16) if kind == 'sage' else (4, 12, 32)):
                    for deg in (('row', 'col') if kind == 'gcn' else ('row',)):
                        out.append(pytest.param(kind, emb, hidden, r, deg, id='%s-%d-%d-r%d%s' % (
                            kind, emb, hidden, r, '-' + deg if kind == 'gcn' else '')))
    return out


@pytest.mark.parametrize('kind,emb,hidden,repr_dim,deg', _forward_params())
def test_two_step_forward_matrix(kind, emb, hidden, repr_dim, deg, monkeypatch):
    """csrc/mlp2.hip inference at each of its 8 instantiations, every masked store tail (repr 4, 12) and the full 32-row
    second product (GAT / GCN repr 32; SAGE repr 16 fills T_1 and the root term side by side), several channel groups."""
    P = _CHANNELS[(kind == 'sage', emb, hidden)]
    groups = _groups(kind, emb, hidden, P)
    assert len(groups) > 1 and (groups[0] == 1 or groups[-1] < groups[0]), groups
    _forward_case(kind, emb, hidden, repr_dim, P, deg, monkeypatch)


def _batch(seed, size=400):
    blocks = _graph()[1]
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(*blocks['u'], size=size), rng.integers(*blocks['i'], size=size),
                     rng.integers(*blocks['i'], size=size)], axis=1).astype(np.int64)


def _train_case(kind, width, repr_dim, P, deg, monkeypatch, two_step=True):
    """One training step, model.loss(b).backward(), on the two-step schedule (two_step=False: a model it refuses) and on the
    level-wise one (PEA_FUSED2_TRAIN=0) with the same parameters, loss and every gradient against float64 autograd; the
    tolerance of test_gpu_backward.py::test_two_step_training_schedule_matches_float64_and_the_levelwise_schedule."""
    from graph_recsys_benchmark_amd.autograd import _Layout
    n = _graph()[0]
    edges, steps = _edges(P), [2] * P
    batch = _batch(P + repr_dim)
    bt = torch.from_numpy(batch).cuda()
    results, sd = {}, None
    for mode in ('1', '0'):
        monkeypatch.setenv('PEA_FUSED2_TRAIN', mode)
        model = build_model(kind, n, edges, steps, width, width, repr_dim, gcn_deg_from=deg)
        model.load_state_dict(random_state_dict(model, 12 + repr_dim, scale=0.2) if sd is None else sd)
        model.train()
        model.zero_grad()
        loss = model.loss(bt)
        loss.backward()
        assert _Layout(model._train_engine).two_step_train == (two_step and mode == '1'), mode
        results[mode] = (float(loss), {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in model.named_parameters()})
        if sd is None:
            sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want_loss, want = f64_loss_and_grads(kind, {k: v.numpy() for k, v in sd.items()}, edges, steps, 1, 'att', batch,
                                         gcn_deg_from=deg)
    g_max = max(np.abs(w).max() for w in want.values())
    for mode, (loss, grads) in results.items():
        np.testing.assert_allclose(loss, want_loss, rtol=2e-5)
        assert set(grads) == set(want)
        for name, w in want.items():
            err = np.abs(grads[name] - w).max()
            assert err <= 2e-4 * np.abs(w).max() + 1e-6 * g_max, 'schedule %s, %s: max err %.3e vs scale %.3e' % (
                mode, name, err, np.abs(w).max())


def _train_params():
    out = []
    for kind in ('gat', 'gcn', 'sage'):
        for width in (64, 128):
            for r in ((4, 8, 12, 16) if kind == 'sage' else (4, 12, 20, 32)):
                for deg in (('row', 'col') if kind == 'gcn' else ('row',)):
                    out.append(pytest.param(kind, width, r, deg, id='%s-%d-r%d%s' % (
                        kind, width, r, '-' + deg if kind == 'gcn' else '')))
    return out


@pytest.mark.parametrize('kind,width,repr_dim,deg', _train_params())
def test_two_step_training_matrix(kind, width, repr_dim, deg, monkeypatch):
    """mlp2 TRAIN + csrc/mlp2_bwd.hip through model.loss(b).backward(): NQ 1, 2, 3, 4 of the backward's product 1 (GAT / GCN
    k = repr 4, 12, 20, 32; SAGE k = 2 x repr 8, 16, 24, 32) at HT = OT = 2 and 4, several channel groups."""
    _train_case(kind, width, repr_dim, _CHANNELS[(kind == 'sage', width, width)], deg, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# channel-count boundaries: kMaxMlp2Chan = 32 channels on the two-step path; P * R <= 1024 for the HIP training head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['gat', 'gcn'])
def test_thirty_two_channels_take_the_two_step_forward(kind, monkeypatch):
    """P = kMaxMlp2Chan = 32: the launch descriptor's last channel entries lie past byte 4096 of the kernel argument; every
    channel of the stack is compared."""
    _forward_case(kind, 64, 64, 16, 32, 'row', monkeypatch)


@pytest.mark.parametrize('kind', ['gat', 'sage'])
def test_thirty_three_channels_take_the_levelwise_forward(kind, monkeypatch):
    _forward_case(kind, 64, 64, 16, 33, 'row', monkeypatch, fused=False)


def test_hip_training_head_predicate_matches_its_gradient_scatter():
    """models/base.py takes the HIP head (csrc/bpr_train.hip) where engine.bpr_train_supported holds, and its backward puts
    the batch's gradient rows back with rows_scatter_sum: both sides of the one predicate, at P * R = 1024 and past it."""
    from graph_recsys_benchmark_amd import _lib, engine
    assert engine.bpr_train_supported(32, 32) and engine.bpr_train_supported(64, 16) and engine.bpr_train_supported(1, 32)
    assert not engine.bpr_train_supported(33, 32) and not engine.bpr_train_supported(40, 28)
    assert not engine.bpr_train_supported(64, 32) and not engine.bpr_train_supported(1, 36)
    ids = torch.tensor([0, 2, 2, -1], dtype=torch.int64, device='cuda')
    for p, r in ((32, 32), (64, 16), (33, 32), (40, 28)):
        src = torch.randn(4, p * r, device='cuda')
        dst = torch.zeros(4, p * r, device='cuda')
        cols = [(p - 1 - q) * r for q in range(p)]
        if engine.bpr_train_supported(p, r):
            engine.rows_scatter_sum(ids, src, p, r, cols, dst)
            want = torch.zeros_like(dst)
            for q in range(p):
                want[0, cols[q]:cols[q] + r] = src[0, q * r:(q + 1) * r]
                want[2, cols[q]:cols[q] + r] = src[1, q * r:(q + 1) * r] + src[2, q * r:(q + 1) * r]
            assert torch.equal(dst, want), (p, r)
        else:
            with pytest.raises(_lib.PeaError):
                engine.rows_scatter_sum(ids, src, p, r, cols, dst)


@pytest.mark.parametrize('kind', ['gat', 'sage'])
def test_thirty_two_channels_train_on_the_two_step_schedule(kind, monkeypatch):
    """P = 32 on the two-step training schedule; GAT at repr 32 is P * R = 1024, exactly the HIP head's limit."""
    _train_case(kind, 64, 16 if kind == 'sage' else 32, 32, 'row', monkeypatch)


def test_thirty_three_channels_of_width_32_train_past_the_head_limit(monkeypatch):
    """P = 33, repr 32: P * R = 1056 > 1024.  Neither the two-step schedule (P > 32) nor the HIP head (its gradient scatter
    takes P * R <= 1024) may be chosen; the step matches float64 autograd."""
    from graph_recsys_benchmark_amd import engine
    _train_case('gat', 64, 32, 33, 'row', monkeypatch, two_step=False)
    assert not engine.bpr_train_supported(33, 32)
