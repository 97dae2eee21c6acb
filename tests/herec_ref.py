"""HeRec restated in torch at a chosen dtype (reference models/herec.py:36-46 with the MSE loss of
experiments/herec_solver_bpr.py:108-121), with every gradient -- the per-pair rows of include/peahip.h (pea_herec_train)
included -- and the input maker of the parity tests.  A helper: not collected."""
import numpy as np
import torch

KEYS = ('w', 'b', 'user_emb', 'item_emb', 'user_rk_bias', 'item_rk_bias')


def make_inputs(d, m, b, seed=0, n_user=150, n_item=300, n_other=50, user_pool=40, lead=0, gap=0):
    """`lead` other nodes, the users, `gap` other nodes, the items, `n_other` other nodes at the end.  E_m = 0.5 randn,
    W_m = randn / sqrt(D), b_m = 0.1 randn, the four embedding tables 0.7 D^-0.25 randn; users drawn from a pool of `user_pool`, so ids repeat; labels 1..5.
    On the CPU this gives |pred| with a median near 2 and a maximum near 12 and a loss near 20, every gradient non-zero.
    Returns a dict of float32 / int64 CPU tensors."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * d + m)
    n = lead + n_user + gap + n_item + n_other
    scale = 0.7 * d ** -0.25
    inp = {'tables': [0.5 * torch.randn(n, d, generator=g) for _ in range(m)],
           'w': torch.randn(m, d, d, generator=g) / d ** 0.5,
           'b': 0.1 * torch.randn(m, d, generator=g),
           'user_emb': scale * torch.randn(n_user, d, generator=g),
           'item_emb': scale * torch.randn(n_item, d, generator=g),
           'user_rk_bias': scale * torch.randn(n_user, d, generator=g),
           'item_rk_bias': scale * torch.randn(n_item, d, generator=g),
           'acc_uids': lead, 'acc_iids': lead + n_user + gap, 'num_nodes': n}
    pool = torch.randperm(n_user, generator=g)[:user_pool]
    inp['unids'] = (lead + pool[torch.randint(0, user_pool, (b,), generator=g)]).to(torch.int64)
    inp['inids'] = (lead + n_user + gap + torch.randint(0, n_item, (b,), generator=g)).to(torch.int64)
    inp['labels'] = torch.randint(1, 6, (b,), generator=g).to(torch.float32)
    return inp


def rk_sum(tables, w, b, nids):
    """S(n) = sum_m sigmoid(E_m[n] W_m^T + b_m)"""
    return sum(torch.sigmoid(t[nids] @ w[m].t() + b[m]) for m, t in enumerate(tables))


def pred_of(inp, p, unids, inids):
    lu, li = unids - inp['acc_uids'], inids - inp['acc_iids']
    tables = [t.to(p['w'].dtype) for t in inp['tables']]
    su, si = rk_sum(tables, p['w'], p['b'], unids), rk_sum(tables, p['w'], p['b'], inids)
    return ((p['user_emb'][lu] * p['item_emb'][li]).sum(-1) + (su * p['user_rk_bias'][lu]).sum(-1) +
            (si * p['item_rk_bias'][li]).sum(-1)), su, si


def run(inp, dtype=torch.float64, device='cpu', divide_by=None):
    """pred [B], loss, the gradients of the six parameter tensors (dense) and the per-pair rows g_user = [g ie[i'], g S(u)],
    g_item = [g ue[u'], g S(i)] with g = 2 (pred - label) / B, as numpy arrays of `dtype`.  divide_by: the mean divides by
    this instead of B (a batch some of whose pairs were dropped)."""
    p = {k: inp[k].to(device=device, dtype=dtype).clone().requires_grad_(True) for k in KEYS}
    moved = dict(inp, tables=[t.to(device) for t in inp['tables']])
    unids, inids = inp['unids'].to(device), inp['inids'].to(device)
    labels = inp['labels'].to(device=device, dtype=dtype)
    pred, su, si = pred_of(moved, p, unids, inids)
    bsz = divide_by if divide_by is not None else max(pred.numel(), 1)
    loss = ((pred - labels) ** 2).sum() / bsz
    loss.backward()
    g = (2.0 * (pred - labels) / bsz).detach().unsqueeze(1)
    lu, li = unids - inp['acc_uids'], inids - inp['acc_iids']
    out = {'pred': pred, 'loss': loss, 'd_w': p['w'].grad, 'd_b': p['b'].grad, 'd_user_emb': p['user_emb'].grad,
           'd_item_emb': p['item_emb'].grad, 'd_user_rk_bias': p['user_rk_bias'].grad, 'd_item_rk_bias': p['item_rk_bias'].grad,
           'g_user': torch.cat([g * p['item_emb'][li], g * su], dim=1), 'g_item': torch.cat([g * p['user_emb'][lu], g * si], dim=1)}
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def table_of(inp, dtype=torch.float64, device='cpu'):
    """The [N, D + 4] table of include/peahip.h (pea_herec_table) as a numpy array"""
    p = {k: inp[k].to(device=device, dtype=dtype) for k in KEYS}
    tables = [t.to(device=device, dtype=dtype) for t in inp['tables']]
    nu, ni, d = p['user_emb'].shape[0], p['item_emb'].shape[0], p['w'].shape[1]
    u = torch.arange(inp['acc_uids'], inp['acc_uids'] + nu, device=device)
    i = torch.arange(inp['acc_iids'], inp['acc_iids'] + ni, device=device)
    out = torch.zeros((inp['num_nodes'], d + 4), dtype=dtype, device=device)
    out[u, :d], out[u, d] = p['user_emb'], 1.0
    out[u, d + 1] = (rk_sum(tables, p['w'], p['b'], u) * p['user_rk_bias']).sum(-1)
    out[i, :d], out[i, d + 1] = p['item_emb'], 1.0
    out[i, d] = (rk_sum(tables, p['w'], p['b'], i) * p['item_rk_bias']).sum(-1)
    return out.cpu().numpy()


def load_model(model, inp):
    """Copy the inputs' parameters into a HeRecRecsysModel (state-dict names of the reference)."""
    sd = {'user_emb.weight': inp['user_emb'], 'item_emb.weight': inp['item_emb'], 'user_rk_bias.weight': inp['user_rk_bias'],
          'item_rk_bias.weight': inp['item_rk_bias']}
    for m in range(inp['w'].shape[0]):
        sd['emb_trans.%d.weight' % m] = inp['w'][m]
        sd['emb_trans.%d.bias' % m] = inp['b'][m]
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model


def golden_inputs(z):
    """The fixture tests/golden/herec_small.npz as the dict make_inputs returns"""
    m = int(z['num_tables'])
    return {'tables': [torch.from_numpy(z['table_%d' % k]) for k in range(m)],
            'w': torch.stack([torch.from_numpy(z['sd.emb_trans.%d.weight' % k]) for k in range(m)]),
            'b': torch.stack([torch.from_numpy(z['sd.emb_trans.%d.bias' % k]) for k in range(m)]),
            'user_emb': torch.from_numpy(z['sd.user_emb.weight']), 'item_emb': torch.from_numpy(z['sd.item_emb.weight']),
            'user_rk_bias': torch.from_numpy(z['sd.user_rk_bias.weight']), 'item_rk_bias': torch.from_numpy(z['sd.item_rk_bias.weight']),
            'acc_uids': int(z['acc_uids']), 'acc_iids': int(z['acc_iids']), 'num_nodes': int(z['num_nodes']),
            'unids': torch.from_numpy(z['unids']), 'inids': torch.from_numpy(z['inids']), 'labels': torch.from_numpy(z['labels'])}
