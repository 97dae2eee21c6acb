"""CFKG restated in torch at a chosen dtype (reference models/cfkg.py:21-27 with the kg_loss of
experiments/cfkg_solver_bpr.py:95-106), with every gradient -- the per-quadruple rows of include/peahip_kge.h (pea_cfkg_train)
included -- the input maker of the parity tests and the small dataset objects the model and the sampler read.  A helper: not
collected."""
import numpy as np
import torch


class FakeDataset:
    """What CFKGRecsysModel and kg_negative_sampling read from a dataset: users at `acc_uids`, `relations` = ordered
    {name: float64 [2, E] edge array}, each typed by its position"""

    def __init__(self, num_nodes, num_uids, acc_uids, relations, num_edge_types=None):
        self.num_nodes, self.num_uids = int(num_nodes), int(num_uids)
        self.type_accs = {'uid': int(acc_uids)}
        self.edge_index_nps = dict(relations)
        self.edge_type_dict = {name: k for k, name in enumerate(self.edge_index_nps)}
        self.num_edge_types = len(self.edge_type_dict) if num_edge_types is None else int(num_edge_types)

    def __getitem__(self, key):
        return getattr(self, key)


def model_dataset(num_nodes, num_uids, acc_uids, num_rel, rating_r_idx=0):
    """A dataset with `num_rel` edge types whose 'user2item' is type rating_r_idx (the edge arrays are empty: the model reads
    none)"""
    names = ['rel%d' % k for k in range(num_rel)]
    names[rating_r_idx] = 'user2item'
    return FakeDataset(num_nodes, num_uids, acc_uids, {k: np.zeros((2, 0)) for k in names})


def sampling_dataset(seed=5, n_user=30, n_item=45, n_other=12):
    """Three relations over a small graph, as kg_negative_sampling reads them (float64 edge arrays, like the reference's)"""
    rng = np.random.default_rng(seed)
    u0, i0, o0 = 0, n_user, n_user + n_item
    rel = {'user2item': np.stack([rng.integers(u0, i0, 150), rng.integers(i0, o0, 150)]),
           'attr2item': np.stack([rng.integers(o0, o0 + n_other, 40), rng.integers(i0, o0, 40)]),
           'attr2user': np.stack([rng.integers(o0, o0 + n_other, 25), rng.integers(u0, i0, 25)])}
    return FakeDataset(o0 + n_other, n_user, u0, {k: v.astype(np.float64) for k, v in rel.items()})


def sorted_rows(rows):
    """The rows of an int array in lexicographic order (the shuffle of the sampler taken out)"""
    rows = np.asarray(rows)
    return rows[np.lexsort(rows.T[::-1])]


def make_inputs(e, n_rel, b, seed=0, n=500, n_user=150, acc_uids=0, head_pool=40, scale=None, n_item=None):
    """x = a randn(N, E), r = a randn(R, E) with a = 0.7 E^-0.25 (or `scale`): <x_h + r, x_t> has a standard deviation near 0.7,
    so neither half of the loss saturates and no gradient vanishes.  Heads drawn from a pool of `head_pool` nodes, so ids
    repeat; three fixed rows: (7, 7, 9, 0) has h == t+, (3, 50, 50, R-1) has t+ == t-, (9, 9, 9, 0) has one node in all three
    places.  unids / inids: B (user, item) pairs for predict, the items from the `n_item` nodes behind the user block (default: every
    node behind it).  Returns a dict of float32 / int64 CPU tensors."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * e + n_rel)
    a = 0.7 * e ** -0.25 if scale is None else scale
    inp = {'x': a * torch.randn(n, e, generator=g), 'r': a * torch.randn(n_rel, e, generator=g), 'num_nodes': n,
           'acc_uids': acc_uids, 'num_uids': n_user, 'rating_r_idx': min(1, n_rel - 1)}
    pool = torch.randperm(n, generator=g)[:head_pool]
    batch = torch.stack([pool[torch.randint(0, head_pool, (b,), generator=g)], torch.randint(0, n, (b,), generator=g),
                         torch.randint(0, n, (b,), generator=g), torch.randint(0, n_rel, (b,), generator=g)], dim=1)
    fixed = torch.tensor([[7, 7, 9, 0], [3, 50, 50, n_rel - 1], [9, 9, 9, 0]])
    k = min(b, 3)
    batch[:k] = fixed[:k]
    inp['batch'] = batch.to(torch.int64)
    inp['unids'] = acc_uids + torch.randint(0, n_user, (b,), generator=g)
    inp['inids'] = acc_uids + n_user + torch.randint(0, n_item or n - acc_uids - n_user, (b,), generator=g)
    return inp


def kg_compose(x, r, batch):
    """kg_loss of experiments/cfkg_solver_bpr.py:95-106 on tensors: (loss, pos, neg)"""
    h, pos_t, neg_t, rr = x[batch[:, 0]], x[batch[:, 1]], x[batch[:, 2]], r[batch[:, 3]]
    pos = torch.sum((h + rr) * pos_t, dim=-1)
    neg = torch.sum((h + rr) * neg_t, dim=-1)
    return -(pos.sigmoid().log().sum() + (-neg).sigmoid().log().sum()), pos, neg


def run(x, r, batch, dtype=torch.float64):
    """loss, pos, neg, the dense gradients dx and dr, and the rows of include/peahip_kge.h: grad_rows [3B, E] in the order
    h, t+, t- per quadruple (GH, a hr, b hr) and GH [B, E] on its own, as tensors of `dtype` on the device of x"""
    x, r = (t.detach().to(dtype).requires_grad_(True) for t in (x, r))
    rows = [x[batch[:, 0]], x[batch[:, 1]], x[batch[:, 2]], r[batch[:, 3]]]
    for t in rows:
        t.retain_grad()
    pos = torch.sum((rows[0] + rows[3]) * rows[1], dim=-1)
    neg = torch.sum((rows[0] + rows[3]) * rows[2], dim=-1)
    loss = -(pos.sigmoid().log().sum() + (-neg).sigmoid().log().sum())
    loss.backward()
    grad_rows = torch.stack([rows[0].grad, rows[1].grad, rows[2].grad], dim=1).reshape(-1, x.shape[1])
    return dict(loss=loss.detach(), pos=pos.detach(), neg=neg.detach(), dx=x.grad, dr=r.grad, grad_rows=grad_rows, gh=rows[3].grad)


def predict_of(x, r, rating_r_idx, unids, inids):
    """forward of models/cfkg.py:21-27"""
    return torch.exp(torch.sum((x[unids] + r[rating_r_idx]) * x[inids], dim=-1))


def load_model(model, x, r):
    """Copy x and r into a CFKGRecsysModel (state-dict names of the reference)"""
    model.load_state_dict({'x': torch.as_tensor(np.asarray(x)), 'r': torch.as_tensor(np.asarray(r))}, strict=True)
    return model


def golden_inputs(z):
    """The fixture tests/golden/cfkg_small.npz as the dict make_inputs returns"""
    return {'x': torch.from_numpy(z['sd.x']), 'r': torch.from_numpy(z['sd.r']), 'num_nodes': int(z['num_nodes']),
            'acc_uids': int(z['acc_uids']), 'num_uids': int(z['num_uids']), 'rating_r_idx': int(z['rating_r_idx']),
            'batch': torch.from_numpy(z['batch']), 'unids': torch.from_numpy(z['unids']), 'inids': torch.from_numpy(z['inids'])}
