"""CFKG (reference graph_recsys_benchmark/models/cfkg.py, with the kg_loss its driver adds at
experiments/cfkg_solver_bpr.py:95-106): the KG-embedding baseline of the reference's result table.

    predict(u, i)          = exp(<x[u] + r[user2item], x[i]>)
    kg_loss(h, t+, t-, rel) = -(sum log sigmoid(<x[h] + r[rel], x[t+]>) + sum log sigmoid(-<x[h] + r[rel], x[t-]>))

The model trains through kg_loss alone, one step per batch of every KG triple.  forward() is the reference's torch composition
and runs anywhere.  On the GPU, with native=True (the default) and a shape engine.cfkg_supported takes, kg_loss() is one launch
of csrc/cfkg.hip (engine.cfkg_loss: forward, loss and the whole backward, the relation gradient summed inside the launch) plus
the deterministic scatter of the node gradient rows.  eval() builds cached_repr [N, E] in torch (an exact add, not hot): x
with r[user2item] added to the rows of the user block, so the plain dot of a user row and an item row is log predict(u, i)
and predict in eval mode, rank_eval, rank_full, recommend and solvers.metrics / metrics_full run on the inner-product kernels
of csrc/dot_score.hip unchanged.

Limits: ranks and AUC are taken on the log-score; they equal the reference's except where its exp saturates to equal values.
The eval-mode routes assume unids lie in the user block and items outside it (forward takes any ids)."""
import torch
import torch.nn.functional as F
from torch.nn import Parameter

from .. import engine as _engine, evaluators
from ..nn.inits import glorot
from .base import GraphRecsysModel


class CFKGRecsysModel(GraphRecsysModel):
    scorer = 'dot'

    def _init(self, **kwargs):
        dataset = kwargs['dataset']
        type_of = getattr(dataset, 'edge_type_dict', None)
        if type_of is None:      # a dataset without the dict gets the types the reference's dataset builds (datasets/movielens.py:329)
            type_of = {name: k for k, name in enumerate(dataset.edge_index_nps.keys())}
        num_edge_types = getattr(dataset, 'num_edge_types', None)
        if num_edge_types is None:
            num_edge_types = len(type_of)
        self.x = Parameter(torch.Tensor(dataset['num_nodes'], kwargs['emb_dim']))
        self.r = Parameter(torch.Tensor(num_edge_types, kwargs['emb_dim']))
        self.rating_r_idx = int(type_of['user2item'])
        self.acc_uids = int(dataset.type_accs['uid'])
        self.num_uids = int(dataset.num_uids)
        self.native = bool(kwargs.get('native', True))
        self.cached_repr = None

    def reset_parameters(self):
        glorot(self.x)
        glorot(self.r)

    def _apply(self, fn, *args, **kwargs):
        """nn.Module.to() / .cuda() move parameters only; the eval-mode table follows them"""
        out = super()._apply(fn, *args, **kwargs)
        if isinstance(self.cached_repr, torch.Tensor):
            self.cached_repr = fn(self.cached_repr)
        return out

    def shard(self, rank, world, tile=256):
        raise NotImplementedError('CFKG is single-GPU: sharding across ranks is not implemented')

    # ------------------------------------------------------------------ the reference's composition
    def forward(self, unids, inids):
        u_repr = self.x[unids]
        i_repr = self.x[inids]
        r_repr = self.r[torch.ones((unids.shape[0]), dtype=torch.long, device=self.r.device) * self.rating_r_idx]
        pred = torch.sum((u_repr + r_repr) * i_repr, dim=-1)
        return torch.exp(pred)

    def _kg_loss_torch(self, batch):
        h = self.x[batch[:, 0]]
        pos_t = self.x[batch[:, 1]]
        neg_t = self.x[batch[:, 2]]
        r = self.r[batch[:, 3]]
        pos_sim = torch.sum((h + r) * pos_t, dim=-1)
        neg_sim = torch.sum((h + r) * neg_t, dim=-1)
        return -(pos_sim.sigmoid().log().sum() + (-neg_sim).sigmoid().log().sum())

    # ------------------------------------------------------------------ the HIP route
    def _native_ok(self, batch):
        return (self.native and self.x.is_cuda and self.x.dtype == torch.float32 and batch.dtype == torch.int64 and
                batch.dim() == 2 and batch.shape[1] >= 4 and
                _engine.cfkg_supported(self.x.shape[1], self.r.shape[0], batch.shape[0]))

    def kg_loss(self, batch):
        """The KG-phase loss of rows (h, t+, t-, rel), in training and in eval mode alike"""
        if self._native_ok(batch):
            return _engine.cfkg_loss(self.x, self.r, batch)
        return self._kg_loss_torch(batch)

    def predict(self, unids, inids):
        # training mode is where gradients are needed: the composition.  Eval mode scores the table eval() built (no grad)
        if self.training or self.cached_repr is None or not self.cached_repr.is_cuda:
            return self.forward(unids, inids)
        return torch.exp(self.scored('predict', unids, inids))

    def loss(self, pos_neg_pair_t):
        """The reference's MFRecsysModel.loss (models/base.py:111-123): BCEWithLogitsLoss on predict.  The CFKG driver never
        calls it in its loop."""
        if self.training:
            pred = self.predict(pos_neg_pair_t[:, 0], pos_neg_pair_t[:, 1])
            label = pos_neg_pair_t[:, -1].float()
        else:
            pred, label = evaluators.eval_pairs(self.predict, pos_neg_pair_t)
        return F.binary_cross_entropy_with_logits(pred, label)

    def eval(self):
        self.train(False)
        _engine.check_pending_errors()       # a bad KG batch of the epoch raises here at the latest (IndexError)
        with torch.no_grad():
            table = self.x.detach().clone()
            table[self.acc_uids:self.acc_uids + self.num_uids] += self.r[self.rating_r_idx]
            self.cached_repr = table
        return self

    def rank_eval(self, unids, cand):
        """engine.dot_rank_eval's contract on the eval-mode table (cand [U, C], column 0 the held-out positive): rank of the
        positive and auc from the kernel's log-scores, exp(scores) as the predictions, and the per-user eval loss recomputed
        from them in the BCE form of the reference's eval mode (models/base.py:117-122).  What solvers.metrics calls."""
        if self.training or self.cached_repr is None:
            raise RuntimeError('rank_eval() reads the eval-mode table: call model.eval() first')
        if self.cached_repr.is_cuda:
            scores, rank, auc, _ = self.scored('rank_eval', unids, cand)
        else:
            t = self.cached_repr
            scores = torch.sum(t[unids.long()].unsqueeze(1) * t[cand.long()], dim=-1)
            rank, auc = evaluators.candidate_ranks(scores)
        pred = torch.exp(scores)
        return pred, rank, auc, evaluators.leave_one_out_loss(pred, 'bce')

    def recommend(self, unids, k, item_range, exclude=None):
        """GraphRecsysModel.recommend with exp of the kernel's scores: the predictions; the order is unchanged"""
        items, scores = super().recommend(unids, k, item_range, exclude=exclude)
        return items, torch.exp(scores)
