"""The frozen-table MLP recommender on top of a walk embedding (reference graph_recsys_benchmark/models/walk.py, with the BPR
loss the driver adds at experiments/metapath2vec_solver_bpr.py:108-114).  cached_repr is the embedding table, a plain tensor;
only fc1 / fc2 train, so the training step is plain autograd over the gathered rows.  Scoring in eval mode, the evaluator
(solvers.metrics / metrics_full / metrics_full_multi, through rank_eval / rank_full / rank_full_multi below) and recommend()
run on the HIP scorer kernels (csrc/fuse_score.hip, csrc/topk.hip) whenever embedding_dim is a multiple of 4 and at most 64;
other widths stay on torch: the compositions of evaluators.py over _score_matrix."""
import torch
import torch.nn.functional as F

from .. import evaluators
from ..nn.inits import glorot
from .base import GraphRecsysModel


class WalkBasedRecsysModel(GraphRecsysModel):
    USER_CHUNK = 64           # users per block of the torch fallbacks: _score_matrix gathers [64 * items, 2 D] floats
    POS_CHUNK = 1024          # positives compared at once in the torch fallback of rank_full_multi

    def _init(self, **kwargs):
        emb = kwargs['embedding']
        self.cached_repr = emb.detach() if isinstance(emb, torch.Tensor) else emb      # a plain tensor, never a parameter
        self.embedding_dim = kwargs['embedding_dim']

        self.fc1 = torch.nn.Linear(2 * kwargs['embedding_dim'], kwargs['embedding_dim'])
        self.fc2 = torch.nn.Linear(kwargs['embedding_dim'], 1)

    def eval(self):
        return self.train(False)

    def reset_parameters(self):
        glorot(self.fc1.weight)
        glorot(self.fc2.weight)

    def _apply(self, fn, *args, **kwargs):
        """nn.Module.to() / .cuda() move parameters and buffers only; the table follows them"""
        out = super()._apply(fn, *args, **kwargs)
        if isinstance(self.cached_repr, torch.Tensor):
            self.cached_repr = fn(self.cached_repr)
        return out

    def _hip_scorer(self):
        return (self.cached_repr.is_cuda and self.fc1.weight.is_cuda and self.embedding_dim % 4 == 0 and
                self.embedding_dim <= 64)

    def forward(self, unids, inids):
        u_repr = self.cached_repr[unids]
        i_repr = self.cached_repr[inids]
        x = torch.cat([u_repr, i_repr], dim=-1)
        x = F.relu(self.fc1(x))
        x = self.fc2(x)
        return x

    def predict(self, unids, inids):
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if self.training or grad or not self._hip_scorer():
            return self.forward(unids, inids)
        return self.scored('predict', unids, inids)

    def loss(self, batch):
        pos_pred = self.predict(batch[:, 0], batch[:, 1])
        neg_pred = self.predict(batch[:, 0], batch[:, 2])
        cf_loss = -(pos_pred - neg_pred).sigmoid().log().sum()

        return cf_loss

    def _score_matrix(self, unids, items):
        """[U, len(items)] scores of every user against the same items, or against a row of items each ([U, C]), in torch"""
        u = unids.numel()
        items = items.expand(u, -1) if items.dim() == 2 else items.unsqueeze(0).expand(u, -1)
        c = items.shape[1]
        return self.forward(unids.repeat_interleave(c), items.reshape(-1)).view(u, c)

    def _require_eval(self, what):
        if self.training:
            raise RuntimeError('%s reads the eval-mode table: call model.eval() first' % what)

    def _callbacks(self, unids, item_range):
        """what evaluators' compositions ask of this model: (block, pairs) over the requested users and the catalogue"""
        items = torch.arange(item_range[0], item_range[1], device=unids.device)
        return (lambda r0, r1: self._score_matrix(unids[r0:r1], items),
                lambda rows, pos_items: self.forward(unids[rows], pos_items).view(-1))

    def rank_eval(self, unids, cand):
        """engine.rank_eval's contract for this model (cand [U, C], column 0 the held-out positive): (scores [U, C], rank of the
        positive int32 [U] = negatives scoring strictly higher, auc [U] = share of the negatives scoring strictly lower, eval loss
        [U] = -sum log sigmoid(pos - neg)).  What solvers.metrics calls; a width the HIP scorer does not take is ranked in torch."""
        self._require_eval('rank_eval()')
        if self._hip_scorer():
            return self.scored('rank_eval', unids, cand)
        with torch.no_grad():
            scores = self._score_matrix(unids.to(torch.int64), cand.to(torch.int64))
            rank, auc = evaluators.candidate_ranks(scores)
            loss = -F.logsigmoid(scores[:, :1] - scores[:, 1:]).sum(dim=1)
            return scores, rank, auc, loss

    def rank_full(self, unids, pos_items, item_range, exclude=None):
        """engine.rank_full's contract for this model: per user the rank of the held-out positive among the catalogue items that are
        neither excluded nor the positive itself (those scoring strictly higher), the share of them scoring strictly lower, and the
        positive's score.  What solvers.metrics_full calls; a width the HIP scorer does not take is ranked in torch
        (evaluators.rank_full, USER_CHUNK users at a time)."""
        self._require_eval('rank_full()')
        if self._hip_scorer():
            return self.scored('rank_full', unids, pos_items, item_range, exclude=exclude)
        with torch.no_grad():
            unids, pos_items = unids.to(torch.int64), pos_items.to(torch.int64)
            return evaluators.rank_full(*self._callbacks(unids, item_range), pos_items, item_range, exclude, self.USER_CHUNK)

    def recommend(self, unids, k, item_range, exclude=None):
        """GraphRecsysModel.recommend; a width the HIP scorer does not take is ranked in torch (evaluators.recommend), in the same
        order (score descending, node id ascending) and with the same (-1, -inf) tail."""
        self._require_eval('recommend()')
        if self._hip_scorer():
            return super().recommend(unids, k, item_range, exclude=exclude)
        with torch.no_grad():
            unids = torch.as_tensor(unids, device=self.cached_repr.device).to(torch.int64)
            block, _ = self._callbacks(unids, item_range)
            return evaluators.recommend(block, unids.numel(), k, item_range, exclude, self.USER_CHUNK, device=unids.device)

    def rank_full_multi(self, unids, pos_rowptr, pos_items, item_range, exclude=None):
        """engine.rank_full_multi's contract for this model: users with any number of held-out positives (a CSR), one catalogue
        scan.  What solvers.metrics_full_multi calls; a width the HIP scorer does not take is ranked in torch
        (evaluators.rank_full_multi)."""
        self._require_eval('rank_full_multi()')
        if self._hip_scorer():
            return self.scored('rank_full_multi', unids, pos_rowptr, pos_items, item_range, exclude=exclude)
        with torch.no_grad():
            unids, pos_rowptr, pos_items = (t.to(torch.int64) for t in (unids, pos_rowptr, pos_items))
            return evaluators.rank_full_multi(*self._callbacks(unids, item_range), pos_rowptr, pos_items, item_range, exclude,
                                              self.USER_CHUNK, self.POS_CHUNK)
