"""HeRec (reference graph_recsys_benchmark/models/herec.py, with the MSE loss the driver adds at
experiments/herec_solver_bpr.py:108-121): the one reference model that consumes SEVERAL metapath2vec tables.

    S(n)       = sum_m sigmoid(emb_trans[m](E_m[n]))         E_m [N, D] frozen tables, plain tensors
    pred(u, i) = <user_emb[u'], item_emb[i']> + <S(u), user_rk_bias[u']> + <S(i), item_rk_bias[i']>
                 u' = u - acc_uids, i' = i - acc_iids

forward() is the reference's torch composition and runs anywhere.  On the GPU, with native=True (the default) and a shape
engine.herec_supported takes, a training step's loss() is one launch of csrc/herec.hip (engine.herec_mse_loss: forward, loss
and the whole backward) and eval() builds cached_repr [N, D + 4] with engine.herec_table: the plain dot product of a user
row and an item row of that table is pred(u, i), so predict in eval mode, rank_eval, rank_full, recommend and
solvers.metrics / metrics_full run on the inner-product kernels of csrc/dot_score.hip unchanged.  On the CPU, or for a
shape the kernels refuse, the same table is built in torch (and loss() stays the composition)."""
import torch
import torch.nn.functional as F

from .. import engine as _engine, evaluators
from ..nn.inits import glorot
from .base import GraphRecsysModel


class HeRecRecsysModel(GraphRecsysModel):
    scorer = 'dot'

    def _init(self, **kwargs):
        self.rk_embeddings = [e.detach() for e in kwargs['embeddings']]      # plain tensors, never parameters
        self.num_uids = kwargs['num_uids']
        self.num_iids = kwargs['num_iids']
        self.acc_uids = kwargs['acc_uids']
        self.acc_iids = kwargs['acc_iids']
        self.embedding_dim = kwargs['embedding_dim']
        self.native = bool(kwargs.get('native', True))
        self.cached_repr = None

        dim = kwargs['embedding_dim']
        self.emb_trans = torch.nn.ModuleList([torch.nn.Linear(dim, dim) for _ in range(len(self.rk_embeddings))])

        self.user_emb = torch.nn.Embedding(self.num_uids, dim)
        self.item_emb = torch.nn.Embedding(self.num_iids, dim)

        self.user_rk_bias = torch.nn.Embedding(self.num_uids, dim)
        self.item_rk_bias = torch.nn.Embedding(self.num_iids, dim)

    def reset_parameters(self):
        for _ in self.emb_trans:
            glorot(_.weight)
        glorot(self.user_emb.weight)
        glorot(self.item_emb.weight)
        glorot(self.user_rk_bias.weight)
        glorot(self.item_rk_bias.weight)

    def _apply(self, fn, *args, **kwargs):
        """nn.Module.to() / .cuda() move parameters and buffers only; the frozen tables follow them"""
        out = super()._apply(fn, *args, **kwargs)
        self.rk_embeddings = [fn(e) for e in self.rk_embeddings]
        if isinstance(self.cached_repr, torch.Tensor):
            self.cached_repr = fn(self.cached_repr)
        return out

    def shard(self, rank, world, tile=256):
        raise NotImplementedError('HeRec is single-GPU: sharding across ranks is not implemented')

    # ------------------------------------------------------------------ the reference's composition
    def _rk_sum(self, nids):
        rk = [torch.sigmoid(emb_tran(rk_embedding[nids])) for emb_tran, rk_embedding in zip(self.emb_trans, self.rk_embeddings)]
        return torch.sum(torch.stack(rk, dim=-1), dim=-1)

    def forward(self, unids, inids):
        pred = torch.sum(self.user_emb(unids - self.acc_uids) * self.item_emb(inids - self.acc_iids), dim=-1)
        pred = pred + torch.sum(self._rk_sum(unids) * self.user_rk_bias(unids - self.acc_uids), dim=-1)
        pred = pred + torch.sum(self._rk_sum(inids) * self.item_rk_bias(inids - self.acc_iids), dim=-1)
        return pred

    # ------------------------------------------------------------------ the HIP routes
    def _on_gpu(self):
        return self.user_emb.weight.is_cuda and all(e.is_cuda for e in self.rk_embeddings)

    def _native_ok(self, batch_size=0):
        return (self.native and self._on_gpu() and len(self.rk_embeddings) >= 1 and
                all(e.dtype == torch.float32 for e in self.rk_embeddings) and
                _engine.herec_supported(self.embedding_dim, len(self.rk_embeddings), batch_size))

    def _stacked(self):
        return (torch.stack([t.weight for t in self.emb_trans]), torch.stack([t.bias for t in self.emb_trans]))

    def predict(self, unids, inids):
        # training mode is where gradients are needed: the composition.  Eval mode scores the table eval() built (no grad)
        if self.training or self.cached_repr is None or not self.cached_repr.is_cuda:
            return self.forward(unids, inids)
        return self.scored('predict', unids, inids)

    def loss(self, batch):
        if self.training:
            unids, inids, labels = batch[:, 0], batch[:, 1], batch[:, -1].float()
            if self._native_ok(batch.shape[0]):
                w, b = self._stacked()
                return _engine.herec_mse_loss(self.rk_embeddings, w, b, self.user_emb.weight, self.item_emb.weight,
                                              self.user_rk_bias.weight, self.item_rk_bias.weight, self.acc_uids, self.acc_iids,
                                              unids.long(), inids.long(), labels)
            return F.mse_loss(self.forward(unids.long(), inids.long()), labels)
        return F.mse_loss(*evaluators.eval_pairs(self.predict, batch))

    def _table_torch(self):
        """cached_repr in torch: what engine.herec_table builds (include/peahip.h, pea_herec_table)"""
        dev, d = self.user_emb.weight.device, self.embedding_dim
        n = self.rk_embeddings[0].shape[0]
        out = torch.zeros((n, d + 4), dtype=torch.float32, device=dev)
        u = torch.arange(self.acc_uids, self.acc_uids + self.num_uids, device=dev)
        i = torch.arange(self.acc_iids, self.acc_iids + self.num_iids, device=dev)
        out[u, :d] = self.user_emb.weight
        out[u, d] = 1.0
        out[u, d + 1] = torch.sum(self._rk_sum(u) * self.user_rk_bias.weight, dim=-1)
        out[i, :d] = self.item_emb.weight
        out[i, d] = torch.sum(self._rk_sum(i) * self.item_rk_bias.weight, dim=-1)
        out[i, d + 1] = 1.0
        return out

    def eval(self):
        self.train(False)
        with torch.no_grad():
            if self._native_ok():
                _engine.check_pending_errors()       # a bad batch of the epoch raises here at the latest (IndexError)
                w, b = self._stacked()
                self.cached_repr = _engine.herec_table(self.rk_embeddings, w, b, self.user_emb.weight, self.item_emb.weight,
                                                       self.user_rk_bias.weight, self.item_rk_bias.weight, self.acc_uids,
                                                       self.acc_iids)
            else:
                self.cached_repr = self._table_torch()
        return self

    def rank_eval(self, unids, cand):
        """engine.dot_rank_eval's contract on the eval-mode table (cand [U, C], column 0 the held-out positive): scores, rank of
        the positive and auc from the kernel; the per-user eval loss is recomputed from the scores in the MSE form of the driver's eval
        mode (experiments/herec_solver_bpr.py:108-121; dot_rank_eval's own loss is the BPR one).  What solvers.metrics calls."""
        if self.training or self.cached_repr is None:
            raise RuntimeError('rank_eval() reads the eval-mode table: call model.eval() first')
        if self.cached_repr.is_cuda:
            scores, rank, auc, _ = self.scored('rank_eval', unids, cand)
        else:
            t = self.cached_repr
            scores = torch.sum(t[unids.long()].unsqueeze(1) * t[cand.long()], dim=-1)
            rank, auc = evaluators.candidate_ranks(scores)
        return scores, rank, auc, evaluators.leave_one_out_loss(scores, 'mse')
