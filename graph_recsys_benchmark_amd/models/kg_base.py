"""What the reference's three graph baselines share (graph_recsys_benchmark/models/kgat.py, kgcn.py, ngcf.py): three convs
of widths H, H/2, H/4 with dropout after each, the table = cat of their L2-normalised outputs ([N, H + H/2 + H/4]), and
the inner-product scorer predict = sum(repr[u] * repr[i]).

The convs are nn/kg_conv.py (sparse half in HIP, differentiable); everything that reads the finished table without
autograd -- predict, the evaluation loss, recommend, solvers.metrics / metrics_full -- goes to csrc/dot_score.hip.

native_train=True (constructor kwarg, default off) sends a training step's loss() through HIP end to end: per conv the
aggregate + the fused dense update of csrc/kg_update.hip (nn.kg_update), then the BPR loss of csrc/dot_train.hip on the
un-normalised conv outputs (engine.dot_bpr_loss).  The dropout masks are then drawn by torch.rand(...) >= p, which is NOT
the random stream of F.dropout: with dropout > 0 the two paths see different masks of the same distribution.  In this
mode no table is built while training: cached_repr is None and predict() raises until cf_eval() / eval() has run.  Widths
the kernels refuse, an att_map that requires grad and batches of more than 5461 triples take the autograd path silently.

native_kg=True (constructor kwarg of KGAT / KGCN, default off, independent of native_train) sends the KG phase through HIP
as well: kg_loss(batch) becomes one launch of csrc/transr_train.hip (engine.transr_loss: the three projections, the loss
and the whole backward), with the index backward into x and r on the existing deterministic scatter.  It works in training
and in eval mode.  kg_loss stays the torch composition on a CPU tensor, for a batch that is not int64 [B, >= 4], for an
emb_dim that is no multiple of 4 in 4..128 and for batches of more than 5461 rows.
"""
import torch
import torch.nn.functional as F
from torch.nn import Parameter

from .. import engine as _engine
from ..nn.inits import glorot
from .base import GraphRecsysModel


class DotRecsysModel(GraphRecsysModel):
    scorer = 'dot'
    # the loss of GraphRecsysModel reads these; the KG models have no entity-aware term, NGCF sets them from its kwargs
    entity_aware = False
    entity_aware_coff = 0.0

    native_train = False
    native_kg = False

    def _convs(self):
        return (self.conv1, self.conv2, self.conv3)

    def _native_ok(self, batch, *conv_args):
        """Whether this training step can take the HIP path (see the module docstring)."""
        if not (self.native_train and self.training and 0 <= self.dropout < 1):
            return False
        if any(torch.is_tensor(a) and a.requires_grad for a in conv_args):
            return False
        convs = self._convs()
        return (all(c.update_supported() for c in convs)
                and _engine.dot_bpr_supported([c.out_channels for c in convs], batch.shape[0]))

    def _native_loss(self, batch, *conv_args):
        """conv1..3 as aggregate -> kg_update with the dropout mask folded in, then the BPR loss on the raw outputs."""
        x, blocks = self.x, []
        for conv in self._convs():
            s = conv.aggregate(x, self.edge_index, *conv_args)
            keep, scale = None, 1.0
            if self.dropout > 0:
                keep = (torch.rand((x.shape[0], conv.out_channels), device=x.device) >= self.dropout).to(torch.uint8)
                scale = 1.0 / (1.0 - self.dropout)
            x = conv.update(x, s, keep, scale)
            blocks.append(x)
        self.cached_repr = None
        return _engine.dot_bpr_loss(blocks, batch)

    def _stack(self, *conv_args):
        """conv1..3 + dropout, then the concatenation of the normalised outputs (models/kgat.py:45-51)."""
        x_1 = F.dropout(self.conv1(self.x, self.edge_index, *conv_args), p=self.dropout, training=self.training)
        x_2 = F.dropout(self.conv2(x_1, self.edge_index, *conv_args), p=self.dropout, training=self.training)
        x_3 = F.dropout(self.conv3(x_2, self.edge_index, *conv_args), p=self.dropout, training=self.training)
        return torch.cat([F.normalize(x_1, dim=-1), F.normalize(x_2, dim=-1), F.normalize(x_3, dim=-1)], dim=-1)

    def predict(self, unids, inids):
        if getattr(self, 'cached_repr', None) is None:
            raise RuntimeError('native_train builds no table while training: call cf_eval() / eval() before predict()')
        if self.cached_repr.requires_grad:      # training: the reference's formula, differentiable
            return torch.sum(self.cached_repr[unids] * self.cached_repr[inids], dim=-1)
        return self.scored('predict', unids, inids)


class KGBaseRecsysModel(DotRecsysModel):
    """KGAT and KGCN: node embeddings x, relation embeddings r, a projection proj_mat, and convs that take the att_map the
    solver recomputes per epoch (experiments/kgat_solver_bpr.py:311-320)."""
    conv_class = None

    def _init(self, **kwargs):
        self.dropout = kwargs['dropout']
        self.native_train = bool(kwargs.get('native_train', False))
        self.native_kg = bool(kwargs.get('native_kg', False))
        emb, hidden = kwargs['emb_dim'], kwargs['hidden_size']
        self.x = Parameter(torch.Tensor(kwargs['dataset']['num_nodes'], emb))
        self.r = Parameter(torch.Tensor(kwargs['dataset'].num_edge_types, emb))
        self.proj_mat = Parameter(torch.Tensor(emb, emb))
        self.edge_index, self.edge_attr = self.update_graph_input(kwargs['dataset'])
        self.conv1 = self.conv_class(emb, hidden)
        self.conv2 = self.conv_class(hidden, hidden // 2)
        self.conv3 = self.conv_class(hidden // 2, hidden // 4)

    def reset_parameters(self):
        glorot(self.x)
        glorot(self.r)
        glorot(self.proj_mat)
        self.conv1.reset_parameters()
        self.conv2.reset_parameters()
        self.conv3.reset_parameters()

    def forward(self, att_map):
        return self._stack(att_map)

    def kg_eval(self):
        torch.nn.Module.eval(self)

    def cf_eval(self, att_map):
        torch.nn.Module.eval(self)
        self._repr_partial = False
        with torch.no_grad():
            self.cached_repr = self.forward(att_map)

    def attention_map(self):
        """att_map of the model's own tensors over its own graph, without grad (the concrete model picks the formula)."""
        raise NotImplementedError

    def loss(self, batch, att_map):
        """BPR loss as the reference's experiment subclass writes it (experiments/kgat_solver_bpr.py:101-108)."""
        if self._native_ok(batch, att_map):
            return self._native_loss(batch, att_map)
        if self.training:
            self.cached_repr = self.forward(att_map)
        pos_pred = self.predict(batch[:, 0], batch[:, 1])
        neg_pred = self.predict(batch[:, 0], batch[:, 2])
        return -(pos_pred - neg_pred).sigmoid().log().sum()

    def kg_loss(self, batch):
        """TransR-style loss over (head, tail+, tail-, relation) rows (experiments/kgat_solver_bpr.py:110-124): one HIP
        launch with native_kg=True (engine.transr_loss, csrc/transr_train.hip), else the torch composition below."""
        if (self.native_kg and self.x.is_cuda and batch.dtype == torch.int64 and batch.dim() == 2 and batch.shape[1] >= 4
                and _engine.transr_supported(self.x.shape[1], batch.shape[0])):
            return _engine.transr_loss(self.x, self.proj_mat, self.r, batch)
        head = torch.mm(self.x[batch[:, 0]], self.proj_mat) + self.r[batch[:, 3]]
        pos_diff = head - torch.mm(self.x[batch[:, 1]], self.proj_mat)
        neg_diff = head - torch.mm(self.x[batch[:, 2]], self.proj_mat)
        pos_pred = (pos_diff * pos_diff).sum(-1)
        neg_pred = (neg_diff * neg_diff).sum(-1)
        return -(pos_pred - neg_pred).sigmoid().log().sum()
