"""NGCFRecsysModel: mirror of graph_recsys_benchmark/models/ngcf.py (kwargs dataset, emb_dim, hidden_size, dropout,
entity_aware, entity_aware_coff, if_use_features; parameters x, conv1..3.{W_1, W_2}), see kg_base.py.  loss() and eval()
are GraphRecsysModel's, which take the inner-product entry points because scorer = 'dot'; with native_train=True a training
step's loss() takes the HIP path of kg_base.py instead (the entity-aware term is added as before)."""
import torch
from torch.nn import Parameter

from .. import engine as _engine
from ..nn import NGCFConv
from ..nn.inits import glorot
from .kg_base import DotRecsysModel


class NGCFRecsysModel(DotRecsysModel):
    def _init(self, **kwargs):
        self.entity_aware = kwargs['entity_aware']
        self.entity_aware_coff = kwargs['entity_aware_coff']
        self.if_use_features = kwargs['if_use_features']
        self.dropout = kwargs['dropout']
        self.native_train = bool(kwargs.get('native_train', False))
        if self.if_use_features:
            raise NotImplementedError('Feature not implemented!')
        emb, hidden = kwargs['emb_dim'], kwargs['hidden_size']
        self.x = Parameter(torch.Tensor(kwargs['dataset']['num_nodes'], emb))
        self.edge_index = self.update_graph_input(kwargs['dataset'])
        self.conv1 = NGCFConv(emb, hidden)
        self.conv2 = NGCFConv(hidden, hidden // 2)
        self.conv3 = NGCFConv(hidden // 2, hidden // 4)

    def reset_parameters(self):
        glorot(self.x)
        self.conv1.reset_parameters()
        self.conv2.reset_parameters()
        self.conv3.reset_parameters()

    def forward(self):
        return self._stack()

    def loss(self, pos_neg_pair_t):
        if self._native_ok(pos_neg_pair_t):
            cf_loss = self._native_loss(pos_neg_pair_t)
            if self.entity_aware:
                return cf_loss + self.entity_aware_coff * _engine.entity_reg(self.x, pos_neg_pair_t)
            return cf_loss
        return super().loss(pos_neg_pair_t)
