"""NGCFRecsysModel: mirror of graph_recsys_benchmark/models/ngcf.py (kwargs dataset, emb_dim, hidden_size, dropout,
entity_aware, entity_aware_coff, if_use_features; parameters x, conv1..3.{W_1, W_2}), see kg_base.py.  loss() and eval()
are GraphRecsysModel's, which take the inner-product entry points because scorer = 'dot'."""
import torch
from torch.nn import Parameter

from ..nn import NGCFConv
from ..nn.inits import glorot
from .kg_base import DotRecsysModel


class NGCFRecsysModel(DotRecsysModel):
    def _init(self, **kwargs):
        self.entity_aware = kwargs['entity_aware']
        self.entity_aware_coff = kwargs['entity_aware_coff']
        self.if_use_features = kwargs['if_use_features']
        self.dropout = kwargs['dropout']
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
