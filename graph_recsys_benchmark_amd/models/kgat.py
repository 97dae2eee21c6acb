"""KGATRecsysModel: mirror of graph_recsys_benchmark/models/kgat.py (kwargs dataset, emb_dim, hidden_size, dropout;
parameters x, r, proj_mat, conv1..3.{weight_add, weight_bi, bias}), see kg_base.py."""
import torch

from ..nn import KGATConv
from ..nn.kg_attention import kgat_attention_map
from .kg_base import KGBaseRecsysModel


class KGATRecsysModel(KGBaseRecsysModel):
    conv_class = KGATConv

    def attention_map(self):
        """The att_map of the model's current x, proj_mat and r over its own graph (experiments/kgat_solver_bpr.py:311-320),
        one launch, detached."""
        with torch.no_grad():
            return kgat_attention_map(self.x, self.proj_mat, self.r, self.edge_index, self.edge_attr, self.x.shape[0])
