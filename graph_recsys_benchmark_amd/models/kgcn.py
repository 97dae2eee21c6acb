"""KGCNRecsysModel: mirror of graph_recsys_benchmark/models/kgcn.py (kwargs dataset, emb_dim, hidden_size, dropout;
parameters x, r, proj_mat, conv1..3.{weight, bias}), see kg_base.py."""
import torch

from ..nn import KGCNConv
from ..nn.kg_attention import kgcn_attention_map
from .kg_base import KGBaseRecsysModel


class KGCNRecsysModel(KGBaseRecsysModel):
    conv_class = KGCNConv

    def attention_map(self):
        """The att_map of the model's current x and r over its own graph (experiments/kgcn_solver_bpr.py:311-319), one
        launch, detached."""
        with torch.no_grad():
            return kgcn_attention_map(self.x, self.r, self.edge_index, self.edge_attr, self.x.shape[0])
