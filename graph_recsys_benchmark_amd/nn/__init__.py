from .conv import GATConv, GCNConv, SAGEConv
from .inits import glorot, zeros
from .kg_attention import kgat_attention_map, kgcn_attention_map, softmax
from .kg_conv import KGATConv, KGCNConv, NGCFConv, weighted_aggregate

__all__ = ['GATConv', 'GCNConv', 'SAGEConv', 'KGATConv', 'KGCNConv', 'NGCFConv', 'weighted_aggregate', 'softmax',
           'kgat_attention_map', 'kgcn_attention_map', 'glorot', 'zeros']
