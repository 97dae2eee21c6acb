from .conv import GATConv, GCNConv, SAGEConv
from .inits import glorot, zeros
from .kg_attention import kgat_attention_map, kgcn_attention_map, softmax
from .kg_conv import KGATConv, KGCNConv, NGCFConv, kg_update, kg_update_supported, weighted_aggregate

__all__ = ['GATConv', 'GCNConv', 'SAGEConv', 'KGATConv', 'KGCNConv', 'NGCFConv', 'weighted_aggregate', 'kg_update', 'kg_update_supported', 'softmax',
           'kgat_attention_map', 'kgcn_attention_map', 'glorot', 'zeros']
