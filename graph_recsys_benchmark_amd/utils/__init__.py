from .graph_input import kg_graph_input, metapath_table, update_pea_graph_input
from .interactions import positives_csr, seen_items_csr
from .sampling import (EntityStore, KGTripleStore, cf_negative_sampling, device_cf_negative_sampling, device_kg_negative_sampling,
                       device_negative_sampling, device_shuffle_rows, entity_aware_row, entity_store, generate_candidates,
                       kg_negative_sampling, kg_triple_store)
from .synthetic import PRESETS, SyntheticHIN

__all__ = ['kg_graph_input', 'metapath_table', 'update_pea_graph_input', 'PRESETS', 'SyntheticHIN', 'cf_negative_sampling',
           'device_negative_sampling', 'entity_aware_row', 'generate_candidates', 'kg_negative_sampling', 'positives_csr',
           'seen_items_csr', 'KGTripleStore', 'kg_triple_store', 'device_kg_negative_sampling', 'device_shuffle_rows',
           'EntityStore', 'entity_store', 'device_cf_negative_sampling']
