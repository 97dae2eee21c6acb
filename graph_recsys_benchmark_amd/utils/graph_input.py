"""update_pea_graph_input: the P x S list of int64 COO [2, E] device tensors per dataset.

Mirror of graph_recsys_benchmark/utils/general_utils.py:280-395 (same signature, same metapath tables, same
torch.flip idiom so reversed relations are fresh equal-content copies, same NotImplementedError for unknown
datasets).  `train_args['num_metapaths']` (optional) keeps only the first n metapaths -- BASELINE.json's
"MovieLens-25m, 9 metapaths" is the first nine of the reference's thirteen.  A 'Synthetic' dataset branch
carries the stress preset of SURVEY.md 8(d).

kg_graph_input restates the KG input of the reference's KGAT / KGCN solvers (experiments/kgat_solver_bpr.py:126-140).
"""
import numpy as np
import torch

# (relation, flipped) per step; tables transcribed from the reference's metapath definitions
_ML_SMALL = [
    [('user2item', 0), ('user2item', 1)], [('user2item', 1), ('user2item', 0)],
    [('year2item', 0), ('user2item', 1)], [('actor2item', 0), ('user2item', 1)],
    [('writer2item', 0), ('user2item', 1)], [('director2item', 0), ('user2item', 1)],
    [('genre2item', 0), ('user2item', 1)], [('tag2item', 0), ('user2item', 1)],
    [('tag2user', 0), ('user2item', 0)],
]
_ML_25M = [
    [('user2item', 0), ('user2item', 1)], [('year2item', 0), ('user2item', 1)],
    [('actor2item', 0), ('user2item', 1)], [('writer2item', 0), ('user2item', 1)],
    [('director2item', 0), ('user2item', 1)], [('genre2item', 0), ('user2item', 1)],
    [('genome_tag2item', 0), ('user2item', 1)], [('tag2user', 1), ('tag2user', 0)],
    [('tag2item', 1), ('tag2user', 0)], [('user2item', 1), ('user2item', 0)],
    [('tag2user', 0), ('user2item', 0)], [('tag2item', 1), ('tag2item', 0)],
    [('tag2user', 1), ('tag2item', 0)],
]
_YELP = [
    [('user2item', 0), ('user2item', 1)], [('user2item', 1), ('user2item', 0)],
    [('stars2item', 0), ('user2item', 1)], [('reviewcount2item', 0), ('user2item', 1)],
    [('attributes2item', 0), ('user2item', 1)], [('categories2item', 0), ('user2item', 1)],
    [('checkincount2item', 0), ('user2item', 1)], [('reviewcount2user', 0), ('user2item', 0)],
    [('friendcount2user', 0), ('user2item', 0)], [('fans2user', 0), ('user2item', 0)],
    [('stars2user', 0), ('user2item', 0)],
]
_STRESS = ([[('user2item', 0), ('user2item', 1)], [('user2item', 1), ('user2item', 0)]] +
           [[('attr_%d2item' % k, 0), ('user2item', 1)] for k in range(8)] +
           [[('attr_02user', 0), ('user2item', 0)], [('attr_02user', 1), ('attr_02user', 0)]] +
           [[('attr_%d2item' % k, 1), ('attr_%d2item' % k, 0)] for k in range(4)])


def metapath_table(dataset_args):
    if dataset_args['dataset'] == 'Movielens':
        if dataset_args['name'] == 'latest-small':
            return _ML_SMALL
        if dataset_args['name'] == '25m':
            return _ML_25M
    elif dataset_args['dataset'] == 'Yelp':
        return _YELP
    elif dataset_args['dataset'] == 'Synthetic':
        return _STRESS
    raise NotImplementedError


def update_pea_graph_input(dataset_args, train_args, dataset):
    table = metapath_table(dataset_args)
    n = train_args.get('num_metapaths')
    if n is not None:
        table = table[:n]
    device = train_args['device']
    base = {}
    for steps in table:
        for rel, _ in steps:
            if rel not in base:
                base[rel] = torch.from_numpy(dataset.edge_index_nps[rel]).long().to(device)
    return [[torch.flip(base[rel], dims=[0]) if flipped else base[rel] for rel, flipped in steps]
            for steps in table]


def kg_graph_input(dataset, device):
    """(edge_index int64 [2, E], edge_attr int64 [E, 1]) of KGATSolver / KGCNSolver.update_graph_input
    (experiments/kgat_solver_bpr.py:126-140, the same method in kgcn_solver_bpr.py): the relations in the order of
    dataset.edge_index_nps, each edge typed edge_type_dict[name], hstacked, then the flipped copy with negated types.
    A dataset without edge_type_dict (SyntheticHIN) gets the types the reference's dataset builds: enumerate over the
    keys of edge_index_nps (datasets/movielens.py:329)."""
    type_of = getattr(dataset, 'edge_type_dict', None)
    if type_of is None:
        type_of = {name: k for k, name in enumerate(dataset.edge_index_nps.keys())}
    pairs = [(ei, np.ones((ei.shape[1], 1)) * type_of[name]) for name, ei in dataset.edge_index_nps.items()]
    edge_index_np = np.hstack([p[0] for p in pairs])
    r_np = np.vstack([p[1] for p in pairs])
    edge_index_np = np.hstack([edge_index_np, np.flip(edge_index_np, 0)])
    r_np = np.vstack([r_np, -r_np])
    return torch.from_numpy(edge_index_np).long().to(device), torch.from_numpy(r_np).long().to(device)
