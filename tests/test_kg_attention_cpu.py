"""CPU: the KG input restated from the reference's KGAT / KGCN solvers, the C ABI of the edge softmax / KG attention
kernels, and the loud failure of their Python surface without a device."""
import numpy as np
import pytest
import torch

from test_cabi import declared_symbols

NEW_SYMBOLS = ('pea_edge_softmax_workspace_bytes', 'pea_edge_softmax', 'pea_edge_softmax_backward', 'pea_kg_edge_types',
               'pea_kg_attention_workspace_bytes', 'pea_kg_attention')


def test_kg_graph_input_matches_update_graph_input():
    """experiments/kgat_solver_bpr.py:126-140: relations in edge_index_nps order, types by enumeration of its keys,
    hstack, then the flipped copy with negated types; int64 [2, E] and [E, 1]."""
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, kg_graph_input
    d = SyntheticHIN('ml_small')
    ei, ea = kg_graph_input(d, 'cpu')
    names = list(d.edge_index_nps)
    total = sum(d.edge_index_nps[n].shape[1] for n in names)
    assert ei.dtype == torch.int64 and ea.dtype == torch.int64
    assert tuple(ei.shape) == (2, 2 * total) and tuple(ea.shape) == (2 * total, 1)
    off = 0
    for k, n in enumerate(names):
        rel = d.edge_index_nps[n].astype(np.int64)
        e = rel.shape[1]
        assert np.array_equal(ei[:, off:off + e].numpy(), rel), n
        assert bool((ea[off:off + e, 0] == k).all()), n
        assert np.array_equal(ei[:, total + off:total + off + e].numpy(), rel[::-1]), n
        assert bool((ea[total + off:total + off + e, 0] == -k).all()), n
        off += e
    assert names[0] == 'user2item' and bool((ea[total:total + d.edge_index_nps['user2item'].shape[1], 0] == 0).all())


def test_kg_graph_input_uses_the_dataset_edge_type_dict():
    from graph_recsys_benchmark_amd.utils import SyntheticHIN, kg_graph_input
    d = SyntheticHIN('ml_small')
    d.edge_type_dict = {n: k + 3 for k, n in enumerate(reversed(list(d.edge_index_nps)))}
    ei, ea = kg_graph_input(d, 'cpu')
    first = list(d.edge_index_nps)[0]
    e0 = d.edge_index_nps[first].shape[1]
    assert bool((ea[:e0, 0] == d.edge_type_dict[first]).all())
    assert bool((ea[ei.shape[1] // 2:ei.shape[1] // 2 + e0, 0] == -d.edge_type_dict[first]).all())


def test_header_and_library_carry_the_kg_attention_surface():
    from graph_recsys_benchmark_amd import _lib
    syms = declared_symbols()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    text = open(_lib.os.path.join(_lib._HERE, '..', 'include', 'peahip.h')).read()
    assert '#define PEA_KG_KGAT 0' in text and '#define PEA_KG_KGCN 1' in text
    assert (_lib.KG_KGAT, _lib.KG_KGCN) == (0, 1)


def test_kg_attention_without_a_device_fails_loudly():
    from graph_recsys_benchmark_amd import _lib
    from graph_recsys_benchmark_amd.nn import kgat_attention_map, kgcn_attention_map, softmax
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    x, r, p = torch.zeros(4, 8), torch.zeros(2, 8), torch.zeros(8, 8)
    ei = torch.tensor([[0, 1], [1, 2]])
    ea = torch.tensor([[0], [-1]])
    with pytest.raises(_lib.PeaError):
        softmax(torch.zeros(3), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.PeaError):
        kgat_attention_map(x, p, r, ei, ea, 4)
    with pytest.raises(_lib.PeaError):
        kgcn_attention_map(x, r, ei, ea, 4)
