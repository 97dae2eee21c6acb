"""CPU: what tests/test_gpu_train_tiles_matrix.py relies on, checked without a GPU.

1. The restatement of the training kernels' dispatch arithmetic (helpers.ceil16 ... helpers.kg_update_cfg, each citing the C
   lines it restates) against the library: where a tile class exists, pea_transr_supported / pea_herec_supported /
   pea_kg_update_supported say yes, and nowhere else.  For HeRec that pins tiles_per_wave, the LDS formula and the budget.
2. Coverage: every supported width is enumerated (32 for TransR, every (D, M) for HeRec, 32 x 32 x {one weight, two weights}
   for the kg_update backward) and the matrix's shape lists, together with the lists of the kernels' own suites (imported, so
   trimming either side fails here), must reach every class the dispatchers can form.
3. Exactness: the integer recipes of the exact cells give the same numbers in float32 and in float64 on the CPU, in every
   output and gradient, at the matrix's widths -- so a bitwise comparison on the GPU means something there."""
import pytest
import torch

import helpers as H
import herec_ref
import test_gpu_herec
import test_gpu_kg_update
import test_gpu_transr
from graph_recsys_benchmark_amd import _lib

WIDTHS = range(0, 141)
KIND_ID = {'kgat': _lib.KGU_KGAT, 'kgcn': _lib.KGU_KGCN, 'ngcf': _lib.KGU_NGCF}


# ------------------------------------------------------------------------------------------- 1. against the library
def test_tiles_per_wave_by_hand():
    assert [H.ceil16(v) for v in (0, 1, 16, 17, 124, 128)] == [0, 16, 16, 32, 128, 128]
    assert [H.tiles_per_wave(t) for t in (1, 4, 5, 8, 9, 16, 17, 25, 32, 33, 36, 49, 64)] == [1, 1, 2, 2, 4, 4, 8, 8, 8, 16, 16, 16, 16]


def test_transr_restatement_agrees_with_the_library():
    lib = _lib.load()
    for e in WIDTHS:
        assert (H.transr_tile_class(e) is not None) == bool(lib.pea_transr_supported(e)), e


def test_herec_restatement_agrees_with_the_library():
    lib = _lib.load()
    for d in WIDTHS:
        for m in range(0, 6):
            assert (H.herec_tile_class(d, m) is not None) == bool(lib.pea_herec_supported(d, m)), (d, m)
    # the three sizes csrc/herec.hip's header quotes, and the one it refuses for its size alone
    assert [H.herec_train_lds_bytes(d, m) for d, m in ((64, 4), (128, 1), (80, 2), (128, 2))] == [148416, 118720, 107968, 220096]
    assert H.herec_tile_class(128, 2) is None and H.herec_train_lds_bytes(128, 2) > H.TILE_LDS_BUDGET


def test_kg_update_restatement_agrees_with_the_library():
    lib = _lib.load()
    for kind, kid in KIND_ID.items():
        for fin in WIDTHS:
            for fout in WIDTHS:
                for bwd in (False, True):
                    cfg = H.kg_update_cfg(kind, fin, fout, bwd)
                    assert (cfg is not None) == bool(lib.pea_kg_update_supported(kid, fin, fout)), (kind, fin, fout)
                    if cfg is not None:         # what the launch needs: the image fits, the tiles fit the template
                        assert cfg['lds'] <= H.TILE_LDS_BUDGET and sum(cfg['chunks']) == fout and cfg['OC'] % 16 == 0
                        assert not bwd or cfg['NT'] <= (16 if kind == 'kgcn' else 8)
    assert H.kg_update_cfg('gat', 64, 64, True) is None


# ------------------------------------------------------------------------------------------- 2. coverage of the class space
def test_transr_lists_reach_every_tile_class():
    space = {H.transr_tile_class(e) for e in WIDTHS} - {None}
    assert sum(H.transr_tile_class(e) is not None for e in WIDTHS) == 32 and len(space) == 8
    for e, nt, it in H.TRANSR_TILE_WIDTHS:
        assert H.transr_tile_class(e) == (nt, it), e
    mine = [e for e, _, _ in H.TRANSR_TILE_WIDTHS]
    hit = {H.transr_tile_class(e) for e in mine + list(test_gpu_transr.WIDTHS)}
    assert hit == space, 'no width left for (NT, IT) in %s' % sorted(space - hit)
    assert {it for e in mine for _, it in [H.transr_tile_class(e)]} >= {3, 5, 6, 7}      # tile ids that are skipped
    assert any(e % 16 and e % 8 for e in mine) and any(e % 16 and e % 8 == 0 for e in mine)      # pad columns; the c + 4 < E tail


def test_herec_lists_reach_every_tile_class():
    every = [H.herec_tile_class(d, m) for d in WIDTHS for m in range(0, 6)]
    space = {(nt, mt) for nt, mt, _ in filter(None, every)}
    assert len(space) == 11 and {it for _, _, it in filter(None, every)} == set(range(1, 9))
    for d, m, nt, it in H.HEREC_TILE_SHAPES:
        assert H.herec_tile_class(d, m) == (nt, m, it), (d, m)
    mine = [(d, m) for d, m, _, _ in H.HEREC_TILE_SHAPES]
    classes = [H.herec_tile_class(d, m) for d, m in mine + list(test_gpu_herec.SHAPES)]
    assert None not in classes
    hit = {(nt, mt) for nt, mt, _ in classes}
    assert hit == space, 'no shape left for (NT, MT) in %s' % sorted(space - hit)
    assert {it for _, _, it in classes} == set(range(1, 9))
    assert {it for nt, mt, it in classes if (nt, mt) == (16, 1)} == {6, 7, 8}


def _kg_classes(widths):
    """{(weights, number of chunks, NT)}, the per-chunk tile counts and the chunk lists of the backward at these widths"""
    classes, counts, chunked = set(), set(), []
    for fin, fout in widths:
        for kind in ('kgcn', 'kgat', 'ngcf'):
            cfg = H.kg_update_cfg(kind, fin, fout, True)
            classes.add((cfg['weights'], len(cfg['chunks']), cfg['NT']))
            counts.update(H.kg_update_tile_counts(cfg))
            if len(cfg['chunks']) > 1:
                chunked.append(cfg['chunks'])
    return classes, counts, chunked


def test_kg_update_lists_reach_every_backward_class():
    supported = [(fin, fout) for fin in range(4, 129, 4) for fout in range(4, 129, 4)]
    assert len(supported) == 32 * 32
    space, _, _ = _kg_classes(supported)
    assert len(space) == 10
    for kind, fin, fout, nt, chunks in H.kg_tile_cases():
        cfg = H.kg_update_cfg(kind, fin, fout, True)
        assert (cfg['NT'], cfg['chunks']) == (nt, chunks), (kind, fin, fout)
    mine = [w for w, _ in H.KG_TILE_WIDTHS]
    hit, counts, chunked = _kg_classes(mine + list(test_gpu_kg_update.WIDTHS))
    assert hit == space, 'no width left for (weights, chunks, NT) in %s' % sorted(space - hit)
    assert any(c[-1] != c[0] and c[-1] % 16 for c in chunked), 'no chunked backward whose last chunk is narrower and no multiple of 16'
    assert counts >= {9, 18, 25, 35}, 'tile counts where the waves skip ids'
    assert {(1, 1, 8), (2, 1, 8)} <= _kg_classes(mine)[0]           # launch_bwd<8> without chunks, both weight counts
    for fin, fout in H.KG_BIG_WIDTHS:                               # the large cells are chunked and span a second tile per workgroup
        assert len(H.kg_update_cfg('kgat', fin, fout, True)['chunks']) == 2 and (H.KG_BIG_ROWS + 15) // 16 > 512


def test_herec_big_table_takes_a_second_tile_across_the_segments():
    c = H.HEREC_BIG_TABLE
    u_tiles, i_tiles = (c['n_user'] + 31) // 32, (c['n_item'] + 31) // 32
    assert (u_tiles, i_tiles) == (282, 257) and u_tiles + i_tiles > 512
    second = range(512, u_tiles + i_tiles)                  # tile T + 512 of workgroup T
    assert all(t - 512 < u_tiles <= t for t in second)      # first a users' tile, then an items'
    assert c['n_user'] % 32 == 15 and c['n_item'] % 32 == 8
    assert H.herec_tile_class(c['d'], c['m']) is not None


# ------------------------------------------------------------------------------------------- 3. exactness of the integer recipes
@pytest.mark.parametrize('b', H.TILE_BATCHES)
@pytest.mark.parametrize('e', [e for e, _, _ in H.TRANSR_TILE_WIDTHS])
def test_transr_integer_recipe_is_exact_in_float32(e, b):
    x, p, r, batch = test_gpu_transr.exact_inputs(e, b, device='cpu')
    pos32, neg32 = test_gpu_transr.exact_pos_neg(x, p, r, batch, torch.float32)
    pos64, neg64 = test_gpu_transr.exact_pos_neg(x, p, r, batch, torch.float64)
    assert e * (2 * e + 1) ** 2 < 2 ** 24 and float(pos64.max()) < 2 ** 24 and float(neg64.max()) < 2 ** 24
    assert torch.equal(pos32.double(), pos64) and torch.equal(neg32.double(), neg64)
    assert float(pos64.max()) > 0 and bool((pos64 != neg64).any())


@pytest.mark.parametrize('b', H.TILE_BATCHES)
@pytest.mark.parametrize('d,m', [(d, m) for d, m, _, _ in H.HEREC_TILE_SHAPES])
def test_herec_integer_recipe_is_exact_in_float32(d, m, b):
    inp, want = test_gpu_herec.exact_inputs(d, m, b)
    for dtype in (torch.float32, torch.float64):
        pred = herec_ref.pred_of(inp, {k: inp[k].to(dtype) for k in herec_ref.KEYS}, inp['unids'], inp['inids'])[0]
        assert torch.equal(pred.double(), want), dtype
    assert bool((want != 0).any()) and bool((want * 2 == (want * 2).round()).all())


KG_EXACT = ([(kind, n, fin, fout) for kind, fin, fout, _, _ in H.kg_tile_cases() for n in (17, 300)] +
            [(kind, H.KG_BIG_ROWS, fin, fout) for fin, fout in H.KG_BIG_WIDTHS for kind in H.KG_KINDS])


@pytest.mark.parametrize('kind,n,fin,fout', KG_EXACT)
def test_kg_update_integer_recipe_is_exact_in_float32(kind, n, fin, fout):
    t = test_gpu_kg_update.exact_inputs(kind, n, fin, fout, device='cpu')
    got, want = test_gpu_kg_update.torch_side(kind, t, torch.float32), test_gpu_kg_update.torch_side(kind, t, torch.float64)
    for name, a, b in zip(test_gpu_kg_update.NAMES, got, want):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a.double(), b), name
            assert float(b.abs().max()) < 2 ** 24, name
