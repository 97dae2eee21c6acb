"""GPU: the training kernels on the tile toolkit of csrc/tile16.h (transr_train.hip, herec.hip, kg_update.hip) on every tile
class their dispatchers can form, with the input makers, references and checks of their own suites (test_gpu_transr.py,
test_gpu_herec.py, test_gpu_kg_update.py: imported, not copied).

A kernel picks its instantiation and its loop bounds from the widths alone: NT = tiles_per_wave(IT * n_ut) accumulator tiles per
wave, HeRec's MT tables, the `id >= IT * n_ut` skip where the tile count is no multiple of 4, zero pad columns where the width
is no multiple of 16, the `c + 4 < D` tail of the eight-chain dot where it is no multiple of 8, and for kg_update with two
weights the cut of the backward into output-column chunks.  The suites run the widths the models use; the shapes here
(helpers.TRANSR_TILE_WIDTHS, HEREC_TILE_SHAPES, KG_TILE_WIDTHS) fill in the rest, and tests/test_train_tiles_cpu.py asserts
without a GPU that both together leave no class out.  Every id names the class the cell is there for, written down by hand in
tests/helpers.py, and every test first asserts that the restated dispatch arithmetic gives that class.

Batches: 17 is two tiles, the second with one row; 4097 is 257 tiles on the 256 workgroups of transr_train.hip / herec.hip, so
workgroup 0 takes a second tile that holds one row.  kg_update: 17 and 300 rows, and 8200 rows (513 tiles on 512 workgroups) at
two chunked widths, where the per-chunk accumulators live across a workgroup's tiles.  The large catalogue of the HeRec table
(9007 users, 8200 items: 282 + 257 tiles of 32 rows on 512 workgroups) makes workgroups 0..26 take a second tile, each time an
items' tile after a users' tile; the users' last tile holds 15 rows, the items' 8.

Tolerances are the rules of the three suites and nothing else: helpers.assert_fp32_close against the fp32 torch peer and the
float64 truth, 1e-5 |truth| + 1e-6 on the TransR loss, torch.equal in the exact cases (tests/test_train_tiles_cpu.py shows
float32 = float64 for those recipes at these widths)."""
import pytest
import torch

import helpers as H
import herec_ref
import test_gpu_herec as HR
import test_gpu_kg_update as KG
import test_gpu_transr as TR
from graph_recsys_benchmark_amd import engine
from graph_recsys_benchmark_amd.nn import kg_update_supported

pytestmark = pytest.mark.gpu

DEV = 'cuda'

TRANSR_CELLS = [(e, nt, it, b) for e, nt, it in H.TRANSR_TILE_WIDTHS for b in H.TILE_BATCHES]
TRANSR_IDS = ['E%d-NT%d-IT%d-B%d' % c for c in TRANSR_CELLS]
HEREC_CELLS = [(d, m, nt, it, b) for d, m, nt, it in H.HEREC_TILE_SHAPES for b in H.TILE_BATCHES]
HEREC_IDS = ['D%d-M%d-NT%d-IT%d-B%d' % c for c in HEREC_CELLS]
HEREC_SHAPE_IDS = ['D%d-M%d-NT%d-IT%d' % c for c in H.HEREC_TILE_SHAPES]
KG_CASES = H.kg_tile_cases()
KG_IDS = [H.kg_tile_id(*c) for c in KG_CASES]
KG_EXACT_CELLS = ([c + (n,) for c in KG_CASES for n in (17, 300)] +
                  [c + (H.KG_BIG_ROWS,) for c in KG_CASES if (c[1], c[2]) in H.KG_BIG_WIDTHS])
KG_EXACT_IDS = ['%s-n%d' % (H.kg_tile_id(*c[:5]), c[5]) for c in KG_EXACT_CELLS]
KG_CHUNKED = [c for c in KG_CASES if len(c[4]) > 1]


# ------------------------------------------------------------------------------------------------ transr_train.hip
def transr_class(e, nt, it, b):
    assert H.transr_tile_class(e) == (nt, it)
    assert engine.transr_supported(e, b)


@pytest.mark.parametrize('e,nt,it,b', TRANSR_CELLS, ids=TRANSR_IDS)
def test_transr_exact_integer_case(e, nt, it, b):
    transr_class(e, nt, it, b)
    TR.check_exact(e, b)


@pytest.mark.parametrize('e,nt,it,b', TRANSR_CELLS, ids=TRANSR_IDS)
def test_transr_loss_and_gradients(e, nt, it, b):
    transr_class(e, nt, it, b)
    TR.check_case(TR.case(e, b), 'E=%d B=%d' % (e, b))


@pytest.mark.parametrize('e,nt,it,b', TRANSR_CELLS, ids=TRANSR_IDS)
def test_transr_raw_gradient_rows(e, nt, it, b):
    transr_class(e, nt, it, b)
    TR.check_raw_rows(e, b)


@pytest.mark.parametrize('e,nt,it,b', TRANSR_CELLS, ids=TRANSR_IDS)
def test_transr_forward_only_gives_the_same_loss(e, nt, it, b):
    transr_class(e, nt, it, b)
    TR.check_forward_only(e, b)


# ------------------------------------------------------------------------------------------------ herec.hip: the training step
def herec_class(d, m, nt, it, b=0):
    assert H.herec_tile_class(d, m) == (nt, m, it)
    assert engine.herec_supported(d, m, b)


@pytest.mark.parametrize('d,m,nt,it,b', HEREC_CELLS, ids=HEREC_IDS)
def test_herec_exact_case(d, m, nt, it, b):
    herec_class(d, m, nt, it, b)
    HR.check_exact(d, m, b)


@pytest.mark.parametrize('d,m,nt,it,b', HEREC_CELLS, ids=HEREC_IDS)
def test_herec_loss_and_gradients(d, m, nt, it, b):
    herec_class(d, m, nt, it, b)
    HR.check_loss_and_gradients(d, m, b)


# ------------------------------------------------------------------------------------------------ herec.hip: the catalogue table
@pytest.mark.parametrize('d,m,nt,it', H.HEREC_TILE_SHAPES, ids=HEREC_SHAPE_IDS)
def test_herec_table(d, m, nt, it):
    herec_class(d, m, nt, it)
    inp = herec_ref.make_inputs(d, m, 17)
    HR.check_table(inp, HR.on_gpu(inp))


def test_herec_table_second_tile_crosses_from_users_to_items():
    c = H.HEREC_BIG_TABLE
    d, m = c['d'], c['m']
    inp = herec_ref.make_inputs(d, m, c['b'], n_user=c['n_user'], n_item=c['n_item'], n_other=c['n_other'], lead=c['lead'], gap=c['gap'])
    u_tiles, i_tiles = -(-c['n_user'] // 32), -(-c['n_item'] // 32)
    assert u_tiles + i_tiles > 512 and u_tiles + i_tiles - 512 <= u_tiles <= 512      # every second tile is an items' tile
    g = HR.on_gpu(inp)
    table = HR.check_table(inp, g)      # the whole table against table_of; rows of other nodes and columns D + 2, D + 3 exactly zero
    u0, i0, n = inp['acc_uids'], inp['acc_iids'], inp['num_nodes']
    assert (u0, i0 - (u0 + c['n_user']), n - (i0 + c['n_item'])) == (c['lead'], c['gap'], c['n_other'])
    for lo, hi in ((0, u0), (u0 + c['n_user'], i0), (i0 + c['n_item'], n)):           # lead, gap, tail
        assert hi > lo and not table[lo:hi].any()
    # the tables as column blocks of one wider buffer (row stride M D + 4 (M - 1)): the same bytes
    wide = torch.zeros((n, m * d + 4 * (m - 1)), device=DEV)
    views = [wide[:, k * (d + 4):k * (d + 4) + d] for k in range(m)]
    for v, t in zip(views, g['tables']):
        v.copy_(t)
    assert all(v.stride(0) == wide.shape[1] for v in views)
    again = engine.herec_table(views, g['w'], g['b'], g['user_emb'], g['item_emb'], g['user_rk_bias'], g['item_rk_bias'], u0, i0)
    assert torch.equal(table, again)


# ------------------------------------------------------------------------------------------------ kg_update.hip
def kg_class(kind, fin, fout, nt, chunks):
    cfg = H.kg_update_cfg(kind, fin, fout, True)
    assert (cfg['NT'], cfg['chunks'], cfg['weights']) == (nt, chunks, 1 if kind == 'kgcn' else 2)
    assert kg_update_supported(kind, fin, fout)


@pytest.mark.parametrize('kind,fin,fout,nt,chunks,n', KG_EXACT_CELLS, ids=KG_EXACT_IDS)
def test_kg_update_exact(kind, fin, fout, nt, chunks, n):
    kg_class(kind, fin, fout, nt, chunks)
    KG.check_exact(kind, n, fin, fout)


@pytest.mark.parametrize('kind,fin,fout,nt,chunks', KG_CASES, ids=KG_IDS)
def test_kg_update_random_float(kind, fin, fout, nt, chunks):
    kg_class(kind, fin, fout, nt, chunks)
    KG.check_random_float(kind, 300, fin, fout)


@pytest.mark.parametrize('kind,fin,fout,nt,chunks', KG_CHUNKED, ids=[H.kg_tile_id(*c) for c in KG_CHUNKED])
def test_kg_update_chunked_backward_keeps_to_its_column_block(kind, fin, fout, nt, chunks):
    """a later chunk reads and rewrites the dx / ds rows the earlier ones left (c0 > 0): with row strides wider than the block, a
    stride mistake there lands on the sentinel columns"""
    kg_class(kind, fin, fout, nt, chunks)
    assert len(chunks) > 1
    KG.check_column_blocks(kind, KG.make(kind, 65, fin, fout, seed=2, exact=True))
