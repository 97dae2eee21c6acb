"""CPU: the dispatch of the dense products (csrc/gemm.hip: plan_gemm_launches, what launch_gemm_batch executes) asked through
pea_dense_route, which needs no device and reads through no pointer: the jobs here carry made-up addresses, of which only the
alignment matters.  The expectations are the hand-written tables of tests/helpers.py that tests/test_gpu_dense_matrix.py runs on
the GPU, and sizes worked out in the comments from the kernels' LDS layouts:
  budget        160 KiB - 1 KiB = 162,816 B of dynamic LDS per workgroup
  persistent    a job's B image: (2 KH + 1) rows (k padded to the class + the bias row) x n_out rounded up to 32 columns x 4 B
  skinny        (16 KQ + 1) x 16 floats per job
  deep          resident: k x 32 NCT x 4 B; 128-chunk: 2 x 128 x 32 NCT x 4 B; fallback: static LDS only"""
import ctypes as C

import pytest

from helpers import DENSE_DEEP_CASES, DENSE_DEEP_IDS, DENSE_MIXED, DENSE_MIXED_DEEP, DENSE_MIXED_PLAN, DENSE_ROUTES, dense_route_rows

BUDGET = 160 * 1024 - 1024
SKINNY, PERSIST, RESIDENT, CHUNK, STAGED = range(5)      # include/peahip.h PEA_ROUTE_*


def _jobs(specs, off=4):
    """DenseJob array for (k, n_out, gated) specs: blocks of wide buffers at made-up, 256-byte aligned addresses; the output
    (and the gate) `off` floats into its row, so off = 2 gives an output that cannot take 16-byte stores"""
    from graph_recsys_benchmark_amd import _lib
    arr = (_lib.DenseJob * len(specs))()
    for q, (k, n_out, gated) in enumerate(specs):
        base = 0x10000000 * (q + 1)
        arr[q] = _lib.DenseJob(base, k + 16, k, base + 0x4000000, n_out + 12, n_out, base + 0x8000000 + 4 * off, n_out + 8,
                               base + 0xc000000 + 4 * off if gated else None, n_out + 8 if gated else 0)
    return arr


def _route(specs, n_rows, rows_given=False, off=4):
    from graph_recsys_benchmark_amd import _lib
    return _lib.dense_route(n_rows, rows_given, _jobs(specs, off))


def _image(kh, n_out):
    return (2 * kh + 1) * ((n_out + 31) // 32 * 32) * 4


@pytest.mark.parametrize('ks,cs,kernel,name,count,ns,off', DENSE_ROUTES, ids=[r[2] + '-k%d-c%d' % (r[0][0], r[1][0]) for r in DENSE_ROUTES])
@pytest.mark.parametrize('rows_given', [False, True])
def test_every_row_of_the_route_table(ks, cs, kernel, name, count, ns, off, rows_given):
    for k in ks:
        for c in cs:
            for n in ns:
                got = _route([(k, c, False)], n, rows_given, off)
                assert dense_route_rows(got) == [(name, kernel, [0])] * count, (k, c, n)
                assert all(e.listed == rows_given for e in got)
                assert [e.col0[0] for e in got] == [sum(e.n_out[0] for e in got[:i]) for i in range(count)]      # chunks tile the columns
                assert sum(e.n_out[0] for e in got) == c
                for e in got:
                    if e.family == SKINNY:
                        assert e.lds_bytes == (16 * e.variant + 1) * 16 * 4 and k <= 16 * e.variant
                    elif e.family == PERSIST:
                        assert e.lds_bytes == _image(e.variant, e.n_out[0]) <= BUDGET and k <= 2 * e.variant and e.col_group == 5
                    elif e.family == RESIDENT:
                        assert e.lds_bytes == k * 32 * e.variant * 4 <= BUDGET and c <= 32 * e.variant
                    elif e.family == CHUNK:
                        assert e.lds_bytes == 2 * 128 * 32 * e.variant * 4 and c <= 32 * e.variant
                    else:
                        assert e.lds_bytes == 0 and e.variant == 64


def test_no_rows_no_launches():
    specs = [(k, c, g) for k, c, g in DENSE_MIXED]
    assert _route(specs, 0) == [] and _route(specs, 0, rows_given=True) == []
    assert _route([], 100) == []


@pytest.mark.parametrize('n_jobs,k,n_out,kernel,names', [
    (12, 16, 64, 'persist<16>', ['gemm_mfma_batch']),
    (13, 16, 64, 'persist<16>', ['gemm_mfma_batch', 'gemm_mfma_shared']),
    (25, 16, 64, 'persist<16>', ['gemm_mfma_batch', 'gemm_mfma_batch', 'gemm_mfma_shared']),
    (13, 64, 16, 'skinny<4>', ['gemm_mfma_narrow', 'gemm_mfma_narrow']),
    (13, 132, 32, 'resident<1>', ['gemm_mfma_deep', 'gemm_mfma_deep'])])
def test_split_at_twelve_jobs(n_jobs, k, n_out, kernel, names):
    got = dense_route_rows(_route([(k, n_out, False)] * n_jobs, 1030))
    assert got == [(nm, kernel, list(range(b, min(b + 12, n_jobs)))) for nm, b in zip(names, range(0, n_jobs, 12))]


@pytest.mark.parametrize('n_out,groups', [(160, [[0], [1], [2], [3]]), (128, [[0, 1], [2, 3]])])
def test_split_at_the_lds_budget(n_out, groups):
    """B images of 129 x 160 x 4 = 82,560 B (two do not fit 162,816 B: four launches of one job) and of 129 x 128 x 4 =
    66,048 B (two fit, three do not: two launches of two jobs)."""
    got = _route([(128, n_out, False)] * 4, 515)
    assert [p[2] for p in dense_route_rows(got)] == groups and all(p[1] == 'persist<64>' for p in dense_route_rows(got))
    assert [e.lds_bytes for e in got] == [len(g) * _image(64, n_out) for g in groups]
    assert 2 * _image(64, 160) > BUDGET >= 2 * _image(64, 128) and 3 * _image(64, 128) > BUDGET


@pytest.mark.parametrize('n_deep', [4, 3, 2])
@pytest.mark.parametrize('rows_given', [False, True])
def test_one_call_with_every_class(n_deep, rows_given):
    got = _route(DENSE_MIXED[:9 + n_deep], 1030, rows_given)
    assert dense_route_rows(got) == DENSE_MIXED_PLAN + [('gemm_mfma_deep', DENSE_MIXED_DEEP[n_deep], list(range(9, 9 + n_deep)))]
    assert [e.col_group for e in got] == [0, 0, 0, 2, 5, 5, 5, 2, 0]      # a gated job in the launch: two column tiles per item
    assert ([e.n_out[0] for e in got[5:8]], [e.col0[0] for e in got[5:8]]) == ([64, 288, 4], [0, 0, 288])      # job 6 in two chunks


@pytest.mark.parametrize('n_out,widths', [(292, [288, 4]), (580, [288, 288, 4]), (288, [288])])
def test_gated_chunks_carry_their_gate_offsets(n_out, widths):
    """A gated job of k = 128 cut at 288 columns (162,816 / 4 / 129 = 315 -> 288) beside an ungated job of the same class: every
    chunk reads its gate from the columns it writes, the launches it is in run two column tiles per item, and the last chunk
    shares its launch with the other job whenever both images fit."""
    got = _route([(128, n_out, True), (128, 64, False)], 515)
    mine = [(e, list(e.job[:e.n_jobs]).index(0)) for e in got if 0 in e.job[:e.n_jobs]]
    assert [e.n_out[q] for e, q in mine] == widths
    assert [e.col0[q] for e, q in mine] == [288 * i for i in range(len(widths))]
    assert [e.gate_col0[q] for e, q in mine] == [e.col0[q] for e, q in mine]
    assert all(e.col_group == 2 and e.family == PERSIST and e.variant == 64 for e, q in mine)
    last = got[-1]
    assert list(last.job[:last.n_jobs]) == ([0, 1] if widths[-1] == 4 else [1])
    assert last.gate_col0[last.n_jobs - 1] == -1 and last.col_group == (2 if widths[-1] == 4 else 5)


@pytest.mark.parametrize('k,n_out,n', DENSE_DEEP_CASES, ids=DENSE_DEEP_IDS)
def test_deep_staged_switch(k, n_out, n, monkeypatch):
    """PEA_DEEP_STAGED=1, read per call: every deep job on gemm_mfma_kernel<64>; nothing else moves."""
    usual = dense_route_rows(_route([(k, n_out, False), (64, 64, False)], n))
    monkeypatch.setenv('PEA_DEEP_STAGED', '1')
    got = _route([(k, n_out, False), (64, 64, False)], n)
    assert dense_route_rows(got) == [('gemm_mfma_shared', 'persist<32>', [1]), ('gemm_mfma_deep', 'fallback', [0])]
    assert got[1].family == STAGED and got[1].lds_bytes == 0
    monkeypatch.setenv('PEA_DEEP_STAGED', '0')
    assert dense_route_rows(_route([(k, n_out, False), (64, 64, False)], n)) == usual
    assert usual[0] == ('gemm_mfma_shared', 'persist<32>', [1]) and usual[1][0] == 'gemm_mfma_deep'


def test_rejections():
    from graph_recsys_benchmark_amd import _lib
    # a gate exists in the persistent kernel only.  The check met here is the one of the job conversion pea_dense_route shares
    # with pea_dense_batch_rows (dense_bwd.hip: dense_jobs); it rejects first, so the planner's own gate check (a gate on every
    # segment or none, k <= 128), which guards the library's internal multi-segment jobs, is out of reach of this entry point
    with pytest.raises(_lib.PeaError, match='a gate needs a row stride covering the columns and k <= 128'):
        _route([(64, 64, False), (132, 32, True)], 40)
    with pytest.raises(_lib.PeaError, match='malformed'):      # n_out = 6
        _route([(16, 6, False)], 40)
    arr = _jobs([(64, 20, False)])
    arr[0].ldw = 22
    with pytest.raises(_lib.PeaError, match='multiple of 4'):
        _lib.dense_route(40, False, arr)
    arr = _jobs([(64, 20, False)])
    arr[0].w += 4
    with pytest.raises(_lib.PeaError, match='16-byte'):
        _lib.dense_route(40, False, arr)
    cnt = C.c_int(-1)
    assert _lib.load().pea_dense_route(40, 0, 1, _jobs([(64, 20, False)]), 0, None, C.byref(cnt)) == 0 and cnt.value == 1
    assert _lib.load().pea_dense_route(40, 0, 1, _jobs([(64, 20, False)]), 1, None, C.byref(cnt)) == -1
