"""The dense products (csrc/gemm.hip through pea_dense_batch[_rows], csrc/dense_bwd.hip through pea_grad_weight[_rows]) on every
route their dispatch can take, each against a float64 torch product of the same operands, with the route read back from the
library: its plan for the call and its launch log.

Two bounds per product, neither tuned on the kernels:
  1. elementwise |got - want| <= (k + 4) 2^-24 (|a| |w|) + 1e-30: the forward bound of an fp32 dot product of length k in any
     summation order (products exact or fused), so every route must meet it (grad_weight: k = the rows summed);
  2. the per-array bounds of tests/test_gpu_dense.py: 2e-6 max|want| sqrt(k), and 3e-6 max|want| max(1, sqrt(n / 1000)) + 1e-4
     for grad_weight.
Outputs are column blocks of NaN-filled buffers: whatever lies outside a job's rows x columns must still be NaN afterwards.

Two accounts of the route, both from the library.  The launch log (pea_profile_read) names what was actually launched: the
profile names separate the narrow kernel (gemm_mfma_narrow), the persistent kernel with one job (gemm_mfma_shared) or several
(gemm_mfma_batch) and the deep-k launches (gemm_mfma_deep), and their count gives the column chunks and the batch splits.  It
cannot tell the template variants apart: skinny<2/4/8>, persist<16/32/64> and the deep resident / 128-chunk / fallback kernels
share their names.  Those come from pea_dense_route, the planner launch_gemm_batch itself executes, asked about the very job
structs of each call (engine.dense_batch(route=...)): every call asserts that its log matches the plan's names, and the
hand-written tables (tests/helpers.py: DENSE_ROUTES, DENSE_MIXED_PLAN) are asserted against the plan's kernels, variants and
batch composition.  The same tables are put to the planner without a GPU in tests/test_dense_route_cpu.py."""
import contextlib
import ctypes as C

import pytest
import torch

from helpers import (DENSE_DEEP_CASES, DENSE_DEEP_IDS, DENSE_MIXED, DENSE_MIXED_DEEP, DENSE_MIXED_PLAN, DENSE_ROUTE_CASES,
                     DENSE_ROUTE_IDS, dense_route_rows)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ helpers
@contextlib.contextmanager
def _launch_log():
    """The names of the library's launches inside the block, in order (pea_profile_enable / pea_profile_read)."""
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    names = []
    cnt = C.c_int()
    lib.pea_profile_read(0, None, None, None, C.byref(cnt))      # drop whatever an earlier user left
    lib.pea_profile_enable(1)
    try:
        yield names
        torch.cuda.synchronize()
    finally:
        lib.pea_profile_enable(0)
        cap = 1024
        buf = C.create_string_buffer(cap * 32)
        lib.pea_profile_read(cap, buf, None, None, C.byref(cnt))
        names += [buf.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode() for i in range(cnt.value)]


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _same_bits(x, y):
    """equal as 32-bit words (torch.equal would take -0.0 for 0.0)"""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


class _Job:
    """One product a [n, k] @ w [k, n_out] -> out, all three (and the gate) column blocks of wider buffers when `wide`: then
    every cell around a, w and the gate is NaN, so a value loaded from outside a block and used shows in the result."""

    def __init__(self, n, k, n_out, gen, gated=False, wide=False, out_off=4, out_pad=8):
        self.n, self.k, self.n_out = n, k, n_out
        a = torch.randn(n, k, generator=gen).cuda()
        w = (torch.randn(k, n_out, generator=gen) * 0.2).cuda()
        gate = torch.randn(n, n_out, generator=gen).cuda() if gated else None
        if wide:
            ab, wb = _nan(n, k + 16), _nan(k + 3, n_out + 12)
            ab[:, 8:8 + k] = a
            wb[:k, 4:4 + n_out] = w
            a, w = ab[:, 8:8 + k], wb[:k, 4:4 + n_out]
            if gated:
                gb = _nan(n, n_out + 8)
                gb[:, 4:4 + n_out] = gate
                gate = gb[:, 4:4 + n_out]
        self.a, self.w, self.gate = a, w, gate
        self.off = out_off
        self.buf = _nan(n, n_out + out_pad)
        self.out = self.buf[:, out_off:out_off + n_out]
        self.want = a.double() @ w.double()
        self.bound = (k + 4) * 2.0 ** -24 * (a.double().abs() @ w.double().abs()) + 1e-30
        if gated:
            self.want = torch.where(gate > 0, self.want, torch.zeros_like(self.want))

    def item(self):
        return (self.a, self.w, self.out) if self.gate is None else (self.a, self.w, self.out, self.gate)

    def reset(self):
        self.buf.fill_(float('nan'))
        return self

    def check(self, rows=None):
        """the written block against float64 (both bounds), everything else still NaN"""
        sel = torch.arange(self.n, device='cuda') if rows is None else rows.long()
        want = self.want
        got = self.out[sel]
        assert not bool(torch.isnan(got).any()), 'NaN inside the job (a cell not written, or a value from outside the operands)'
        err = (got.double() - want[sel]).abs()
        if sel.numel():
            ratio = float((err / self.bound[sel]).max())
            top, scale = float(err.max()), float(want[sel].abs().max())
            print('n=%d k=%d n_out=%d rows=%d: max err / elementwise bound = %.3f, max err = %.3e (array bound %.3e)'
                  % (self.n, self.k, self.n_out, sel.numel(), ratio, top, 2e-6 * scale * self.k ** 0.5))
            assert ratio <= 1.0, 'elementwise bound missed by a factor of %.3f' % ratio
            assert top <= 2e-6 * scale * self.k ** 0.5, (top, scale)
        rest = torch.ones(self.n, dtype=torch.bool, device='cuda')
        rest[sel] = False
        assert bool(torch.isnan(self.buf[rest]).all()), 'a row outside the list was written'
        assert bool(torch.isnan(self.buf[:, :self.off]).all()) and bool(torch.isnan(self.buf[:, self.off + self.n_out:]).all()), \
            'a column outside the job was written'


def _run(jobs, rows=None):
    """One dense_batch call: the names in its launch log, which must be the names of the library's plan for the very job
    structs of the call, and that plan as (profile name, kernel, [source job, ...]) rows."""
    from graph_recsys_benchmark_amd import engine
    route = []
    with _launch_log() as names:
        engine.dense_batch([j.item() for j in jobs], rows=rows, route=route)
    plan = dense_route_rows(route)
    assert names == [p[0] for p in plan], 'the launch log and the plan differ'
    assert all(e.listed == (rows is not None) for e in route)
    return names, plan


def _rows3(n):
    return torch.arange(0, n, 3, dtype=torch.int32, device='cuda')


_EMPTY = dict(dtype=torch.int32, device='cuda')

def _one_route(k, n_out, kernel, name, count, n, off):
    g = torch.Generator().manual_seed(1000 * k + 7 * n_out + n)
    job = _Job(n, k, n_out, g, out_off=off)
    want = [(name, kernel, [0])] * count        # the table: against the library's plan and (the names) against its launch log
    assert _run([job]) == ([name] * count, want)
    job.check()
    first = job.out.clone()
    assert _run([job.reset()]) == ([name] * count, want)
    assert _same_bits(job.out, first), 'two identical calls differ'
    rows = _rows3(n)
    assert _run([job.reset()], rows=rows) == ([name] * count, want)
    job.check(rows)
    assert _same_bits(job.out[rows.long()], first[rows.long()]), 'a listed row differs from the same row of the unlisted call'
    assert _run([job.reset()], rows=torch.empty(0, **_EMPTY)) == ([], [])
    assert bool(torch.isnan(job.buf).all()), 'an empty row list wrote something'


# ------------------------------------------------------------------------------------------------ 1. one case per route
@pytest.mark.parametrize('k,n_out,kernel,name,count,n,off', DENSE_ROUTE_CASES, ids=DENSE_ROUTE_IDS)
def test_every_route_matches_float64(k, n_out, kernel, name, count, n, off):
    """Unlisted, rows 0, 3, 6, ... listed, and an empty list; two calls bit-identical, listed rows bit-identical to unlisted."""
    _one_route(k, n_out, kernel, name, count, n, off)


@pytest.mark.parametrize('k,n_out,n', DENSE_DEEP_CASES, ids=DENSE_DEEP_IDS)
def test_deep_shapes_on_the_fallback_kernel(k, n_out, n, monkeypatch):
    """PEA_DEEP_STAGED=1 (read per call) sends every deep job to gemm_mfma_kernel<64>: the shapes the resident and the
    128-chunk kernels normally take, on the kernel that otherwise only sees n_out > 128."""
    monkeypatch.setenv('PEA_DEEP_STAGED', '1')
    _one_route(k, n_out, 'fallback', 'gemm_mfma_deep', 1, n, 4)


# ------------------------------------------------------------------------------------------------ 2. batches
def _alone(job, rows=None):
    """the ungated product of the job's operands from a call of its own"""
    solo = torch.full_like(job.buf, float('nan'))
    from graph_recsys_benchmark_amd import engine
    engine.dense_batch([(job.a, job.w, solo[:, job.off:job.off + job.n_out])], rows=rows)
    return solo[:, job.off:job.off + job.n_out]


def _same_bits_as_alone(job, rows=None):
    sel = torch.arange(job.n, device='cuda') if rows is None else rows.long()
    solo = _alone(job, rows)[sel]
    if job.gate is not None:
        solo = torch.where(job.gate[sel] > 0, solo, torch.zeros_like(solo))
    assert _same_bits(job.out[sel], solo), 'k=%d n_out=%d: bits differ between the batch and a call of its own' % (job.k, job.n_out)


@pytest.mark.parametrize('n_jobs,k,n_out,names', [
    (13, 16, 64, ['gemm_mfma_batch', 'gemm_mfma_shared']),
    (25, 16, 64, ['gemm_mfma_batch', 'gemm_mfma_batch', 'gemm_mfma_shared']),
    (13, 64, 16, ['gemm_mfma_narrow', 'gemm_mfma_narrow'])])
@pytest.mark.parametrize('listed', [False, True])
def test_batches_split_at_twelve_jobs(n_jobs, k, n_out, names, listed):
    n = 1030
    g = torch.Generator().manual_seed(n_jobs + k)
    jobs = [_Job(n, k, n_out, g) for _ in range(n_jobs)]
    rows = _rows3(n) if listed else None
    got, plan = _run(jobs, rows=rows)
    assert got == names and [p[2] for p in plan] == [list(range(b, min(b + 12, n_jobs))) for b in range(0, n_jobs, 12)]
    for j in jobs:
        j.check(rows)
    for j in (jobs[0], jobs[11], jobs[12], jobs[-1]):       # either side of the split
        _same_bits_as_alone(j, rows)


@pytest.mark.parametrize('n', [64, 4099])
def test_skinny_item_orders_give_the_same_bits(n, monkeypatch):
    """Jobs with equal tile counts are walked tile-major (item i = tile i / n_jobs of job i % n_jobs); PEA_SKINNY_JOBMAJOR=1
    restores the job-major order.  Which wave computes a tile must not change a bit."""
    g = torch.Generator().manual_seed(n)
    jobs = [_Job(n, k, c, g) for k, c in ((64, 16), (36, 12), (64, 4), (40, 16), (64, 8))]
    assert _run(jobs)[0] == ['gemm_mfma_narrow']
    for j in jobs:
        j.check()
    tile_major = [j.out.clone() for j in jobs]
    monkeypatch.setenv('PEA_SKINNY_JOBMAJOR', '1')
    assert _run([j.reset() for j in jobs])[0] == ['gemm_mfma_narrow']
    for j, t in zip(jobs, tile_major):
        j.check()
        assert _same_bits(j.out, t)
        _same_bits_as_alone(j)


@pytest.mark.parametrize('n_out,names', [(160, ['gemm_mfma_shared'] * 4), (128, ['gemm_mfma_batch'] * 2)])
def test_batches_split_at_the_lds_budget(n_out, names):
    """B images of 129 x 160 x 4 = 82,560 B (two do not fit 162,816 B: four launches of one job) and of 129 x 128 x 4 =
    66,048 B (two fit, three do not: two launches of two jobs)."""
    n = 515
    g = torch.Generator().manual_seed(n_out)
    jobs = [_Job(n, 128, n_out, g) for _ in range(4)]
    got, plan = _run(jobs)
    assert got == names and [p[2] for p in plan] == ([[0], [1], [2], [3]] if n_out == 160 else [[0, 1], [2, 3]])
    for j in jobs:
        j.check()
        _same_bits_as_alone(j)


@pytest.mark.parametrize('n_deep,deep_kernel', [(4, 'fallback'), (3, 'staged<4>'), (2, 'resident<2>')])     # DENSE_MIXED_DEEP
@pytest.mark.parametrize('listed', [False, True])
def test_one_call_with_every_class(n_deep, deep_kernel, listed):
    """All classes in one call.  The deep group's kernel follows from its largest k and n_out: with (132, 132) the fallback, with
    (136, 128) the four-tile 128-chunk kernel for all three, with the first two the resident kernel (B images of different
    depth in one launch).  Gated and ungated jobs share the persistent launches (2 column tiles per item for all of them)."""
    n = 1030
    g = torch.Generator().manual_seed(n_deep)
    jobs = [_Job(n, k, c, g, gated=gt) for k, c, gt in DENSE_MIXED[:9 + n_deep]]
    assert deep_kernel == DENSE_MIXED_DEEP[n_deep]
    rows = _rows3(n) if listed else None
    names, plan = _run(jobs, rows=rows)
    assert plan == DENSE_MIXED_PLAN + [('gemm_mfma_deep', deep_kernel, list(range(9, 9 + n_deep)))]
    for j in jobs:
        j.check(rows)
    for j in jobs[:9]:          # not promised across the deep variants (the resident kernel pairs k with k + 4, the others k with k + 64)
        _same_bits_as_alone(j, rows)
    first = [j.out.clone() for j in jobs]
    assert _run([j.reset() for j in jobs], rows=rows) == (names, plan)
    sel = slice(None) if rows is None else rows.long()
    assert all(_same_bits(j.out[sel], t[sel]) for j, t in zip(jobs, first)), 'two identical calls differ'


@pytest.mark.parametrize('n_out,count', [(292, 2), (580, 3)])
@pytest.mark.parametrize('listed', [False, True])
def test_chunked_gate_with_planted_zeros(n_out, count, listed):
    """A gated job cut into column chunks (the chunk's gate pointer moves with its columns) beside an ungated job of the same k
    class.  Bitwise where(gate > 0, ungated, 0); of the planted gate values 0.0, -0.0 and 1e-30 only the last is open."""
    n, k = 515, 128
    g = torch.Generator().manual_seed(n_out)
    gated, plain = _Job(n, k, n_out, g, gated=True, wide=True), _Job(n, k, 64, g)
    cells = [(r, c) for r in (0, 3, 513) for c in (0, 31, 32, 287, 288, n_out - 1)]       # rows 0, 3, 513 are on the list too
    vals = [0.0, -0.0, 1e-30]
    for q, (r, c) in enumerate(cells):
        gated.gate[r, c] = vals[q % 3]
    gated.want = torch.where(gated.gate > 0, gated.a.double() @ gated.w.double(), torch.zeros_like(gated.want))
    rows = _rows3(n) if listed else None
    # chunk images: 288 columns 148,608 B, the last chunk (<= 32 columns) 16,512 B, the 64-column job 33,024 B
    names, plan = _run([gated, plain], rows=rows)
    assert len(names) == count and [p[2] for p in plan] == [[0]] * (count - 1) + [[0, 1]]     # the last chunk beside the plain job
    gated.check(rows)
    plain.check(rows)
    _same_bits_as_alone(gated, rows)
    _same_bits_as_alone(plain, rows)
    solo = _alone(gated, rows)
    for q, (r, c) in enumerate(cells):
        got = float(gated.out[r, c])
        if q % 3 == 2:
            assert _same_bits(gated.out[r, c], solo[r, c]) and got != 0.0, (r, c, got)
        else:
            assert _same_bits(gated.out[r, c], torch.zeros((), device='cuda')), (r, c, got)      # +0.0, not -0.0


# ------------------------------------------------------------------------------------------------ 3. strided operands
@pytest.mark.parametrize('k,n_out,gated,names', [
    (64, 16, False, ['gemm_mfma_narrow']),
    (16, 64, True, ['gemm_mfma_shared']),
    (64, 100, True, ['gemm_mfma_shared']),
    (128, 36, False, ['gemm_mfma_shared']),
    (128, 300, False, ['gemm_mfma_shared'] * 2),      # chunks of 288 + 12 columns
    (128, 300, True, ['gemm_mfma_shared'] * 2),
    (64, 612, True, ['gemm_mfma_shared'] * 2),
    (260, 32, False, ['gemm_mfma_deep']),             # resident<1>
    (576, 64, False, ['gemm_mfma_deep']),             # resident<2>
    (700, 36, False, ['gemm_mfma_deep']),             # staged<2>
    (136, 100, False, ['gemm_mfma_deep']),            # staged<4>
    (132, 132, False, ['gemm_mfma_deep'])])           # fallback
@pytest.mark.parametrize('n', [33, 1030])
def test_operands_inside_nan_filled_buffers(k, n_out, gated, names, n):
    """a = wide_a[:, 8:8 + k], w = big[:k, 4:4 + n_out] (rows below the block too), gate and out at 4-float offsets, and
    every cell around the blocks NaN.  The B images are padded to 32 columns: what fills the pad may be anything, but it may
    never reach a stored column, and the strides must be honoured wherever a B image is loaded -- the result is finite,
    within the bounds, and bit-identical to the same product from contiguous operands."""
    from graph_recsys_benchmark_amd import engine
    g = torch.Generator().manual_seed(k + n_out + n)
    job = _Job(n, k, n_out, g, gated=gated, wide=True)
    assert job.w.stride(0) % 4 == 0 and job.w.stride(0) > n_out and job.a.stride(0) > k
    for rows in (None, _rows3(n)):
        assert _run([job.reset()], rows=rows)[0] == names
        job.check(rows)
        dense = _nan(n, n_out)
        item = (job.a.contiguous(), job.w.contiguous(), dense) + ((job.gate.contiguous(),) if gated else ())
        engine.dense_batch([item], rows=rows)
        sel = slice(None) if rows is None else rows.long()
        assert _same_bits(job.out[sel], dense[sel])


# ------------------------------------------------------------------------------------------------ 4. weight gradient
_GW_MA, _GW_NB = (1, 16, 17, 20, 32, 33, 48, 64), (4, 16, 17, 32, 36, 64)


def _gw_check(pairs, outs, n_sum, sel=None):
    for (a, b), out in zip(pairs, outs):
        a64, b64 = (a.double(), b.double()) if sel is None else (a[sel].double(), b[sel].double())
        want = a64.t() @ b64
        bound = (n_sum + 4) * 2.0 ** -24 * (a64.abs().t() @ b64.abs()) + 1e-30
        assert out.shape == want.shape and not bool(torch.isnan(out).any())
        err = (out.double() - want).abs()
        ratio, top, scale = float((err / bound).max()), float(err.max()), float(want.abs().max())
        assert ratio <= 1.0, 'grad_weight %s: elementwise bound missed by a factor of %.3f' % (tuple(want.shape), ratio)
        assert top <= 3e-6 * scale * max(1.0, (n_sum / 1000.0) ** 0.5) + 1e-4, (tuple(want.shape), top, scale)


def _gw_tile_pairs(n, g):
    """all 48 (ma, nb) pairs as column blocks of two wide buffers, at column offsets that are not multiples of 4 either"""
    wa, wb = torch.randn(n, 72, generator=g).cuda(), torch.randn(n, 72, generator=g).cuda()
    return [(wa[:, q % 7:q % 7 + ma], wb[:, (3 * q) % 8:(3 * q) % 8 + nb])
            for q, (ma, nb) in enumerate((ma, nb) for ma in _GW_MA for nb in _GW_NB)]


def _gw_45_pairs(n, g):
    wa, wb = torch.randn(n, 64 * 9, generator=g).cuda(), torch.randn(n, 64 * 5, generator=g).cuda()
    return [(wa[:, 64 * i:64 * i + 64], wb[:, 64 * j:64 * j + 64]) for i in range(9) for j in range(5)]


@pytest.mark.parametrize('n', [1, 37, 4099])
def test_grad_weight_every_tile_shape_in_one_call(n):
    """(ma, nb) classes <= 16 / <= 32 / <= 64 on both sides: all nine launch_gw<MT, NT> shapes, several blocks each."""
    from graph_recsys_benchmark_amd import engine
    pairs = _gw_tile_pairs(n, torch.Generator().manual_seed(n))
    with _launch_log() as names:
        outs = engine.grad_weight(pairs)
    assert names == ['grad_weight', 'grad_weight_sum'] * 9
    _gw_check(pairs, outs, n)
    again = engine.grad_weight(pairs)
    assert all(_same_bits(x, y) for x, y in zip(outs, again))


@pytest.mark.parametrize('n', [37, 4099])
def test_grad_weight_more_blocks_than_one_launch_holds(n):
    """45 blocks of 64 x 64 against kGwMaxJobs = 40: two pairs of launches."""
    from graph_recsys_benchmark_amd import engine
    pairs = _gw_45_pairs(n, torch.Generator().manual_seed(n))
    with _launch_log() as names:
        outs = engine.grad_weight(pairs)
    assert names == ['grad_weight', 'grad_weight_sum'] * 2
    _gw_check(pairs, outs, n)
    again = engine.grad_weight(pairs)
    assert all(_same_bits(x, y) for x, y in zip(outs, again))


@pytest.mark.parametrize('n', [37, 4099])
@pytest.mark.parametrize('which', ['tiles', 'blocks45'])
def test_grad_weight_over_an_empty_and_a_full_row_set(n, which):
    """A RowSet with count 0 gives the product over no rows (exact zeros, written, not left alone); with count N the full one."""
    from graph_recsys_benchmark_amd import engine
    pairs = (_gw_tile_pairs if which == 'tiles' else _gw_45_pairs)(n, torch.Generator().manual_seed(n + 1))
    none = engine.RowSet(n, torch.device('cuda')).fill_from(torch.zeros(n, 4, device='cuda'), 4)
    every = engine.RowSet(n, torch.device('cuda')).fill_from(torch.ones(n, 4, device='cuda'), 4)
    assert int(none.count.item()) == 0 and int(every.count.item()) == n
    for _ in range(2):      # the second call finds the first one's values in the recycled output blocks
        outs = engine.grad_weight(pairs, rows=none)
        assert all(bool((o == 0).all()) for o in outs)
        outs = engine.grad_weight(pairs, rows=every)
        _gw_check(pairs, outs, n)
    again = engine.grad_weight(pairs, rows=every)
    assert all(_same_bits(x, y) for x, y in zip(outs, again))
    some = torch.zeros(n, 4, device='cuda')
    some[::3, 1] = 1.0
    third = engine.RowSet(n, torch.device('cuda')).fill_from(some, 4)
    _gw_check(pairs, engine.grad_weight(pairs, rows=third), (n + 2) // 3, sel=torch.arange(0, n, 3, device='cuda'))


# ------------------------------------------------------------------------------------------------ 5. argument checks
def test_dense_batch_argument_checks():
    from graph_recsys_benchmark_amd import _lib, engine
    n = 40
    g = torch.Generator().manual_seed(5)
    a = torch.randn(n, 260, generator=g).cuda()
    with pytest.raises(_lib.PeaError):       # a gate exists in the persistent kernel only: k <= 128
        engine.dense_batch([(a[:, :132], torch.randn(132, 32, generator=g).cuda(), _nan(n, 32), torch.ones(n, 32, device='cuda'))])
    with pytest.raises(_lib.PeaError):       # n_out = 6
        engine.dense_batch([(a[:, :16], torch.randn(16, 6, generator=g).cuda(), _nan(n, 6))])
    # a weight view whose row stride is not a multiple of 4 floats: the library refuses it (its B loaders read 16 bytes at a
    # time and would straddle rows); the engine hands over a copy instead
    for k, n_out in ((64, 20), (16, 16), (260, 20)):
        wide_w = (torch.randn(k, n_out + 2, generator=g) * 0.2).cuda()
        w = wide_w[:, :n_out]
        out = _nan(n, n_out)
        job = _lib.DenseJob(a.data_ptr(), a.stride(0), k, w.data_ptr(), w.stride(0), n_out, out.data_ptr(), out.stride(0), None, 0)
        rc = _lib.load().pea_dense_batch(n, 1, (_lib.DenseJob * 1)(job), _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == -1 and 'multiple of 4' in _lib.last_error(), (rc, _lib.last_error())
        assert bool(torch.isnan(out).all())
        engine.dense_batch([(a[:, :k], w, out)])
        want = a[:, :k].double() @ w.double()
        err = (out.double() - want).abs()
        assert bool((err <= (k + 4) * 2.0 ** -24 * (a[:, :k].double().abs() @ w.double().abs()) + 1e-30).all())
    # ... nor a weight block that does not start on a 16-byte boundary (here one float into its buffer)
    k, n_out = 64, 20
    flat = (torch.randn(k * n_out + 4, generator=g) * 0.2).cuda()
    w = flat[1:1 + k * n_out].view(k, n_out)
    out = _nan(n, n_out)
    job = _lib.DenseJob(a.data_ptr(), a.stride(0), k, w.data_ptr(), w.stride(0), n_out, out.data_ptr(), out.stride(0), None, 0)
    rc = _lib.load().pea_dense_batch(n, 1, (_lib.DenseJob * 1)(job), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and '16-byte' in _lib.last_error(), (rc, _lib.last_error())
    assert bool(torch.isnan(out).all())
    engine.dense_batch([(a[:, :k], w, out)])
    err = (out.double() - a[:, :k].double() @ w.double()).abs()
    assert bool((err <= (k + 4) * 2.0 ** -24 * (a[:, :k].double().abs() @ w.double().abs()) + 1e-30).all())
