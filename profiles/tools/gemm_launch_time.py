"""Per-launch times of the dense GEMM kernels (csrc/gemm.hip) from the library's launch log (pea_profile_read_ex), for
comparing two builds of libpeahip.so: run once per library (PEA_LIB selects it), several times alternating, and compare the
medians.

    PEA_LIB=/path/to/libpeahip.so python profiles/tools/gemm_launch_time.py [model] [routes]

model:  the headline model's training step (forward, BPR loss, backward), 30 warm-up steps, then 7 logged steps: per gemm_*
        launch of the step (in launch order) the median of its 7 times.
routes: one engine.dense_batch call per row of helpers.DENSE_ROUTES (its largest k and n_out) at n = 1,000,000 rows,
        unlisted and with rows 0, 3, 6, ... listed, and one gated job per k class of the persistent kernel: 2 warm-up
        calls, 7 logged, the median of the call's gemm time.
Times in microseconds.
"""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import DENSE_ROUTES  # noqa: E402
from graph_recsys_benchmark_amd import _lib, engine  # noqa: E402

REPS = 7


def logged(fn):
    """[(launch name, ms)] of fn()"""
    lib = _lib.load()
    cap = 1 << 13
    names = C.create_string_buffer(cap * 32)
    ms, units, gathered, table = (C.c_float * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    cnt = C.c_int()
    lib.pea_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.pea_profile_enable(0)
    _lib.check(lib.pea_profile_read_ex(cap, names, ms, units, gathered, table, C.byref(cnt)))
    return [(names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode(), ms[i]) for i in range(cnt.value)]


def model_step():
    import bench
    from graph_recsys_benchmark_amd.utils.synthetic import SyntheticHIN
    dev = torch.device('cuda', 0)
    ds = SyntheticHIN('ml25m_shaped', seed=2019)
    model = bench.build_model(ds, 'gat', dev)
    model.train()
    batch = torch.from_numpy(ds.bpr_batch()).to(dev)

    def step():
        model.zero_grad()
        model.loss(batch).backward()

    for _ in range(30):
        step()
    torch.cuda.synchronize()
    runs = [[(n, t) for n, t in logged(step) if n.startswith('gemm_')] for _ in range(REPS)]
    assert all([n for n, _ in r] == [n for n, _ in runs[0]] for r in runs), 'the steps differ in their launches'
    for i, (name, _) in enumerate(runs[0]):
        print('model %02d %-22s %9.2f' % (i, name, 1e3 * statistics.median(r[i][1] for r in runs)))
    print('model all gemm launches    %9.2f' % (1e3 * statistics.median(sum(t for _, t in r) for r in runs)))


def routes():
    n = 1000000
    g = torch.Generator(device='cuda').manual_seed(1)
    gated = [((k,), (c,), 'persist<%d> gated' % kh, '', 1, (), 4) for k, c, kh in ((16, 64, 16), (64, 64, 32), (128, 36, 64))]
    for ks, cs, kernel, name, count, ns, off in DENSE_ROUTES + gated:
        k, c = ks[-1], cs[-1]
        a = torch.randn(n, k, generator=g, device='cuda')
        w = torch.randn(k, c, generator=g, device='cuda') * 0.2
        buf = torch.zeros(n, c + 8, device='cuda')
        item = (a, w, buf[:, off:off + c])
        if kernel.endswith('gated'):
            item += (torch.randn(n, c, generator=g, device='cuda'),)
        for listed in (False, True):
            rows = torch.arange(0, n, 3, dtype=torch.int32, device='cuda') if listed else None
            call = lambda: engine.dense_batch([item], rows=rows)
            for _ in range(2):
                call()
            ts = [sum(t for nm, t in logged(call) if nm.startswith('gemm_')) for _ in range(REPS)]
            print('route %-17s k%-5d c%-5d %-8s %9.2f  (min %.2f max %.2f)' % (kernel, k, c, 'listed' if listed else 'unlisted',
                                                                       1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)))
        del a, w, buf


if __name__ == '__main__':
    torch.cuda.set_device(0)
    what = sys.argv[1:] or ['model', 'routes']
    if 'model' in what:
        model_step()
    if 'routes' in what:
        routes()
