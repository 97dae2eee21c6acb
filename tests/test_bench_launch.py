"""bench.py --gpus N self-launch supervision (CPU): a rank that exits non-zero takes the job down at once, with its
exit code, instead of leaving its peers in a collective until a watchdog fires."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _job(code):
    return ([sys.executable, '-c', code], dict(os.environ))


def test_failed_rank_takes_the_job_down_quickly(tmp_path):
    marks = [str(tmp_path / ('alive%d' % r)) for r in range(3)]
    hang = "import sys,time,pathlib; pathlib.Path(sys.argv[1]).write_text('up'); time.sleep(120)"
    jobs = [([sys.executable, '-c', hang, marks[0]], dict(os.environ)),
            _job('import time,sys; time.sleep(0.5); sys.exit(7)'),          # rank 1 dies; ranks 0 and 2 "sit in a collective"
            ([sys.executable, '-c', hang, marks[2]], dict(os.environ))]
    t0 = time.time()
    rc = bench.launch_ranks(jobs, grace_s=2.0)
    dt = time.time() - t0
    assert rc == 7
    assert dt < 20, 'supervision waited %.1f s for peers of a dead rank' % dt
    assert os.path.exists(marks[0]) and os.path.exists(marks[2])       # the peers had really started


def test_signalled_rank_reports_nonzero():
    rc = bench.launch_ranks([_job('import os,signal; os.kill(os.getpid(), signal.SIGKILL)'), _job('import time; time.sleep(60)')],
                            grace_s=2.0)
    assert rc != 0


def test_all_ranks_ok():
    assert bench.launch_ranks([_job('pass'), _job('import time; time.sleep(0.2)')]) == 0


def test_metric_string_follows_the_workload():
    a = bench.parse([])
    assert bench.metric_name(a) == 'BPR-scored edges/sec, PEAGAT MovieLens-25m, emb_dim=64, 9 metapaths'
    b = bench.parse(['--preset', 'yelp_shaped', '--kind', 'sage'])
    assert 'yelp_shaped' in bench.metric_name(b) and 'PEASAGE' in bench.metric_name(b)
    assert bench.metric_name(b) != bench.metric_name(a)


def test_plain_run_leaves_the_extra_legs_to_full():
    a = bench.parse(['--steps', '7', '--warmup', '2'])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    b = bench.parse(['--full', '--dump-outputs', 'out'])
    assert b.full and b.dump_outputs == 'out'


def test_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    import types
    import numpy as np
    import torch
    table = torch.arange(64 * 16, dtype=torch.float32).reshape(64, 16)
    bench.dump_outputs(str(tmp_path / 'whole'), types.SimpleNamespace(cached_repr=table, _repr_partial=False), torch.tensor(1.25))
    assert sorted(os.listdir(tmp_path / 'whole')) == ['cached_repr.npy', 'loss.npy']
    loss = np.load(tmp_path / 'whole' / 'loss.npy')
    assert loss.dtype == np.float64 and loss.tolist() == [1.25]
    got = np.load(tmp_path / 'whole' / 'cached_repr.npy')
    assert got.dtype == np.float32 and np.array_equal(got, table.numpy())
    monkeypatch.setattr(bench, 'DUMP_BYTES', 16 * 4 * 10)          # above the cap: a fixed sample of 10 rows, and their ids
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), types.SimpleNamespace(cached_repr=table, _repr_partial=False), torch.tensor(1.25))
    rows = np.load(tmp_path / 'a' / 'cached_repr_rows.npy')
    assert rows.dtype == np.float64 and rows.size == 10
    assert np.array_equal(np.load(tmp_path / 'a' / 'cached_repr.npy'), table.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / 'b' / 'cached_repr_rows.npy'))
    bench.dump_outputs(str(tmp_path / 'rank'), types.SimpleNamespace(cached_repr=table, _repr_partial=True), torch.tensor(1.25))
    assert os.listdir(tmp_path / 'rank') == ['loss.npy']         # a sharded rank holds only its own rows
