"""The deferred error-flag queue (graph_recsys_benchmark_amd/errors.py) on CPU int32 tensors: no device needed."""
import pytest
import torch

from graph_recsys_benchmark_amd import engine, errors


def flag(value=0, persistent=False):
    return torch.full((1,) if persistent else (), value, dtype=torch.int32)


@pytest.fixture(autouse=True)
def empty_queue():
    errors.check()
    yield
    try:
        errors.check()
    except IndexError:
        pass


def test_a_raised_flag_raises_once_and_empties_the_queue():
    errors.defer(flag(0))
    errors.defer(flag(1))
    assert len(errors._pending_err) == 2
    with pytest.raises(IndexError, match='index out of range in BPR triples'):     # the default text
        errors.check()
    assert not errors._pending_err and not errors._pending_what
    errors.check()


def test_the_first_raised_flag_in_queue_order_names_the_message():
    errors.defer(flag(0), 'never raised')
    errors.defer(flag(1), 'second in the queue')
    errors.defer(flag(1), 'third in the queue')
    errors.defer(flag(1))
    with pytest.raises(IndexError, match='^second in the queue$'):
        errors.check()
    errors.defer(flag(1))
    errors.defer(flag(1), 'a named one behind the BPR flag')
    with pytest.raises(IndexError, match='^index out of range in BPR triples$'):
        errors.check()


def test_the_65th_flag_drains_the_queue_first(monkeypatch):
    drains = []
    real = errors.check
    monkeypatch.setattr(errors, 'check', lambda: (drains.append(len(errors._pending_err)), real())[1])
    for _ in range(64):
        errors.defer(flag(0))
    assert drains == [] and len(errors._pending_err) == errors.MAX_PENDING == 64
    last = flag(0)
    errors.defer(last)
    assert drains == [64]
    assert len(errors._pending_err) == 1 and errors._pending_err[0] is last


def test_a_persistent_flag_is_queued_once_survives_checks_and_is_rearmed():
    f = flag(0, persistent=True)
    before = len(errors._persistent)
    for _ in range(3):
        errors.defer_persistent(f)
    assert len(errors._persistent) == before + 1
    errors.check()                                  # clean: nothing raised, still registered
    f.fill_(1)
    with pytest.raises(IndexError, match='BPR triples'):
        errors.check()
    assert int(f) == 0 and not errors._pending_err  # zeroed, the one-shot queue empty
    errors.check()
    f.fill_(1)                                      # set again: raises again without a new defer_persistent
    with pytest.raises(IndexError):
        errors.check()
    assert int(f) == 0
    del f
    errors.check()
    assert len(errors._persistent) == before        # its owner dropped it: no longer read


def test_a_one_shot_flag_is_named_before_a_persistent_one():
    f = flag(1, persistent=True)
    errors.defer_persistent(f)
    errors.defer(flag(1), 'the one-shot flag')
    with pytest.raises(IndexError, match='^the one-shot flag$'):
        errors.check()
    assert int(f) == 0


def test_engine_shares_the_queue_and_its_entry_points():
    assert engine._pending_err is errors._pending_err
    assert engine.check_pending_errors is errors.check and engine._defer_error is errors.defer
    engine._defer_error(flag(1))
    assert engine._pending_err is errors._pending_err and len(engine._pending_err) == 1
    with pytest.raises(IndexError):
        engine.check_pending_errors()
    assert engine._pending_err is errors._pending_err and not engine._pending_err


def test_ws_flag_views_a_small_workspace_and_clones_out_of_a_large_one():
    assert errors.WS_FLAG_VIEW_MAX == 4096 and errors.MAX_PENDING * errors.WS_FLAG_VIEW_MAX == 256 * 1024
    small = torch.zeros(4096, dtype=torch.uint8)
    large = torch.zeros(4097, dtype=torch.uint8)
    for ws in (small, large):
        ws[:4] = torch.tensor([1], dtype=torch.int32).view(torch.uint8)
    fs, fl = errors.ws_flag(small), errors.ws_flag(large)
    assert fs.dtype == fl.dtype == torch.int32 and fs.dim() == fl.dim() == 0 and int(fs) == int(fl) == 1
    assert fs.untyped_storage().data_ptr() == small.untyped_storage().data_ptr()
    assert fl.untyped_storage().nbytes() == 4
