"""The deferred device error flags.  A launch that validates ids on the device sets an int32 flag instead of stopping; the
flag is queued here and read where the host synchronizes anyway (predict, rank_eval, model.eval(), bpr_score(validate=True)),
one host read for all of them.  The queue keeps a flag's storage alive until then, so the rule is: a queued flag pins at most
WS_FLAG_VIEW_MAX bytes -- ws_flag() views a small workspace and takes a 4-byte clone out of a large one."""
import weakref

import torch

MAX_PENDING = 64            # one-shot flags queued before defer() checks first: a long async loop never grows the list
WS_FLAG_VIEW_MAX = 4096     # a full queue of workspace views pins at most 64 x 4 KiB = 256 KiB
BPR_MESSAGE = 'index out of range in BPR triples'

_pending_err = []           # the queued one-shot flags, in launch order; never rebound (engine._pending_err is this list)
_pending_what = []          # _pending_what[k]: the IndexError message of _pending_err[k]
_persistent = []            # weak references to the flags of defer_persistent, each once


def check():
    """Raise IndexError if a launch since the last check saw an id out of range -- what the reference raises at
    `cached_repr[unids]` (models/base.py:209-210) -- with the message of the first raised flag: the one-shot flags in queue
    order, then the persistent ones.  Reading the flags is a stream synchronize.  The one-shot flags are dropped either way;
    a persistent flag stays registered while its owner lives and is zeroed (re-armed) after a raise."""
    kept = [f for f in (ref() for ref in _persistent) if f is not None]
    _persistent[:] = [weakref.ref(f) for f in kept]
    flags, messages = _pending_err + kept, _pending_what + [BPR_MESSAGE] * len(kept)
    del _pending_err[:], _pending_what[:]
    raised = torch.stack([f.reshape(-1)[0] for f in flags]).tolist() if flags else []
    if any(raised):
        for f in kept:
            f.zero_()
        raise IndexError(next(m for m, v in zip(messages, raised) if v))


def defer(flag, what=None):
    """Queue the int32 error flag of one launch for the next check(); `what`: its IndexError message, if not the BPR one."""
    if len(_pending_err) >= MAX_PENDING:
        check()
    _pending_err.append(flag)
    _pending_what.append(what or BPR_MESSAGE)


def defer_persistent(flag):
    """Register a flag that its owner hands to launch after launch (sharding.ShardLayout); registering it again is a no-op."""
    if not any(ref() is flag for ref in _persistent):
        _persistent.append(weakref.ref(flag))


def ws_flag(ws):
    """The int32 error flag a kernel leaves at byte 0 of its uint8 workspace `ws`, fit for defer(): a view of a small
    workspace, a 4-byte clone (one more launch) out of one above WS_FLAG_VIEW_MAX bytes."""
    flag = ws[:4].view(torch.int32)[0]
    return flag if ws.numel() <= WS_FLAG_VIEW_MAX else flag.clone()
