"""Dense helpers of the conv-stack backward (autograd.py): row sets, weight gradients, batched products, the two-layer
backward data path and the column-block sum.  PyTorch holds the memory; the arithmetic runs in libpeahip.so."""
import torch

from . import _lib


def _rows2d(t):
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1:
        raise ValueError('expected a CUDA float32 [rows, cols] view with unit column stride')
    return t


_cached_ws = {}


def _workspace(what, device, nbytes):
    """The uint8 workspace of `nbytes` that the calls named `what` share on `device`: allocated once, then reused."""
    key = (what, device, nbytes)
    if key not in _cached_ws:
        _cached_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return _cached_ws[key]


class RowSet:
    """Rows of a table that hold a non-zero, on the device: flags uint8 [N], ids int32 [N] (the first `count` valid, ascending),
    count int32 [1] -- the host never reads the count (csrc/rows.hip).  Buffers are allocated once and refilled."""

    def __init__(self, n, device):
        lib = _lib.require_device()
        self.n = int(n)
        self.flags = torch.zeros(self.n, dtype=torch.uint8, device=device)
        self.ids = torch.zeros(self.n, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self._ws = torch.empty(int(lib.pea_rows_nonzero_workspace_bytes(self.n)), dtype=torch.uint8, device=device)

    def zero_rows_of(self, table, width):
        """table[ids[q], 0:width] = 0 for the listed rows."""
        table = _rows2d(table)
        _lib.check(_lib.load().pea_rows_zero(_lib.ptr(table), table.stride(0), int(width), _lib.ptr(self.ids), _lib.ptr(self.count),
                                             _lib.current_stream()))

    def fill_from(self, table, width, also=None):
        """flags / ids / count of the rows of table [N, ld] whose first `width` columns hold a non-zero -- or that are flagged
        in `also` (uint8 [N])."""
        table = _rows2d(table)
        _lib.check(_lib.load().pea_rows_nonzero_or(self.n, int(width), _lib.ptr(table), table.stride(0), _lib.ptr(also),
                                                   _lib.ptr(self.flags), _lib.ptr(self.ids), _lib.ptr(self.count),
                                                   _lib.ptr(self._ws), self._ws.numel(), _lib.current_stream()))
        return self


def grad_weight(pairs, shard=None, rows=None):
    """[a_q^T b_q for (a_q, b_q) in pairs]: a_q [N, ma], b_q [N, nb] float32 views (row strides free) over the same N
    rows -- the weight gradients of one level in one pair of launches (pea_grad_weight: fixed-order reduction).  A pair may
    carry (mask uint8 [N], alt [N, nb]): rows flagged in mask take their b operand from alt (include/peahip.h, pea_gw_job).
    shard = (rank, world, tile): this rank's SHARE (the sum over the rows it owns); the caller all-reduces."""
    lib = _lib.require_device()
    if not pairs:
        return []
    n = pairs[0][0].shape[0]
    dev = pairs[0][0].device
    jobs = (_lib.GwJob * len(pairs))()
    outs = []
    for q, item in enumerate(pairs):
        a, b = _rows2d(item[0]), _rows2d(item[1])
        mask, alt = (item[2], _rows2d(item[3])) if len(item) > 2 else (None, None)     # rows flagged in mask read alt instead of b
        alt_scale = item[4] if len(item) > 4 else None                                  # ... times alt_scale[row] (float32 [N])
        if a.shape[0] != n or b.shape[0] != n:
            raise ValueError('grad_weight: operands of one call must share the row count')
        out = torch.empty((a.shape[1], b.shape[1]), dtype=torch.float32, device=dev)
        outs.append(out)
        if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n or alt.shape != b.shape):
            raise ValueError('grad_weight: the row mask must be uint8 [N] and the alternative operand shaped like b')
        jobs[q] = _lib.GwJob(a.data_ptr(), a.stride(0), a.shape[1], b.data_ptr(), b.stride(0), b.shape[1],
                             out.data_ptr(), out.stride(0), None if mask is None else mask.data_ptr(),
                             None if alt is None else alt.data_ptr(), 0 if alt is None else alt.stride(0),
                             None if alt_scale is None else alt_scale.data_ptr())
    ws = _workspace('grad_weight', dev, int(lib.pea_grad_weight_workspace_bytes()))
    if rows is not None:        # RowSet: the reduction runs over the listed rows only (the others contribute exact zeros)
        _lib.check(lib.pea_grad_weight_rows(n, _lib.ptr(rows.ids), _lib.ptr(rows.count), rows.n, len(pairs), jobs, _lib.ptr(ws),
                                            ws.numel(), _lib.current_stream()))
    elif shard is not None and shard[1] > 1:
        _lib.check(lib.pea_grad_weight_sharded(n, int(shard[2]), int(shard[1]), int(shard[0]), len(pairs), jobs, _lib.ptr(ws),
                                               ws.numel(), _lib.current_stream()))
    else:
        _lib.check(lib.pea_grad_weight(n, len(pairs), jobs, _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    return outs


def dense_batch(triples_, rows=None, route=None):
    """out_q = a_q @ w_q for (a_q [N, k], w_q [k, n_out], out_q [N, n_out] view) in triples_: one launch (the input
    gradients dIn = dT W of one level); k, n_out and a's row stride must be multiples of 4 (a w whose row stride is not,
    or that does not start on a 16-byte boundary, is copied first).  rows (int32 device tensor): only those rows are
    computed (the rows a rank owns in a sharded training step).  A fourth element gate_q [N, n_out] (k <= 128) zeroes the
    outputs where gate_q <= 0: the relu mask of the layer below, applied in the epilogue.  route: diagnostic only -- a list
    that receives the library's account of the launches this call makes (_lib.dense_route of the very job structs); the
    tests of the dispatch use it, nothing in the product does."""
    lib = _lib.require_device()
    if not triples_:
        return
    n = triples_[0][0].shape[0]
    jobs = (_lib.DenseJob * len(triples_))()
    keep = []
    for q, item in enumerate(triples_):
        a, w, out = item[:3]
        gate = item[3] if len(item) > 3 else None
        a, out = _rows2d(a), _rows2d(out)
        # the library reads w with 16-byte loads: unit column stride, row stride a multiple of 4 floats, 16-byte aligned
        ok = w.stride(1) == 1 and w.stride(0) % 4 == 0 and w.data_ptr() % 16 == 0
        w = _rows2d(w if ok else w.clone(memory_format=torch.contiguous_format))
        keep.append(w)
        if a.shape != (n, w.shape[0]) or out.shape != (n, w.shape[1]):
            raise ValueError('dense_batch: shapes %s @ %s -> %s' % (tuple(a.shape), tuple(w.shape), tuple(out.shape)))
        g_ptr, g_ld = None, 0
        if gate is not None:
            gate = _rows2d(gate)
            if gate.shape != out.shape:
                raise ValueError('dense_batch: gate %s for output %s' % (tuple(gate.shape), tuple(out.shape)))
            g_ptr, g_ld = gate.data_ptr(), gate.stride(0)
        jobs[q] = _lib.DenseJob(a.data_ptr(), a.stride(0), w.shape[0], w.data_ptr(), w.stride(0), w.shape[1],
                                out.data_ptr(), out.stride(0), g_ptr, g_ld)
    if route is not None:
        route += _lib.dense_route(n if rows is None else rows.numel(), rows is not None, jobs)
    if rows is not None:
        _lib.check(lib.pea_dense_batch_rows(rows.numel(), _lib.ptr(rows), len(triples_), jobs, _lib.current_stream()))
    else:
        _lib.check(lib.pea_dense_batch(n, len(triples_), jobs, _lib.current_stream()))


def _mlp2_workspace(name, n_chans, emb, hid, out, device):
    need = int(_lib.load().pea_mlp2_backward_data_workspace_bytes(n_chans, int(emb), int(hid), int(out)))
    if need == 0:
        raise ValueError('%s: unsupported widths (%d, %d, %d)' % (name, emb, hid, out))
    return _workspace('mlp2_backward_data', device, need)


def mlp2_backward_data(chans, emb, hid, out, dt1, h, dz, da, rows=None, weights_in_out=False):
    """Both products of the first layer's backward data path in one launch (csrc/mlp2_bwd.hip): for every channel
    (w0 [hid, emb], w1 [out, hid], dt1_col, h_col, dz_col, da_col) of `chans`:  dz = (dt1 . w1) where h > 0 else 0;
    da = dz . w0.  dt1, h, dz, da: float32 [N, ld] views of the training workspace.  rows (RowSet): the listed rows only."""
    lib = _lib.require_device()
    n = dt1.shape[0]
    arr = (_lib.Mlp2BwdChan * len(chans))()
    keep = []
    for q, (w0, w1, c1, ch, cz, ca) in enumerate(chans):
        w0, w1 = (t.detach() if t.is_contiguous() else t.detach().contiguous() for t in (w0, w1))
        keep += [w0, w1]
        arr[q] = _lib.Mlp2BwdChan(w0.data_ptr(), w1.data_ptr(), int(c1), int(ch), int(cz), int(ca))
    ws = _mlp2_workspace('mlp2_backward_data', len(chans), emb, hid, out, dt1.device)
    _lib.check(lib.pea_mlp2_backward_data(n, len(chans), arr, int(emb), int(hid), int(out), _lib.ptr(dt1), dt1.stride(0),
                                          _lib.ptr(h), h.stride(0), _lib.ptr(dz), dz.stride(0), _lib.ptr(da), da.stride(0),
                                          None if rows is None else _lib.ptr(rows.ids), None if rows is None else _lib.ptr(rows.count),
                                          1 if weights_in_out else 0, _lib.ptr(ws), ws.numel(), _lib.current_stream()))


def mlp2_backward_data_sage(chans, emb, hid, out, dt1, dr1, h, dz, dm, dxr, rows=None):
    """SAGE form of mlp2_backward_data (pea_mlp2_backward_data_sage): per channel (w_rel0 [hid, emb], w_root0, w_rel1 [out, hid],
    w_root1, dt1_col, dr1_col, h_col, dz_col, dm_col, dxr_col):  dz = (dt1 . w_rel1 + dr1 . w_root1) where h > 0 else 0;
    dm = dz . w_rel0;  dxr = dz . w_root0."""
    lib = _lib.require_device()
    n = dt1.shape[0]
    arr = (_lib.Mlp2BwdChan * len(chans))()
    arr_s = (_lib.Mlp2BwdChanSage * len(chans))()
    keep = []
    for q, (w0, w0r, w1, w1r, c1, cr, ch, cz, cm, cx) in enumerate(chans):
        ws_ = [t.detach() if t.is_contiguous() else t.detach().contiguous() for t in (w0, w0r, w1, w1r)]
        keep += ws_
        arr[q] = _lib.Mlp2BwdChan(ws_[0].data_ptr(), ws_[2].data_ptr(), int(c1), int(ch), int(cz), int(cm))
        arr_s[q] = _lib.Mlp2BwdChanSage(ws_[1].data_ptr(), ws_[3].data_ptr(), int(cr), int(cx))
    ws = _mlp2_workspace('mlp2_backward_data_sage', len(chans), emb, hid, out, dt1.device)
    _lib.check(lib.pea_mlp2_backward_data_sage(n, len(chans), arr, arr_s, int(emb), int(hid), int(out), _lib.ptr(dt1), dt1.stride(0),
                                               _lib.ptr(dr1), dr1.stride(0), _lib.ptr(h), h.stride(0), _lib.ptr(dz), dz.stride(0),
                                               _lib.ptr(dm), dm.stride(0), _lib.ptr(dxr), dxr.stride(0),
                                               None if rows is None else _lib.ptr(rows.ids),
                                               None if rows is None else _lib.ptr(rows.count), _lib.ptr(ws), ws.numel(),
                                               _lib.current_stream()))


def block_sum(src, n_blocks, width):
    """[N, width] = sum of the n_blocks side-by-side column blocks of src [N, >= n_blocks * width] (fixed order)."""
    lib = _lib.require_device()
    src = _rows2d(src)
    out = torch.empty((src.shape[0], width), dtype=torch.float32, device=src.device)
    _lib.check(lib.pea_block_sum(src.shape[0], int(n_blocks), int(width), _lib.ptr(src), src.stride(0), _lib.ptr(out), out.stride(0),
                                 _lib.current_stream()))
    return out
