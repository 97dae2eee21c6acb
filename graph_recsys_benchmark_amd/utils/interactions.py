"""Index bookkeeping around the full-catalogue entry points (engine.recommend_topk / rank_full): which items a user
has already interacted with, in the layout the kernels read.  Plain torch sort / unique / searchsorted on whatever
device the edges live on."""
import numpy as np
import torch


def seen_items_csr(user_item_edges, unids, item_range):
    """(rowptr int64 [U + 1], items int64) -- row q lists, strictly ascending and without duplicates, the items of the
    catalogue item_range = (lo, hi) that user unids[q] has an edge to.  user_item_edges: [2, E] array or tensor of
    (user node id, item node id), any order, duplicates allowed (the reference keeps dataset.edge_index_nps[...] as
    float64 numpy).  Users may repeat and come in any order; edges of users not requested and items outside the
    catalogue are ignored.  The result lives on the device of `unids` if that is a tensor, else on the edges' device."""
    if isinstance(user_item_edges, np.ndarray):
        user_item_edges = torch.from_numpy(np.ascontiguousarray(user_item_edges).astype(np.int64, copy=False))
    edges = user_item_edges.to(torch.int64)
    if edges.dim() != 2 or edges.shape[0] != 2:
        raise ValueError('user_item_edges must be [2, E]')
    dev = unids.device if isinstance(unids, torch.Tensor) else edges.device
    edges = edges.to(dev)
    unids = torch.as_tensor(unids, dtype=torch.int64, device=dev).reshape(-1)
    lo, hi = int(item_range[0]), int(item_range[1])
    users, items = edges[0], edges[1]
    keep = (items >= lo) & (items < hi)
    users, items = users[keep], items[keep]
    span = max(hi - lo, 1)
    keys = torch.unique(users * span + (items - lo))           # sorted by (user, item), duplicates collapsed
    key_users = torch.div(keys, span, rounding_mode='floor')
    beg = torch.searchsorted(key_users, unids, right=False)
    end = torch.searchsorted(key_users, unids, right=True)
    counts = end - beg
    rowptr = torch.zeros(unids.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rowptr[1:])
    total = int(rowptr[-1])
    row = torch.repeat_interleave(torch.arange(unids.numel(), device=dev), counts, output_size=total)
    within = torch.arange(total, device=dev) - rowptr[:-1][row]
    out = keys[beg[row] + within] % span + lo
    return rowptr, out


def positives_csr(pairs_or_lists, unids):
    """(pos_rowptr int64 [U + 1], pos_items int64 [Q]) -- row q lists, strictly ascending and without duplicates, the held-out
    positives of user unids[q]: the layout engine.rank_full_multi reads.  pairs_or_lists: a [2, E] array or tensor of (user node
    id, item node id) test edges, any order, duplicates allowed, edges of users not requested ignored; or a sequence of U lists
    of item node ids, one per entry of unids.  Users may repeat (as test edges every copy gets the user's row; as lists each
    copy has its own) and a row may be empty.  Items are not confined to any catalogue: rank_full_multi ranks a positive
    wherever it lies.  The result lives on the device of `unids` if that is a tensor, else on the edges' device (lists: CPU)."""
    dev = unids.device if isinstance(unids, torch.Tensor) else None
    as_edges = isinstance(pairs_or_lists, (np.ndarray, torch.Tensor)) and pairs_or_lists.ndim == 2 and pairs_or_lists.shape[0] == 2
    if isinstance(pairs_or_lists, (np.ndarray, torch.Tensor)) and not as_edges:
        raise ValueError('test edges must be [2, E]; per-user positives come as a sequence of lists')
    if as_edges:
        edges = pairs_or_lists
        if isinstance(edges, np.ndarray):
            edges = torch.from_numpy(np.ascontiguousarray(edges).astype(np.int64, copy=False))
        dev = edges.device if dev is None else dev
        edges = edges.to(torch.int64).to(dev)
        unids = torch.as_tensor(unids, dtype=torch.int64, device=dev).reshape(-1)
        users, items = edges[0], edges[1]
    else:
        dev = torch.device('cpu') if dev is None else dev
        unids = torch.as_tensor(unids, dtype=torch.int64, device=dev).reshape(-1)
        lists = [np.asarray(row, dtype=np.int64).reshape(-1) for row in pairs_or_lists]
        if len(lists) != unids.numel():
            raise ValueError('one list of positives per entry of unids')
        # a row of its own per entry: the "user" of an item is its position in unids
        users = torch.from_numpy(np.repeat(np.arange(len(lists), dtype=np.int64), [len(row) for row in lists])).to(dev)
        items = torch.from_numpy(np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)).to(dev)
        unids = torch.arange(len(lists), dtype=torch.int64, device=dev)
    if items.numel() and int(items.min()) < 0:
        raise ValueError('item node ids are non-negative')
    span = int(items.max()) + 1 if items.numel() else 1
    keys = torch.unique(users * span + items)                  # sorted by (user, item), duplicates collapsed
    key_users = torch.div(keys, span, rounding_mode='floor')
    beg = torch.searchsorted(key_users, unids, right=False)
    end = torch.searchsorted(key_users, unids, right=True)
    counts = end - beg
    rowptr = torch.zeros(unids.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rowptr[1:])
    total = int(rowptr[-1])
    row = torch.repeat_interleave(torch.arange(unids.numel(), device=dev), counts, output_size=total)
    within = torch.arange(total, device=dev) - rowptr[:-1][row]
    return rowptr, keys[beg[row] + within] % span
