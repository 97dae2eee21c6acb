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
