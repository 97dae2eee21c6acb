"""MetaPath2Vec with the reference's module surface (graph_recsys_benchmark/models/metapath2vec.py), the walks and the
skip-gram loss routed to the gfx950 HIP library.

Differences, all on purpose:
  * the walks are drawn on the GPU (csrc/walk.hip) from a counter-based Philox stream instead of torch_sparse's adj.sample on
    the CPU (:55,101-121) and torch.randint (:129): reproducible from (seed, number of the sample() call), not the
    reference's stream;
  * pos_sample / neg_sample return WHOLE walks [rows, walk_length + 1]; windows(rw) cuts them into the reference's
    [rows * (walk_length + 2 - context_size), context_size] layout (:117-121), loss() takes either;
  * a node without an edge in a step's relation ends its walk with -1 (the reference's adj.sample reads the next row's slot);
    loss() skips the pairs that hold a -1 and averages over the valid pairs;
  * loss() runs forward and backward in one HIP call (csrc/skipgram.hip) that reads every table row once per walk position;
    native=False (or a shape the kernels do not take) is the torch composition of the reference's formula on the same walks;
  * the sklearn test() helper is not carried over.
"""
import torch
from torch.nn import Embedding
from torch.utils.data import DataLoader

from .. import engine as _engine

EPS = 1e-15


class MetaPath2Vec(torch.nn.Module):
    def __init__(self, edge_index_dict, embedding_dim, metapath, walk_length, context_size, num_nodes_dict, types, type_accs,
                 walks_per_node=1, num_negative_samples=1, sparse=False, native=True, seed=None):
        super().__init__()
        assert metapath[0][0] == metapath[-1][-1]
        assert walk_length >= context_size

        self.edge_index_dict = edge_index_dict           # values in GLOBAL node ids, as the reference's driver passes them
        self.embedding_dim = embedding_dim
        self.metapath = metapath
        self.walk_length = walk_length
        self.context_size = context_size
        self.walks_per_node = walks_per_node
        self.num_negative_samples = num_negative_samples
        self.num_nodes_dict = num_nodes_dict
        self.sparse = bool(sparse)
        self.native = bool(native)
        self.seed = torch.initial_seed() if seed is None else int(seed)

        count = 0
        self.start, self.end = {}, {}
        for key in types:
            self.start[key] = count
            count += num_nodes_dict[key]
            self.end[key] = count
            assert self.start[key] == type_accs[key]     # embedding row = global node id

        self.embedding = Embedding(count, embedding_dim, sparse=sparse)
        self._plan = None
        self._calls = 0                                  # sample() calls so far: call k draws from the offsets 2k and 2k + 1

        self.reset_parameters()

    def reset_parameters(self):
        self.embedding.reset_parameters()

    def forward(self, node_type, batch=None):
        """Returns the embeddings for the nodes in :obj:`batch` of type :obj:`node_type`.  Reading the table out is where a walk
        id beyond the table, flagged on the device by an earlier loss(), raises its IndexError (so does eval())."""
        _engine.check_pending_errors()
        emb = self.embedding.weight[self.start[node_type]:self.end[node_type]]
        return emb if batch is None else emb[batch]

    def train(self, mode=True):
        if not mode:
            _engine.check_pending_errors()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        """a plan lives on the device it was built on: .to() / .cuda() drop it, the next sample() builds it where the table is"""
        self._plan = None
        return super()._apply(fn, *args, **kwargs)

    def loader(self, **kwargs):
        return DataLoader(range(self.num_nodes_dict[self.metapath[0][0]]), collate_fn=self.sample, **kwargs)

    # ------------------------------------------------------------------ walks (csrc/walk.hip)
    def _get_plan(self):
        """One GraphPlan over the metapath's distinct edge types.  A plan's CSR row of a node holds the sources of its in-edges;
        the reference steps from edge_index[0] to edge_index[1] (:50-54,109), so every COO goes in flipped."""
        if self._plan is None:
            dev = self.embedding.weight.device
            flipped = [torch.flip(self.edge_index_dict[keys].to(dev), dims=[0]).contiguous() for keys in self.metapath]
            self._plan = _engine.GraphPlan(self.embedding.num_embeddings, [flipped], self_loops=False)
            self._relations = list(self._plan.relation_of[0])
        return self._plan

    def _starts(self, batch, repeat):
        if not isinstance(batch, torch.Tensor):
            batch = torch.tensor(batch)
        batch = batch.to(self.embedding.weight.device, torch.int64).reshape(-1)
        return (batch + self.start[self.metapath[0][0]]).repeat(repeat)

    def pos_sample(self, batch):
        """[len(batch) * walks_per_node, walk_length + 1] walks along the metapath, in global node ids; row r starts at
        batch[r % len(batch)] (ids local to the start type, like the reference's loader hands out)."""
        plan = self._get_plan()
        return _engine.metapath_walks(plan, self._relations, self._starts(batch, self.walks_per_node), self.walk_length,
                                      self.seed, 2 * self._calls)

    def neg_sample(self, batch):
        """[len(batch) * walks_per_node * num_negative_samples, walk_length + 1]: every step uniform over its type's nodes"""
        lo = [self.start[keys[-1]] for keys in self.metapath]
        cnt = [self.num_nodes_dict[keys[-1]] for keys in self.metapath]
        starts = self._starts(batch, self.walks_per_node * self.num_negative_samples)
        return _engine.uniform_walks(lo, cnt, starts, self.walk_length, self.seed, 2 * self._calls + 1)

    def sample(self, batch):
        if not isinstance(batch, torch.Tensor):
            batch = torch.tensor(batch)
        out = self.pos_sample(batch), self.neg_sample(batch)
        self._calls += 1
        return out

    def windows(self, rw):
        """The reference's window layout of whole walks (:117-121): [rows * (walk_length + 2 - context_size), context_size]"""
        num_walks_per_rw = 1 + self.walk_length + 1 - self.context_size
        return torch.cat([rw[:, j:j + self.context_size] for j in range(num_walks_per_rw)], dim=0)

    # ------------------------------------------------------------------ loss (csrc/skipgram.hip)
    def _native_ok(self, pos_rw, neg_rw):
        w = self.embedding.weight
        return (self.native and w.is_cuda and pos_rw.is_cuda and neg_rw.is_cuda and pos_rw.shape[1] == neg_rw.shape[1] and
                _engine.skipgram_supported(self.embedding_dim, pos_rw.shape[1], self.context_size,
                                           pos_rw.shape[0] + neg_rw.shape[0]))

    def _side_torch(self, rw, positive):
        c, n = self.context_size, self.embedding.num_embeddings
        win = rw.unfold(1, c, 1).reshape(-1, c) if rw.size(1) > c else rw
        start, rest = win[:, :1], win[:, 1:].contiguous()
        valid = ((start >= 0) & (start < n) & (rest >= 0) & (rest < n)).view(-1)
        h_start = self.embedding(start.clamp(0, n - 1))
        h_rest = self.embedding(rest.clamp(0, n - 1))
        out = (h_start * h_rest).sum(dim=-1).view(-1)
        sig = torch.sigmoid(out)
        term = -torch.log((sig if positive else 1 - sig) + EPS)
        return (term * valid).sum() / valid.sum().clamp(min=1)

    def loss(self, pos_rw, neg_rw):
        r"""Computes the loss given positive and negative random walks: whole walks, or windows(walks); any [M, T] with
        T >= context_size."""
        assert pos_rw.size(1) >= self.context_size and neg_rw.size(1) >= self.context_size
        if self._native_ok(pos_rw, neg_rw):
            return _engine.skipgram_loss(self.embedding.weight, pos_rw, neg_rw, self.context_size, sparse=self.sparse)
        return self._side_torch(pos_rw, True) + self._side_torch(neg_rw, False)

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.embedding.weight.size(0), self.embedding.weight.size(1))
