"""NFM (reference graph_recsys_benchmark/models/nfm.py, driven by experiments/nfm_solver_bce.py): the neural factorisation
machine over the pair (user, item), the one reference model on MFRecsysModel.

The reference wraps torchfm.model.nfm.NeuralFactorizationMachineModel.  torchfm is not a dependency here: the module tree
below is [recalled] from pytorch-fm 0.7 (torchfm.layer, torchfm.model.nfm) with its attribute names, so that state_dict()
carries the reference's keys (emb.embedding.embedding.weight, emb.linear.fc.weight, emb.linear.bias, emb.fm.1.*,
emb.mlp.mlp.0.*, emb.mlp.mlp.1.*, emb.mlp.mlp.4.*) and a reference checkpoint loads.  What the reference's own file decides
-- the id concatenation, the MSE-on-sigmoid loss, its eval branch -- is pinned by tests/golden/nfm_small.npz.

    c = 0.5 ((e_u + e_i)^2 - (e_u^2 + e_i^2))     a = Dropout(BN1(c))     r = Dropout(relu(BN2(a W1^T + b1)))
    y = lin[u] + lin[U + i] + bias0 + r w2^T + b2     pred = sigmoid(y)     loss = mean((pred - label)^2)

forward / predict / loss take LOCAL ids (uid in [0, num_users), iid in [0, num_items)), as the reference's solver passes them,
and are the torch composition everywhere.  On the GPU, for a shape engine.nfm_supported takes:
  * native_train=True routes a training-mode loss() through csrc/nfm.hip (engine.nfm_mse_loss: forward, loss and the whole
    backward); the dropout masks are drawn on the device from torch's generator and handed to the kernel.  Off by default:
    those masks are not F.dropout's stream, so a seeded run differs from the composition's (as native_train of the KG models);
  * native=True (the default): eval() folds the two batch normalisations into the first linear layer once (engine.nfm_fold)
    and predict in eval mode, rank_eval, rank_full and recommend run on the MFMA pair scorer (engine.nfm_*).
On the CPU, or for a shape the kernels refuse, the same fold is built in torch.  rank_eval, rank_full and recommend take NODE
ids and subtract acc_uids / acc_iids: solvers.metrics, metrics_full and metrics_full_multi accept the model through the hooks
they look for, rank_full_multi among them (one catalogue scan for users with several held-out positives).
  * fused_scan=True (the default): where the HIP scorer runs and engine.nfm_scan_supported takes the widths and k, recommend,
    rank_full and rank_full_multi are ONE fused pass over the catalogue each (csrc/nfm_scan.hip, include/peahip_fm_eval.h):
    the [users, items] logit matrix is never written, and a pair's logit has the bits of the pair scorer, so the lists and
    integers are the composition's.
  * otherwise (fused_scan=False, the CPU, a refused shape, k > 128) they are the compositions of evaluators.py, the yardstick
    the fused route is tested and measured against: the scorer's item-range form per USER_CHUNK users, then a comparison or a
    stable sort."""
import numpy as np
import torch

from .. import engine as _engine, evaluators
from .base import MFRecsysModel


# ---------------------------------------------------------------- torchfm's modules, [recalled] from pytorch-fm 0.7
class _FeaturesEmbedding(torch.nn.Module):
    def __init__(self, field_dims, embed_dim):
        super().__init__()
        self.embedding = torch.nn.Embedding(sum(field_dims), embed_dim)
        self.offsets = np.array((0, *np.cumsum(field_dims)[:-1]), dtype=np.int64)
        torch.nn.init.xavier_uniform_(self.embedding.weight.data)

    def forward(self, x):
        x = x + x.new_tensor(self.offsets).unsqueeze(0)
        return self.embedding(x)


class _FeaturesLinear(torch.nn.Module):
    def __init__(self, field_dims, output_dim=1):
        super().__init__()
        self.fc = torch.nn.Embedding(sum(field_dims), output_dim)
        self.bias = torch.nn.Parameter(torch.zeros((output_dim,)))
        self.offsets = np.array((0, *np.cumsum(field_dims)[:-1]), dtype=np.int64)

    def forward(self, x):
        x = x + x.new_tensor(self.offsets).unsqueeze(0)
        return torch.sum(self.fc(x), dim=1) + self.bias


class _FactorizationMachine(torch.nn.Module):
    def __init__(self, reduce_sum=True):
        super().__init__()
        self.reduce_sum = reduce_sum

    def forward(self, x):
        square_of_sum = torch.sum(x, dim=1) ** 2
        sum_of_square = torch.sum(x ** 2, dim=1)
        ix = square_of_sum - sum_of_square
        if self.reduce_sum:
            ix = torch.sum(ix, dim=1, keepdim=True)
        return 0.5 * ix


class _MultiLayerPerceptron(torch.nn.Module):
    def __init__(self, input_dim, embed_dims, dropout, output_layer=True):
        super().__init__()
        layers = []
        for embed_dim in embed_dims:
            layers.append(torch.nn.Linear(input_dim, embed_dim))
            layers.append(torch.nn.BatchNorm1d(embed_dim))
            layers.append(torch.nn.ReLU())
            layers.append(torch.nn.Dropout(p=dropout))
            input_dim = embed_dim
        if output_layer:
            layers.append(torch.nn.Linear(input_dim, 1))
        self.mlp = torch.nn.Sequential(*layers)

    def forward(self, x):
        return self.mlp(x)


class _NeuralFactorizationMachineModel(torch.nn.Module):
    def __init__(self, field_dims, embed_dim, mlp_dims, dropouts):
        super().__init__()
        self.embedding = _FeaturesEmbedding(field_dims, embed_dim)
        self.linear = _FeaturesLinear(field_dims)
        self.fm = torch.nn.Sequential(_FactorizationMachine(reduce_sum=False), torch.nn.BatchNorm1d(embed_dim),
                                      torch.nn.Dropout(dropouts[0]))
        self.mlp = _MultiLayerPerceptron(embed_dim, mlp_dims, dropouts[1])

    def forward(self, x):
        cross_term = self.fm(self.embedding(x))
        x = self.linear(x) + self.mlp(cross_term)
        return torch.sigmoid(x.squeeze(1))


class NFMRecsysModel(MFRecsysModel):
    USER_CHUNK = 256          # users per launch of the item-range form in the compositions: a [256, items] logit block
    POS_CHUNK = 1024          # positives compared at once in the composition of rank_full_multi: a [1024, items] block

    def _init(self, **kwargs):
        self.num_users, self.num_items = int(kwargs['num_users']), int(kwargs['num_items'])
        self.emb_dim, self.hidden_size = int(kwargs['emb_dim']), int(kwargs['hidden_size'])
        self.dropout = float(kwargs['dropout'])
        self.acc_uids, self.acc_iids = int(kwargs.get('acc_uids', 0)), int(kwargs.get('acc_iids', 0))
        self.native = bool(kwargs.get('native', True))
        self.native_train = bool(kwargs.get('native_train', False))
        self.fused_scan = bool(kwargs.get('fused_scan', True))
        self.emb = _NeuralFactorizationMachineModel([self.num_users, self.num_items], self.emb_dim, (self.hidden_size,),
                                                    [self.dropout, self.dropout])
        self.folded = None            # engine.NfmFolded of the last eval()
        self.cached_repr = None       # the folded first layer [H, E]: what solvers.metrics* read the device from

    def reset_parameters(self):
        pass

    def shard(self, rank, world, tile=256):
        raise NotImplementedError('NFM is single-GPU: sharding across ranks is not implemented')

    # ------------------------------------------------------------------ the reference's composition
    def forward(self, uid, iid):
        user_item_pair_t = torch.cat([uid.view(-1, 1), iid.view(-1, 1)], dim=1)
        return self.emb(user_item_pair_t)

    def _parts(self):
        """The parameter tensors in the order engine.nfm_* take them: emb, lin, bias0, bn1, w1, b1, bn2, w2, b2"""
        e, bn1, mlp = self.emb, self.emb.fm[1], self.emb.mlp.mlp
        bn2 = mlp[1]
        return (e.embedding.embedding.weight, e.linear.fc.weight, e.linear.bias,
                (bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var), mlp[0].weight, mlp[0].bias,
                (bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var), mlp[4].weight, mlp[4].bias)

    def _bns(self):
        return self.emb.fm[1], self.emb.mlp.mlp[1]

    def _on_gpu(self):
        return self.emb.embedding.embedding.weight.is_cuda

    def _native_ok(self, batch_size=2):
        bn1, bn2 = self._bns()
        return (self.native and self._on_gpu() and self.emb.embedding.embedding.weight.dtype == torch.float32 and
                bn1.eps == bn2.eps and bn1.track_running_stats and bn2.track_running_stats and bn1.affine and bn2.affine and
                _engine.nfm_supported(self.emb_dim, self.hidden_size, batch_size))

    def predict(self, unids, inids):
        # training mode is where gradients are needed: the composition.  Eval mode scores the folded weights (no grad)
        if self.training or self.folded is None or not self.folded.device.type == 'cuda' or not self._native_ok():
            return self.forward(unids, inids)
        return _engine.nfm_predict(self.folded, unids, inids)

    def loss(self, pos_neg_pair_t):
        batch = pos_neg_pair_t
        if self.training:
            bn1, bn2 = self._bns()
            b = batch.shape[0]
            if (self.native_train and self.dropout < 1.0 and bn1.momentum is not None and bn1.momentum == bn2.momentum and
                    self._native_ok(b)):
                uid, iid, label = batch[:, 0].long(), batch[:, 1].long(), batch[:, -1].float()
                keep, scale = None, 1.0
                if self.dropout > 0.0:
                    dev = uid.device
                    keep = (torch.rand((b, self.emb_dim), device=dev) >= self.dropout,
                            torch.rand((b, self.hidden_size), device=dev) >= self.dropout)
                    scale = 1.0 / (1.0 - self.dropout)
                parts = self._parts()
                out = _engine.nfm_mse_loss(*parts, self.num_users, uid, iid, label, keep=keep, keep_scale=scale, eps=bn1.eps,
                                           momentum=bn1.momentum)
                bn1.num_batches_tracked += 1
                bn2.num_batches_tracked += 1
                return out
            pred = self.predict(batch[:, 0], batch[:, 1])
            label = batch[:, -1].float()
        else:
            pred, label = evaluators.eval_pairs(self.predict, batch)
        return torch.nn.MSELoss()(pred, label)

    # ------------------------------------------------------------------ eval mode: the fold and the scorer
    def train(self, mode=True):
        if mode:
            self.folded = self.cached_repr = None      # the fold describes the parameters of the moment it was made
        return super().train(mode)

    def eval(self):
        self.train(False)
        with torch.no_grad():
            parts = self._parts()
            eps = self._bns()[0].eps
            if self._native_ok():
                _engine.check_pending_errors()       # a bad batch of the epoch raises here at the latest (IndexError)
                self.folded = _engine.nfm_fold(*parts, self.num_users, eps=eps)
            else:
                self.folded = _engine.nfm_fold_torch(*parts, self.num_users, eps=eps)
            self.cached_repr = self.folded.w
        return self

    def _require_fold(self, what):
        if self.training or self.folded is None:
            raise RuntimeError('%s reads the eval-mode fold: call model.eval() first' % what)

    def _hip_scorer(self):
        return self.folded.device.type == 'cuda' and self._native_ok()

    def _fused(self, k=0):
        """whether a catalogue call keeping k items per user (0: the rank forms) takes the fused scan"""
        return self.fused_scan and self._hip_scorer() and _engine.nfm_scan_supported(self.emb_dim, self.hidden_size, k)

    @staticmethod
    def _on(exclude, dev):
        return None if exclude is None else tuple(t.to(dev) for t in exclude)

    def _logits_torch(self, uid, iid):
        """y of local ids uid [..] x iid [..] (broadcast against each other) over the fold, in torch"""
        f = self.folded
        x = f.emb[uid] * f.emb[f.num_users + iid]
        z = torch.relu(x @ f.w.t() + f.b)
        return ((f.lin[uid] + f.lin[f.num_users + iid]) + f.bias) + z @ f.w2

    def _block(self, uid, lo, n):
        """logits [U', n] of the local users uid against the local items lo .. lo + n - 1"""
        if self._hip_scorer():
            return _engine.nfm_score_block(self.folded, uid, lo, n)
        items = torch.arange(lo, lo + n, device=uid.device)
        return self._logits_torch(uid.view(-1, 1), items.view(1, -1))

    def _callbacks(self, unids, lo, hi):
        """what evaluators' compositions ask of this model: (block, pairs) over the requested NODE users unids and the catalogue
        [lo, hi) -- the scorer's item-range form on a slice of the users, and the logits of (user row, item NODE id) pairs"""
        def block(r0, r1):
            return self._block(unids[r0:r1] - self.acc_uids, lo - self.acc_iids, hi - lo)

        def pairs(rows, items):
            uid, iid = unids[rows] - self.acc_uids, items - self.acc_iids
            if self._hip_scorer():
                return _engine.nfm_predict(self.folded, uid, iid, logits=True)[0]
            return self._logits_torch(uid, iid)
        return block, pairs

    def rank_eval(self, unids, cand):
        """engine.dot_rank_eval's contract for this model, on NODE ids (cand [U, C], column 0 the held-out positive): (pred
        [U, C], rank of the positive int32 [U], auc [U], eval loss [U]).  rank and auc compare the logits (pred orders alike
        until the sigmoid saturates); the loss is the reference's eval-branch MSE recomputed from pred (models/nfm.py:27-32).
        What solvers.metrics calls."""
        self._require_fold('rank_eval()')
        with torch.no_grad():
            uid, items = unids.to(torch.int64) - self.acc_uids, cand.to(torch.int64) - self.acc_iids
            if self._hip_scorer():
                _, pred, rank, auc = _engine.nfm_rank_eval(self.folded, uid, items)
            else:
                y = self._logits_torch(uid.view(-1, 1), items)
                pred = torch.sigmoid(y)
                rank, auc = evaluators.candidate_ranks(y)
            return pred, rank, auc, evaluators.leave_one_out_loss(pred, 'mse')

    def rank_full(self, unids, pos_items, item_range, exclude=None):
        """engine.rank_full's contract for this model, on NODE ids: per user the rank of the held-out positive among the items of
        item_range that are neither excluded nor the positive itself (those whose logit is strictly higher), the share of them
        strictly lower, and the positive's logit.  One fused scan (engine.nfm_rank_full) where _fused() holds; else a
        composition: the scorer's range form per USER_CHUNK users, then a comparison.  What solvers.metrics_full calls."""
        self._require_fold('rank_full()')
        lo, hi = int(item_range[0]), int(item_range[1])
        with torch.no_grad():
            dev = self.folded.device
            unids, pos_items = unids.to(dev).to(torch.int64), pos_items.to(dev).to(torch.int64)
            if self._fused():
                return _engine.nfm_rank_full(self.folded, unids - self.acc_uids, pos_items, lo - self.acc_iids, hi - lo,
                                             item_node0=self.acc_iids, exclude=self._on(exclude, dev))
            return evaluators.rank_full(*self._callbacks(unids, lo, hi), pos_items, (lo, hi), exclude, self.USER_CHUNK)

    def recommend(self, unids, k, item_range, exclude=None):
        """GraphRecsysModel.recommend's contract on NODE ids: the k best items of item_range for every user, ordered by (logit
        descending, node id ascending), exclude = (rowptr, items) left out; (items int64 [U, k], logits [U, k]) with a
        (-1, -inf) tail where fewer than k items are eligible.  One fused scan (engine.nfm_recommend_topk) where _fused(k)
        holds; else a composition: the scorer's range form per USER_CHUNK users, then a stable sort."""
        self._require_fold('recommend()')
        lo, hi = int(item_range[0]), int(item_range[1])
        with torch.no_grad():
            dev = self.folded.device
            unids = torch.as_tensor(unids, device=dev).to(torch.int64)
            if 1 <= int(k) <= 128 and self._fused(int(k)):
                return _engine.nfm_recommend_topk(self.folded, unids - self.acc_uids, int(k), lo - self.acc_iids, hi - lo,
                                                  item_node0=self.acc_iids, exclude=self._on(exclude, dev))
            block, _ = self._callbacks(unids, lo, hi)
            return evaluators.recommend(block, unids.numel(), k, (lo, hi), exclude, self.USER_CHUNK, device=dev)

    def rank_full_multi(self, unids, pos_rowptr, pos_items, item_range, exclude=None):
        """engine.rank_full_multi's contract for this model, on NODE ids: the positives are a CSR (pos_rowptr [U + 1], pos_items
        [Q], every row strictly ascending); a user's negatives are the items of item_range in neither its exclusion row nor its
        positive row.  Returns, in the flat order of pos_items, (above int32 [Q] = negatives whose logit is strictly higher,
        below int32 [Q] = strictly lower, pos_score [Q]) and n_neg int32 [U].  One fused scan (engine.nfm_rank_full_multi)
        where _fused() holds; else the scorer's range form per USER_CHUNK users and a comparison per POS_CHUNK positives.  What
        solvers.metrics_full_multi calls."""
        self._require_fold('rank_full_multi()')
        lo, hi = int(item_range[0]), int(item_range[1])
        with torch.no_grad():
            dev = self.folded.device
            unids = torch.as_tensor(unids, device=dev).to(torch.int64)
            pos_rowptr, pos_items = pos_rowptr.to(dev).to(torch.int64), pos_items.to(dev).to(torch.int64)
            if self._fused():
                return _engine.nfm_rank_full_multi(self.folded, unids - self.acc_uids, pos_rowptr, pos_items, lo - self.acc_iids,
                                                   hi - lo, item_node0=self.acc_iids, exclude=self._on(exclude, dev))
            return evaluators.rank_full_multi(*self._callbacks(unids, lo, hi), pos_rowptr, pos_items, (lo, hi), exclude,
                                              self.USER_CHUNK, self.POS_CHUNK)
