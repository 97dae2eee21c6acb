"""Writes tests/golden/nfm_small.npz from the REFERENCE's NFM model (graph_recsys_benchmark/models/nfm.py), run on the CPU on
top of the restated torchfm of tests/nfm_ref.py (install_torchfm: torchfm itself is not installed; the restatement is
[recalled], the reference's file above it is the real one).  Run on the authoring machine only, from the repository root, with
the reference checkout where oracle/make_golden.py expects it:

    python tests/make_nfm_golden.py

60 users, 90 items, emb_dim 20, hidden_size 24, dropout 0, B = 37 labelled pairs of local ids; the parameters are the parity
tests' values (tests/nfm_ref.py: make_inputs) loaded into the reference model's state dict.  The file holds numbers only: the
inputs, the state dict before ('sd.<name>') and after ('sd1.<name>') one training-mode forward, pred, the loss and every
parameter's .grad ('grad.<name>') of that forward, the eval-mode predict of the same pairs, and the eval-branch loss of a
(u, pos, neg...) block.  The archive is written with fixed member timestamps, so a rerun gives the same bytes."""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import nfm_ref                                                      # noqa: E402
from oracle.make_golden import load_reference_models                # noqa: E402

N_USER, N_ITEM, E, H, B, N_NEG = 60, 90, 20, 24, 37, 12


def write_npz(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    load_reference_models()
    nfm_ref.install_torchfm()
    ref = importlib.import_module('graph_recsys_benchmark.models.nfm')
    inp = nfm_ref.make_inputs(E, H, B, seed=21, U=N_USER, I=N_ITEM, user_pool=20)
    torch.manual_seed(0)
    model = ref.NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=E, hidden_size=H, dropout=0)
    nfm_ref.load_model(model, inp)
    out = {'uid': inp['uid'].numpy(), 'iid': inp['iid'].numpy(), 'label': inp['label'].numpy().astype(np.int64)}
    for name, t in model.state_dict().items():
        out['sd.' + name] = t.detach().numpy().copy()
    model.train()
    batch = torch.stack([inp['uid'], inp['iid'], inp['label'].long()], dim=1)
    # pred comes from a second instance: the reference's loss() runs the forward itself, and the recorded state dict is the one
    # after exactly ONE training-mode forward
    twin = nfm_ref.load_model(ref.NFMRecsysModel(num_users=N_USER, num_items=N_ITEM, emb_dim=E, hidden_size=H, dropout=0), inp)
    pred = twin.train().predict(batch[:, 0], batch[:, 1])
    loss = model.loss(batch)
    loss.backward()
    out['pred'], out['loss'] = pred.detach().numpy(), loss.detach().numpy()
    for name, t in model.state_dict().items():
        out['sd1.' + name] = t.detach().numpy().copy()
    for name, t in model.named_parameters():
        out['grad.' + name] = t.grad.numpy().copy()
    model.eval()
    with torch.no_grad():
        out['eval_pred'] = model.predict(batch[:, 0], batch[:, 1]).numpy()
        g = torch.Generator().manual_seed(5)
        block = torch.cat([torch.full((N_NEG, 1), 7), torch.full((N_NEG, 1), 33), torch.randint(0, N_ITEM, (N_NEG, 1), generator=g)],
                          dim=1)
        out['eval_block'], out['eval_loss'] = block.numpy(), model.loss(block).numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'nfm_small.npz')
    write_npz(path, out)
    print('%s: %d arrays, %d bytes; loss %.6f, eval loss %.6f, pred in [%.3f, %.3f]' % (
        path, len(out), os.path.getsize(path), float(loss.detach()), float(out['eval_loss']), float(pred.detach().min()), float(pred.detach().max())))


if __name__ == '__main__':
    main()
