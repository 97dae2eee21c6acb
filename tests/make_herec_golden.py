"""Writes tests/golden/herec_small.npz from the REFERENCE's HeRec model (graph_recsys_benchmark/models/herec.py), run on the CPU
with the loss of experiments/herec_solver_bpr.py:108-121 in training mode (MSELoss()(pred, label)).  Run on the authoring
machine only, from the repository root, with the reference checkout where oracle/make_golden.py expects it:

    python tests/make_herec_golden.py

N = 200 nodes, 60 users at 0, 90 items at 60, D = 20, M = 3, B = 37, labels in 1..5; the parameters are the parity tests' values
(tests/herec_ref.py: make_inputs) loaded into the reference model's state dict.  The file holds numbers only: the inputs, the
state dict ('sd.<name>'), pred, the loss and every parameter's .grad ('grad.<name>')."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import herec_ref                                                    # noqa: E402
from oracle.make_golden import load_reference_models                # noqa: E402

N_USER, N_ITEM, N_OTHER, D, M, B = 60, 90, 50, 20, 3, 37


def main():
    load_reference_models()
    ref = importlib.import_module('graph_recsys_benchmark.models.herec')
    inp = herec_ref.make_inputs(D, M, B, seed=11, n_user=N_USER, n_item=N_ITEM, n_other=N_OTHER, user_pool=20)
    torch.manual_seed(0)
    model = ref.HeRecRecsysModel(embeddings=inp['tables'], num_uids=N_USER, num_iids=N_ITEM, acc_uids=inp['acc_uids'],
                                 acc_iids=inp['acc_iids'], embedding_dim=D)
    herec_ref.load_model(model, inp)
    model.train()
    pred = model.predict(inp['unids'], inp['inids'])
    loss = torch.nn.MSELoss()(pred, inp['labels'].float())
    loss.backward()
    out = {'num_tables': np.int64(M), 'acc_uids': np.int64(inp['acc_uids']), 'acc_iids': np.int64(inp['acc_iids']),
           'num_nodes': np.int64(inp['num_nodes']), 'unids': inp['unids'].numpy(), 'inids': inp['inids'].numpy(),
           'labels': inp['labels'].numpy(), 'pred': pred.detach().numpy(), 'loss': loss.detach().numpy()}
    for k, t in enumerate(inp['tables']):
        out['table_%d' % k] = t.numpy()
    for name, t in model.state_dict().items():
        out['sd.' + name] = t.detach().numpy()
    for name, t in model.named_parameters():
        out['grad.' + name] = t.grad.numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'herec_small.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes; loss %.6f, |pred| median %.3f max %.3f' % (
        path, len(out), os.path.getsize(path), float(loss.detach()), float(pred.detach().abs().median()), float(pred.detach().abs().max())))


if __name__ == '__main__':
    main()
