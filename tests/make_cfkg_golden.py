"""Writes tests/golden/cfkg_small.npz from the REFERENCE's CFKG model (graph_recsys_benchmark/models/cfkg.py), run on the CPU, with
the kg_loss its driver subclass adds (experiments/cfkg_solver_bpr.py:95-106: the driver module itself pulls in the whole
experiment stack, so the twelve cited lines are restated here and act on the reference model's OWN x and r), and from the
reference's own kg_negative_sampling (datasets/movielens.py:861-877), called unbound on a small fake dataset under a fixed seed.
Run on the authoring machine only, from the repository root, with the reference checkout where oracle/make_golden.py expects it:

    python tests/make_cfkg_golden.py

N = 200 nodes, 60 users at 0, 90 items at 60, E = 20, R = 5, B = 37; the parameters are the parity tests' values
(tests/cfkg_ref.py: make_inputs) loaded into the reference model's state dict.  The file holds numbers only: the inputs, the state
dict ('sd.<name>'), predict on 37 pairs, the kg loss with every parameter's .grad ('grad.<name>'), a float64 copy of the loss
and the gradients ('f64.<name>'), and the sorted rows of the sampler with the edge arrays it was given ('kg.<name>')."""
import contextlib
import importlib
import io
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cfkg_ref                                                                             # noqa: E402
from oracle.make_golden import load_reference_models, load_reference_sampling_and_solver    # noqa: E402

N, N_USER, N_ITEM, E, R, B = 200, 60, 90, 20, 5, 37
KG_SEED = 2020


def main():
    mods = load_reference_models()
    ref = importlib.import_module('graph_recsys_benchmark.models.cfkg')
    inp = cfkg_ref.make_inputs(E, R, B, seed=11, n=N, n_user=N_USER, n_item=N_ITEM)
    ds = cfkg_ref.model_dataset(N, N_USER, inp['acc_uids'], R, inp['rating_r_idx'])
    torch.manual_seed(0)
    model = ref.CFKGRecsysModel(dataset=ds, emb_dim=E)
    assert list(model.state_dict().keys()) == ['x', 'r'] and model.rating_r_idx == inp['rating_r_idx']
    cfkg_ref.load_model(model, inp['x'], inp['r'])
    model.train()
    with torch.no_grad():
        pred = model.predict(inp['unids'], inp['inids'])
        logit = torch.sum((model.x[inp['unids']] + model.r[model.rating_r_idx]) * model.x[inp['inids']], dim=-1)
    worst = float(logit.abs().max())
    print('max |<x_u + r, x_i>| = %.4f' % worst)
    assert worst < 20, 'scale the inputs: exp must stay finite and well conditioned'
    # kg_loss, experiments/cfkg_solver_bpr.py:95-106, on the reference model's own parameters
    loss, pos, neg = cfkg_ref.kg_compose(model.x, model.r, inp['batch'])
    loss.backward()
    f64 = cfkg_ref.run(inp['x'], inp['r'], inp['batch'], torch.float64)
    out = {'num_nodes': np.int64(N), 'acc_uids': np.int64(inp['acc_uids']), 'num_uids': np.int64(N_USER),
           'acc_iids': np.int64(inp['acc_uids'] + N_USER), 'num_iids': np.int64(N_ITEM),
           'rating_r_idx': np.int64(model.rating_r_idx), 'unids': inp['unids'].numpy(), 'inids': inp['inids'].numpy(),
           'batch': inp['batch'].numpy(), 'pred': pred.numpy(), 'loss': loss.detach().numpy(), 'pos': pos.detach().numpy(),
           'neg': neg.detach().numpy(), 'f64.loss': f64['loss'].numpy(), 'f64.x': f64['dx'].numpy(), 'f64.r': f64['dr'].numpy()}
    for name, t in model.state_dict().items():
        out['sd.' + name] = t.detach().numpy()
    for name, t in model.named_parameters():
        out['grad.' + name] = t.grad.numpy()
    # the reference's own sampler on a fake dataset
    ml, _ = load_reference_sampling_and_solver(mods)
    fake = cfkg_ref.sampling_dataset()
    random.seed(KG_SEED); np.random.seed(KG_SEED); torch.manual_seed(KG_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        ml.MovieLens.kg_negative_sampling(fake)
    assert fake.train_data.dtype == torch.int64 and fake.train_data.shape[1] == 4
    out['kg.seed'] = np.int64(KG_SEED)
    out['kg.train_data_sorted'] = cfkg_ref.sorted_rows(fake.train_data.numpy())
    out['kg.train_data_length'] = np.int64(fake.train_data_length)
    out['kg.num_nodes'] = np.int64(fake.num_nodes)
    out['kg.relations'] = np.array(list(fake.edge_index_nps.keys()))
    for name, ei in fake.edge_index_nps.items():
        out['kg.edge.' + name] = ei
    path = os.path.join(ROOT, 'tests', 'golden', 'cfkg_small.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes; kg loss %.6f, pred median %.3f max %.3f, %d sampled rows' % (
        path, len(out), os.path.getsize(path), float(loss.detach()), float(pred.median()), float(pred.max()),
        fake.train_data.shape[0]))


if __name__ == '__main__':
    main()
