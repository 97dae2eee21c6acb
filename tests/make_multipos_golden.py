"""Writes tests/golden/rec_utils_multi.json from the REFERENCE's own metric functions (graph_recsys_benchmark/utils/rec_utils.py:
hit :7, ndcg :18, auc :28) on hit vectors with SEVERAL positives, which its leave-one-out splits never feed them.  Run on the
authoring machine only, from the repository root, with the reference checkout where oracle/make_golden.py expects it:

    python tests/make_multipos_golden.py

20 cases: P = 1 .. 12 positives (every count at least once) among 99 negatives, float32 scores without ties, some cases with the
positives drawn from a higher mean so that several land in the first 20 places.  The hit vector is built as reference
solvers.py:88-89 builds it (torch.sort of [pos || neg] descending, hit = index < P; the two lines are restated here, the solver
module itself pulls in the whole experiment stack).  The file holds numbers only: per case the positives' and negatives' scores,
the hit vector, and what hit(), ndcg() and auc() returned."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import load_reference_models    # noqa: E402

N_NEG, SEED = 99, 1312
COUNTS = list(range(1, 13)) + [2, 3, 5, 7, 9, 11, 12, 4]


def main():
    ru = load_reference_models()['rec_utils']      # with the np.int alias utils/rec_utils.py:21 needs
    rng = np.random.default_rng(SEED)
    cases = []
    for idx, p in enumerate(COUNTS):
        while True:
            shift = (0.0, 1.0, 2.5)[idx % 3]
            pos = (rng.standard_normal(p) + shift).astype(np.float32)
            neg = rng.standard_normal(N_NEG).astype(np.float32)
            if np.unique(np.concatenate([pos, neg])).size == p + N_NEG:
                break
        _, indices = torch.sort(torch.cat([torch.from_numpy(pos), torch.from_numpy(neg)]), descending=True)
        hit_vec = (indices < p).numpy()
        cases.append({'pos': [float(v) for v in pos], 'neg': [float(v) for v in neg],
                      'hit_vec': [int(v) for v in hit_vec], 'hit': [int(v) for v in ru.hit(hit_vec)],
                      'ndcg': [float(v) for v in ru.ndcg(hit_vec)], 'auc': float(ru.auc(pos, neg))})
    path = os.path.join(ROOT, 'tests', 'golden', 'rec_utils_multi.json')
    with open(path, 'w') as f:
        json.dump({'num_neg': N_NEG, 'seed': SEED, 'ks': list(range(5, ru.NUM_RECS_RANGE + 1)), 'cases': cases}, f)
    print('%s: %d cases, %d bytes; hits in the first 20: %s' % (
        path, len(cases), os.path.getsize(path), [int(sum(c['hit_vec'][:20])) for c in cases]))


if __name__ == '__main__':
    main()
