"""engine.py is the facade of the host side: every name it defined before it was split by concern is still engine.<name>, and
none of the modules it was split into imports it back."""
import os
import re

import pytest

from graph_recsys_benchmark_amd import engine

# dir(engine) of the last commit that held everything in engine.py, without the imported modules (C, torch, _lib) and the
# dunders.  Two names are left out on purpose: _gw_ws and _m2b_ws, the two workspace caches that became dense_ops._cached_ws.
NAMES = [
    'DOT_TRAIN_MAX_BLOCKS', 'GRAPHS_ENABLED', 'GraphPlan', 'HEREC_MAX_TABLES', 'KINDS', 'PARAM_SLOTS', 'PEAEngine',
    'ROWS_SCATTER_MAX', 'RowSet', 'ShardLayout', '_BprTrainLoss', '_DotBprLoss', '_EntityReg', '_HerecLoss', '_SkipgramLoss',
    '_TransrLoss', '_block16', '_catalogue_args', '_check_scored', '_defer_error', '_dot_table', '_entity_launch',
    '_fingerprint', '_herec_args', '_int64_batch', '_pending_err', '_pending_what', '_rank_io', '_rows2d', '_scatter_dense',
    '_shard_replay_mode', '_walk_rows', '_walk_starts', 'block_sum', 'bpr_score', 'bpr_train_loss', 'bpr_train_raw',
    'bpr_train_supported', 'check_pending_errors', 'dense_batch', 'dot_bpr_loss', 'dot_bpr_supported', 'dot_bpr_train_raw',
    'dot_predict', 'dot_rank_eval', 'dot_rank_full', 'dot_recommend_topk', 'entity_reg', 'fuse_ablate', 'grad_weight',
    'herec_mse_loss', 'herec_supported', 'herec_table', 'herec_train_raw', 'metapath_walks', 'mlp2_backward_data',
    'mlp2_backward_data_sage', 'predict', 'rank_eval', 'rank_eval_multi', 'rank_full', 'recommend_topk', 'rows_scatter_sum',
    'skipgram_loss', 'skipgram_supported', 'skipgram_train_raw', 'transr_loss', 'transr_supported', 'transr_train_raw',
    'uniform_walks']

SPLIT_MODULES = ['errors', 'dense_ops', 'scoring', 'losses', 'walk_ops']


@pytest.mark.parametrize('name', NAMES)
def test_engine_still_has(name):
    assert hasattr(engine, name)


def test_engine_keeps_what_callers_set_on_it():
    """bench.py clears engine.GRAPHS_ENABLED and a test zeroes engine.ROWS_SCATTER_MAX: plain module globals of engine"""
    assert engine.GRAPHS_ENABLED is True and 'GRAPHS_ENABLED' in vars(engine)
    assert engine.ROWS_SCATTER_MAX == 16384


@pytest.mark.parametrize('module', SPLIT_MODULES + ['sharding'])
def test_module_does_not_import_engine(module):
    path = os.path.join(os.path.dirname(engine.__file__), module + '.py')
    with open(path) as f:
        source = f.read()
    hits = [line for line in source.splitlines()
            if re.search(r'from\s+\.\s+import\s+.*\bengine\b|from\s+\.engine\b|\bimport\s+.*\bengine\b|from\s+\S*\.engine\s+import', line)]
    assert not hits, hits


def test_errors_imports_nothing_of_the_package():
    path = os.path.join(os.path.dirname(engine.__file__), 'errors.py')
    with open(path) as f:
        imports = [line.strip() for line in f if re.match(r'\s*(import|from)\s', line)]
    assert imports == ['import weakref', 'import torch']
