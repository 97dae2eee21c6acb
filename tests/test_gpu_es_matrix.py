"""GPU: the edge softmax and the KGAT / KGCN attention maps (csrc/kg_attention.hip: es_rows_kernel, es_merge_kernel,
es_finish_kernel, kg_types_kernel behind nn.softmax, nn.kgat_attention_map, nn.kgcn_attention_map) on rows of known degree, at
every lane width and on every plan shape, each against float64: oracle.pyg_restatement.segment_softmax over helpers.f64_alpha.

The graph (helpers.es_graph: 2082 nodes, 17,444 edges, 40 self loops and 230 duplicated edges, all taking part) holds rows of
0, 1, 3, 4, 5, 31, 32, 33 (32 = kShortDeg = the LDS slots of a short row), 63, 64, 65, 127, 128, 129, 200, 255, 256, 257 (one trip of
a long item is (64 / G) x 4 edges: 256 for the scalar softmax, 64 ... 4 for G = 4 ... 64), 511, 512, 513 (512 = kChunk = the LDS
slots of a long item) and 1100 edges as in-degrees AND as out-degrees.  Edge types are drawn per COO edge from (-(T-1) .. T-1),
T = 37 and once T = 1, the copies of a duplicated edge differing in type and logit.

  test_plan_holds_every_row_form                 pea_plan_relation_info of the KG plan and of both softmax plans: short rows, long
                                                 items, hub rows, hub slots, max degree as helpers.es_plan_bins restates them, one
                                                 slice; PEA_CHUNK 512, 64 (hub rows of 2 ... 18 records) and 16 (69 records)
  test_softmax_forward_backward_on_every_degree  nn.softmax and its backward, index = destination and index = source, PEA_CHUNK 512 /
                                                 64, logits of spread 3, spread 30, +1e4 +- 3, -1e4 +- 30; the six launch names
  test_softmax_without_hub_rows                  PEA_CHUNK=2048: no hub row, so no merge and no finish launch
  test_softmax_masked_edges                      -inf on a third of every row of 3 edges and more: exactly 0.0 there, the rule
                                                 elsewhere, a finite backward that is 0 on masked edges; a row that is -inf
                                                 throughout comes out as zeros (the reference gives NaN)
  test_kg_maps_at_every_lane_width               both modes x emb 16, 32, 64, 128, 256 (full lanes), 4, 12, 20, 24, 36, 40, 96, 132, 160
                                                 (idle lanes) x both type tables; at emb 40 the float64 map with types in CSR-slot
                                                 order must miss the rule
  test_kg_maps_with_other_plan_shapes            one width per G x both modes on PEA_CHUNK=64, 16, 1024, 2048, PEA_SHORT_DEG=64 and two
                                                 source-sliced plans; which rows became which form is asserted from the plan info
  test_c_abi_strides_workspace_and_refusals      _lib directly: x as a column block between NaN columns, edge_type with stride 3,
                                                 and every refused call returns its error, launches nothing and writes nothing

Branches the knob cases reach (the plan assertion of each case fails when its knob is ignored):
  PEA_CHUNK=64     hub rows of 2 ... 18 records; at G = 16 a chunk of 62 edges is less than one trip
  PEA_CHUNK=16     every row above 32 edges is a hub row; 1100 edges = 69 records: es_merge_kernel's `c += kWave` loop runs twice
  PEA_SHORT_DEG=64 short rows of 33 ... 64 edges exceed kShortCap: do_item parks their scores in the global scratch
  PEA_CHUNK=1024   rows of 513 edges are DIRECT long items above the 512 LDS slots of a wave: the scratch fallback of long items;
                   1100 = 2 hub chunks of 550
  PEA_CHUNK=2048   the 1100-edge rows are direct items as well; es_rows alone
  sliced8          PEA_SLICE_MIN_EDGES=1, PEA_SLICE_BYTES = n x emb: 8 source slices; the rows of 513 and 1100 edges are cut per
                   slice (rows up to PEA_CHUNK edges stay direct items in a sliced plan): 32 chunks, one full round of 8 x 4
  sliced8_chunk256 the same with PEA_CHUNK=256: the rows of 257, 511, 512, 513 and 1100 edges are cut per slice, 72 chunks and
                   24 `slot == -2` padding items in three rounds

Rule, per edge: |hip - f64| <= 2e-5 |f64| + 1e-9; backward: 2e-5 |g64| + 1e-6 y max|g| + 1e-9 (tests/test_gpu_kg_attention.py's,
unchanged).  Every case also asserts equal bits of two calls, row sums of 1 within 1e-5 and finite outputs, and prints the used
fraction of the rule.  tests/test_es_matrix_cpu.py holds the float32 restatement of every case to half of the rule.

Measured on the MI355X, largest used fraction: KGAT 0.049 to 0.079, KGCN 0.015 to 0.134 (T = 1: at most 0.010), softmax forward
0.022 to 0.031, softmax backward 0.057 to 0.110 of its bound; an unsliced plan shape against the default plan's output: at most 0.12."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

_CACHE = {}
KNOBS = ('PEA_CHUNK', 'PEA_SHORT_DEG', 'PEA_SLICE_MIN_EDGES', 'PEA_SLICE_BYTES')
N = H.es_graph()['n']
EI = H.es_graph()['edge_index']
E = EI.shape[1]
DEG = {'dst': np.bincount(EI[1], minlength=N), 'src': np.bincount(EI[0], minlength=N)}
INFO = ('edges', 'max_degree', 'short_rows', 'long_items', 'hub_rows', 'hub_slots')
FILL = -123.25


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _set_env(monkeypatch, env):
    """The plan knobs are read when a plan is made, and a plan is cached per tensor: every environment has its own tensors (`tag`)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _edges(tag):
    return _cached(('ei', tag), lambda: torch.from_numpy(EI).cuda())


def _types(tag, n_types):
    return _cached(('ea', tag, n_types), lambda: torch.from_numpy(np.array(H.es_types(n_types))).view(-1, 1).cuda())


def _index(tag, side):
    return _cached(('idx', tag, side), lambda: torch.from_numpy(np.array(H.es_index(side))).cuda())


def _kg_inputs(emb, n_types):
    return _cached(('kg_in', emb, n_types), lambda: tuple(t.cuda() for t in H.es_kg_inputs(emb, n_types)))


def _kernel_names(step):
    """profile names (csrc/prof.hip) of the launches `step` makes"""
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    lib.pea_profile_enable(1)
    try:
        out = step()
        torch.cuda.synchronize()
    finally:
        lib.pea_profile_enable(0)
    cap = 4096
    names, cnt = C.create_string_buffer(cap * 32), C.c_int()
    lib.pea_profile_read(cap, names, None, None, C.byref(cnt))
    return out, [names.raw[i * 32:(i + 1) * 32].split(b'\0')[0].decode() for i in range(cnt.value)]


def _es_names(names):
    return [nm for nm in names if nm.startswith('es_')]


def _info(plan):
    """(the six leading fields of pea_plan_relation_info by name, slices)"""
    from graph_recsys_benchmark_amd import _lib
    info = (C.c_int64 * 9)()
    _lib.check(_lib.load().pea_plan_relation_info(plan._h, 0, info))
    return dict(zip(INFO, [int(v) for v in info[:6]])), int(info[8])


def _want(bins):
    return {k: bins[k] for k in INFO}


def _kg_plan(tag, emb, n_types):
    from graph_recsys_benchmark_amd.nn import kg_attention as KA
    return KA._kg_plan(_edges(tag), _types(tag, n_types), N, emb, n_types)


def _hip_map(mode, emb, n_types, tag):
    from graph_recsys_benchmark_amd.nn import kgat_attention_map, kgcn_attention_map
    x, proj, r = _kg_inputs(emb, n_types)
    ei, ea = _edges(tag), _types(tag, n_types)
    return kgat_attention_map(x, proj, r, ei, ea, N) if mode == 'kgat' else kgcn_attention_map(x, r, ei, ea, N)


def _check_forward(got, want, side, what):
    """the rule, finite outputs, row sums; returns the used fraction of the rule"""
    assert got.dtype == np.float32 and got.shape == (E,)
    assert np.isfinite(got).all(), what
    frac = H.es_rule_fraction(got, want)
    print('%s: %.3f of the rule' % (what, frac))
    assert frac <= 1.0, '%s: %.2f times the rule' % (what, frac)
    sums = np.zeros(N)
    np.add.at(sums, H.es_index(side), got.astype(np.float64))
    assert np.abs(sums[DEG[side] > 0] - 1).max() <= 1e-5 and not sums[DEG[side] == 0].any()
    return frac


def _run_map(mode, emb, n_types, tag, hub):
    """one map under the profile, twice: numpy float32 [E]; the es_* launches are es_rows_<mode> and, when the plan has hub rows,
    the merge and the finish launch, once each"""
    got, names = _kernel_names(lambda: _hip_map(mode, emb, n_types, tag))
    want_names = ['es_%s_%s' % (k, mode) for k in (('rows', 'merge', 'finish') if hub else ('rows',))]
    assert _es_names(names) == want_names, names
    assert got.dtype == torch.float32 and tuple(got.shape) == (E,) and not got.requires_grad
    assert torch.equal(got, _hip_map(mode, emb, n_types, tag)), 'two calls differ'
    return got.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize('chunk', [512, 64, 16], ids=['chunk512', 'chunk64', 'chunk16'])
def test_plan_holds_every_row_form(chunk, monkeypatch):
    from graph_recsys_benchmark_amd.nn import kg_attention as KA
    _set_env(monkeypatch, {} if chunk == 512 else {'PEA_CHUNK': chunk})
    tag = ('chunk', chunk)
    plans = [('kg', 'dst', _kg_plan(tag, 64, H.ES_T))]
    plans += [('softmax', side, KA._softmax_plan(_index(tag, side), N)) for side in ('dst', 'src')]
    for what, side, plan in plans:
        got, slices = _info(plan)
        bins = H.es_plan_bins(DEG[side], chunk)
        print(what, side, got, slices)
        assert got == _want(bins), (what, side)
        assert slices == 1                    # the KG plan of this small graph is below kSliceMinEdges, the softmax plan passes 0 row bytes
        assert got['edges'] == E and got['max_degree'] == 1100 and got['short_rows'] > 0 and got['hub_rows'] > 0
        per_row = sorted(-(-DEG[side][DEG[side] > max(chunk, 32)] // chunk))
        if chunk == 512:                      # 513 -> 257 + 256, 1100 -> 367 + 367 + 366: each on two rows
            assert bins['chunks'] == {513: [257, 256], 1100: [367, 367, 366]}
            assert per_row == [2, 2, 3, 3] and got['hub_slots'] == 10 and got['long_items'] > 10
        elif chunk == 64:       # 65, 127, 128 -> 2; 129 -> 3; 200, 255, 256 -> 4; 257 -> 5; 511, 512 -> 8; 513 -> 9; 1100 -> 18
            assert per_row == sorted(2 * [2, 2, 2, 3, 4, 8, 8, 9, 18] + [4, 4, 5])
            assert bins['chunks'][1100] == [62] * 17 + [46] and got['hub_slots'] == 2 * 56 + 13
        else:                   # no direct long item is left; 1100 -> 69 records of 16 (the last: 12), one more than a wave folds per trip
            assert got['long_items'] == got['hub_slots'] and bins['chunks'][1100] == [16] * 68 + [12] and max(per_row) == 69


# ---------------------------------------------------------------------------------------------- the generic softmax
def _softmax_step(logits, idx):
    from graph_recsys_benchmark_amd.nn import softmax
    s = torch.from_numpy(np.array(logits)).cuda().requires_grad_(True)
    gr = torch.from_numpy(np.array(H.es_grad_out())).cuda()

    def step():
        y = softmax(s, idx, N)
        y.backward(gr)
        return y

    y, names = _kernel_names(step)
    assert torch.equal(y.detach(), softmax(s.detach(), idx, N)), 'two calls differ'
    return y.detach().cpu().numpy(), s.grad.cpu().numpy(), names


def _check_softmax(name, side, chunk, monkeypatch):
    from graph_recsys_benchmark_amd.nn import kg_attention as KA
    _set_env(monkeypatch, {} if chunk == 512 else {'PEA_CHUNK': chunk})
    idx = _index(('chunk', chunk), side)
    got_info, slices = _info(KA._softmax_plan(idx, N))
    assert got_info == _want(H.es_plan_bins(DEG[side], chunk)) and slices == 1
    logits = H.es_masked_logits(side) if name == 'masked' else H.es_logits(name)
    y, g, names = _softmax_step(logits, idx)
    kinds = ('rows', 'merge', 'finish') if got_info['hub_rows'] > 0 else ('rows',)
    assert _es_names(names) == ['es_%s_%s' % (k, m) for m in ('softmax', 'bwd') for k in kinds], names
    y64, g64 = H.es_softmax_case(name, side)
    what = 'softmax %s index_%s chunk%d' % (name, side, chunk)
    _check_forward(y, y64, side, what)
    assert g.dtype == np.float32 and np.isfinite(g).all()
    frac = H.es_bwd_fraction(g, g64, y64, float(np.abs(H.es_grad_out()).max()))
    print('%s backward: %.3f of its bound' % (what, frac))
    assert frac <= 1.0, '%s backward: %.2f times its bound' % (what, frac)
    return y, g, got_info


@pytest.mark.parametrize('logits', list(H.ES_LOGITS))
@pytest.mark.parametrize('chunk', [512, 64], ids=['chunk512', 'chunk64'])
@pytest.mark.parametrize('side', ['dst', 'src'], ids=['index_dst', 'index_src'])
def test_softmax_forward_backward_on_every_degree(side, chunk, logits, monkeypatch):
    y, g, info = _check_softmax(logits, side, chunk, monkeypatch)
    assert info['hub_rows'] == (4 if chunk == 512 else 21)


@pytest.mark.parametrize('side', ['dst', 'src'], ids=['index_dst', 'index_src'])
def test_softmax_without_hub_rows(side, monkeypatch):
    """The other half of `merge and finish launches exactly when the plan has hub rows`: the 1100-edge rows as direct long items"""
    y, g, info = _check_softmax('spread3', side, 2048, monkeypatch)
    assert info['hub_rows'] == 0 and info['hub_slots'] == 0 and info['long_items'] == int((DEG[side] > 32).sum())


@pytest.mark.parametrize('chunk', [512, 64], ids=['chunk512', 'chunk64'])
@pytest.mark.parametrize('side', ['dst', 'src'], ids=['index_dst', 'index_src'])
def test_softmax_masked_edges(side, chunk, monkeypatch):
    """-inf is how a PyG-style softmax is masked.  Every row of 3 edges and more loses a third of its edges, its first one among them
    (the row state starts from a -inf score); the rows of 200 edges and more lose their first third, whole chunks at PEA_CHUNK=64
    (records of (kNegBig, 0) in the merge).  Measured: a row that is -inf THROUGHOUT comes out as zeros with a zero gradient,
    where the reference's -inf - (-inf) gives NaN; that is asserted as found, not against the reference."""
    from graph_recsys_benchmark_amd.nn import softmax
    y, g, info = _check_softmax('masked', side, chunk, monkeypatch)
    m = H.es_mask(side)
    assert m.sum() > E // 4 and not y[m].any() and not g[m].any()          # exactly 0.0, forward and backward
    assert (y[~m] > 0).all()
    idx = torch.tensor([0, 0, 0, 1, 1, 3], device='cuda')
    s = torch.tensor([float('-inf')] * 3 + [0.5, float('-inf'), 2.0], device='cuda', requires_grad=True)
    z = softmax(s, idx, 4)
    z.backward(torch.ones(6, device='cuda'))
    print('a row of -inf only:', z.tolist(), s.grad.tolist())
    assert z.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 1.0] and s.grad.tolist() == [0.0] * 6


# ---------------------------------------------------------------------------------------------- the KG maps
WIDTH_CASES = [(mode, emb, nt) for mode in H.ES_MODES for emb in H.ES_FULL_WIDTHS + H.ES_IDLE_WIDTHS for nt in (H.ES_T, 1)]


@pytest.mark.parametrize('mode,emb,n_types', WIDTH_CASES, ids=[H.es_case_id(*c) for c in WIDTH_CASES])
def test_kg_maps_at_every_lane_width(mode, emb, n_types, monkeypatch):
    _set_env(monkeypatch, {})
    got_info, slices = _info(_kg_plan('default', emb, n_types))
    assert got_info == _want(H.es_plan_bins(DEG['dst'])) and slices == 1 and got_info['hub_rows'] == 4
    got = _run_map(mode, emb, n_types, 'default', hub=True)
    what = H.es_case_id(mode, emb, n_types)
    _check_forward(got, H.es_kg_reference(mode, emb, n_types), 'dst', what)
    if (emb, n_types) == (40, H.ES_T):        # teeth: the same comparison against the map with types in CSR-slot order
        frac = H.es_rule_fraction(got, H.es_kg_reference(mode, emb, n_types, wrong='slot'))
        print('%s against types in slot order: %.3g times the rule' % (what, frac))
        assert frac > 10.0


SHAPES = ('chunk64', 'chunk16', 'short64', 'chunk1024', 'chunk2048', 'sliced8', 'sliced8_chunk256')
SHAPE_CASES = [(mode, emb, shape) for mode in H.ES_MODES for emb in H.ES_KNOB_WIDTHS for shape in SHAPES]


def _shape_env(shape, emb):
    sliced = {'PEA_SLICE_MIN_EDGES': 1, 'PEA_SLICE_BYTES': N * emb}      # the gather table is ~4 N emb bytes: 4 slices' worth, one phase
    return {'chunk64': {'PEA_CHUNK': 64}, 'chunk16': {'PEA_CHUNK': 16}, 'short64': {'PEA_SHORT_DEG': 64},
            'chunk1024': {'PEA_CHUNK': 1024}, 'chunk2048': {'PEA_CHUNK': 2048}, 'sliced8': sliced,
            'sliced8_chunk256': dict(sliced, PEA_CHUNK=256)}[shape]


@pytest.mark.parametrize('mode,emb,shape', SHAPE_CASES, ids=['%s-%s' % (H.es_case_id(m, w), s) for m, w, s in SHAPE_CASES])
def test_kg_maps_with_other_plan_shapes(mode, emb, shape, monkeypatch):
    deg = DEG['dst']
    _set_env(monkeypatch, {})
    default = _cached(('default_map', mode, emb), lambda: _run_map(mode, emb, H.ES_T, 'default', hub=True))
    env = _shape_env(shape, emb)
    _set_env(monkeypatch, env)
    got_info, slices = _info(_kg_plan(shape, emb, H.ES_T))
    print(shape, got_info, slices)
    chunk, short_deg = env.get('PEA_CHUNK', 512), env.get('PEA_SHORT_DEG', 32)
    if shape.startswith('sliced'):
        bins = H.es_sliced_bins(EI, N, chunk)
        assert slices == H.ES_SLICES and got_info == _want(bins)
        # the rows that were cut per slice: the plan counts them as hub rows, their per-slice chunks as hub slots, the padding
        # items of the slice-affine layout among the long items
        assert bins['sliced_degrees'] == ([513, 513, 1100, 1100] if chunk == 512 else [257, 511, 511, 512, 512, 513, 513, 1100, 1100])
        assert got_info['hub_rows'] == len(bins['sliced_degrees'])
        # 4 rows x 8 slices fill one round of 8 x 4 items exactly; 9 rows leave `slot == -2` padding items in the third round
        assert bins['pad_items'] == 0 if chunk == 512 else bins['pad_items'] > 0
        assert got_info['hub_slots'] >= 8 * sum(d >= 511 for d in bins['sliced_degrees'])
        assert got_info['long_items'] == int(((deg > 32) & (deg <= chunk)).sum()) + got_info['hub_slots'] + bins['pad_items']
    else:
        bins = H.es_plan_bins(deg, chunk, short_deg)
        assert slices == 1 and got_info == _want(bins)
        if shape == 'chunk64':
            assert got_info['hub_rows'] == 21 and bins['chunks'][1100] == [62] * 17 + [46]
        elif shape == 'chunk16':          # 69 records: the second trip of es_merge_kernel's loop
            assert len(bins['chunks'][1100]) == 69 and got_info['long_items'] == got_info['hub_slots']
        elif shape == 'short64':          # rows of 33 ... 64 edges are short rows, beyond the 32 LDS slots of a subgroup
            moved = int(((deg > 32) & (deg <= 64)).sum())
            assert moved >= 3 and got_info['short_rows'] == int((deg <= 32).sum()) + moved and got_info['hub_slots'] == 10
        elif shape == 'chunk1024':        # 513 edges: a direct long item above the 512 LDS slots; 1100 = 2 chunks of 550
            assert got_info['hub_rows'] == 2 and bins['chunks'] == {1100: [550, 550]}
            assert got_info['long_items'] == int(((deg > 32) & (deg <= 512)).sum()) + 2 + 4
        else:                             # chunk2048: nothing but short rows and direct long items
            assert got_info['hub_rows'] == 0 and got_info['long_items'] == int((deg > 32).sum())
    got = _run_map(mode, emb, H.ES_T, shape, hub=got_info['hub_rows'] > 0)
    what = '%s-%s' % (H.es_case_id(mode, emb), shape)
    _check_forward(got, H.es_kg_reference(mode, emb, H.ES_T), 'dst', what)
    if not shape.startswith('sliced'):    # the edges of a row keep their order: the same scores, folded in other groups
        frac = H.es_rule_fraction(got, default)
        print('%s against the default plan: %.3f of the rule, %d of %d edges with other bits' % (what, frac, int((got != default).sum()), E))
        assert frac <= 1.0


# ---------------------------------------------------------------------------------------------- the C ABI
def _raw_plan(flags, row_bytes):
    from graph_recsys_benchmark_amd import _lib
    ei = _edges('default')
    h = C.c_void_p()
    _lib.check(_lib.load().pea_plan_create(N, 1, (C.c_void_p * 1)(ei.data_ptr()), (C.c_int64 * 1)(E), flags, row_bytes, 0, 1, 256,
                                           _lib.current_stream(), C.byref(h)))
    return h


@pytest.mark.parametrize('emb', [40, 132], ids=['G16-idle-emb40', 'G64-idle-emb132'])
def test_c_abi_strides_workspace_and_refusals(emb, monkeypatch):
    from graph_recsys_benchmark_amd import _lib
    lib = _lib.load()
    _set_env(monkeypatch, {})
    stream = _lib.current_stream()
    T = H.ES_T
    good = _raw_plan(_lib.PLAN_EDGE_IDS, 4 * emb)
    loops = _raw_plan(_lib.PLAN_EDGE_IDS | _lib.PLAN_SELF_LOOPS, 4 * emb)
    no_ids = _raw_plan(0, 4 * emb)
    try:
        # ---- pea_kg_edge_types: stride 1 and stride 3 give the types in CSR-slot order; +-(T-1) pass, +-T do not
        t = torch.from_numpy(np.array(H.es_types(T))).cuda()
        assert bool((t == T - 1).any()) and bool((t == -(T - 1)).any()) and bool((t == 0).any())
        wide = torch.full((E, 3), 10 ** 6, dtype=torch.int64, device='cuda')           # a column beside the types is out of range
        wide[:, 0] = t
        types = torch.full((E,), -99, dtype=torch.int32, device='cuda')
        types3 = torch.full((E,), -99, dtype=torch.int32, device='cuda')
        assert lib.pea_kg_edge_types(good, 0, _lib.ptr(t), 1, T, _lib.ptr(types), stream) == 0
        assert lib.pea_kg_edge_types(good, 0, _lib.ptr(wide), 3, T, _lib.ptr(types3), stream) == 0, lib.pea_last_error()
        want_types = H.es_types(T)[H.es_csr_order(EI[1])].astype(np.int32)
        assert np.array_equal(types.cpu().numpy(), want_types) and torch.equal(types, types3)
        scratch_types = torch.empty_like(types)
        for bad in (T, -T):
            t2 = t.clone()
            t2[E // 2] = bad
            assert lib.pea_kg_edge_types(good, 0, _lib.ptr(t2), 1, T, _lib.ptr(scratch_types), stream) == -2       # PEA_ERR_RANGE
        for rc_want, args in ((-1, (good, 0, _lib.ptr(t), 0, T)), (-1, (good, 0, _lib.ptr(t), 1, 0)), (-1, (good, 0, None, 1, T)),
                              (-1, (loops, 0, _lib.ptr(t), 1, T)), (-1, (no_ids, 0, _lib.ptr(t), 1, T)), (-1, (good, 1, _lib.ptr(t), 1, T))):
            assert lib.pea_kg_edge_types(*args, _lib.ptr(scratch_types), stream) == rc_want, args
        assert lib.pea_kg_edge_types(good, 0, _lib.ptr(t), 1, T, None, stream) == -1

        # ---- pea_kg_attention
        x, proj, r = _kg_inputs(emb, T)
        ldx, xcol = emb + 24, 4
        xbuf = torch.full((N, ldx), float('nan'), device='cuda')                       # a column the kernels must not read is a NaN
        xbuf[:, xcol:xcol + emb] = x
        xin = xbuf[:, xcol:]
        assert xin.data_ptr() % 16 == 0 and xin.stride(0) == ldx
        for mode_name, mode in (('kgat', _lib.KG_KGAT), ('kgcn', _lib.KG_KGCN)):
            nbytes = int(lib.pea_kg_attention_workspace_bytes(good, 0, mode, emb))
            assert nbytes > 0 and lib.pea_kg_attention_workspace_bytes(None, 0, mode, emb) == 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
            out = torch.full((E,), FILL, device='cuda')
            pj = _lib.ptr(proj) if mode == _lib.KG_KGAT else None

            def call(plan=good, width=emb, xp=_lib.ptr(x), ld=emb, pr=pj, rel=_lib.ptr(r), ty=_lib.ptr(types), room=nbytes, dst=out):
                return lib.pea_kg_attention(plan, 0, mode, width, xp, ld, pr, rel, ty, _lib.ptr(dst), _lib.ptr(ws), room, stream)

            refused = [(-4, dict(room=nbytes - 1)),                                     # PEA_ERR_NOMEM: a workspace one byte short
                       (-1, dict(width=6)), (-1, dict(width=260, ld=260)),              # PEA_ERR_ARG from here on
                       (-1, dict(xp=_lib.ptr(xin), ld=ldx + 1)),                        # an odd row stride
                       (-1, dict(ld=emb - 4)),                                          # a row stride below emb
                       (-1, dict(xp=None)), (-1, dict(rel=None)), (-1, dict(ty=None)),
                       (-1, dict(plan=loops)), (-1, dict(plan=no_ids))]
            if mode == _lib.KG_KGAT:
                refused.append((-1, dict(pr=None)))
            for rc_want, kw in refused:
                rc, names = _kernel_names(lambda: call(**kw))
                assert rc == rc_want and names == [], (mode_name, kw, rc, names, lib.pea_last_error())
                assert bool((out == FILL).all()), (mode_name, kw)
            assert call(dst=None) == -1
            rc, names = _kernel_names(call)
            assert rc == 0 and _es_names(names) == ['es_%s_%s' % (k, mode_name) for k in ('rows', 'merge', 'finish')], (rc, names)
            packed = out.cpu().numpy()
            assert not (packed == FILL).any()
            _check_forward(packed, H.es_kg_reference(mode_name, emb, T), 'dst', '%s emb %d through the C ABI' % (mode_name, emb))
            # x as a column block of a wider buffer: KGCN reads ldx itself, KGAT hands it to the dense product; the same bits
            strided = torch.full((E,), FILL, device='cuda')
            rc, names = _kernel_names(lambda: call(xp=_lib.ptr(xin), ld=ldx, dst=strided))
            assert rc == 0 and 'es_rows_' + mode_name in names, (rc, names, lib.pea_last_error())
            assert np.array_equal(strided.cpu().numpy(), packed), '%s: ldx %d changes the result' % (mode_name, ldx)
            # the types handed over with stride 3 are the same table
            again = torch.full((E,), FILL, device='cuda')
            assert call(ty=_lib.ptr(types3), dst=again) == 0 and np.array_equal(again.cpu().numpy(), packed)
    finally:
        torch.cuda.synchronize()
        for h in (good, loops, no_ids):
            lib.pea_plan_destroy(h)
