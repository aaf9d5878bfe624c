"""Device cut pursuit (csrc/spg_cutpursuit.hip) against references that share no code with it or with the restatement
(cutpursuit_cases.py): ops.min_cut against an exhaustive search over all labelings and against closed forms at the constants of
the host loop (16 pulses, 16 levels, blocks of 256, excess beyond an int); spg_cp_accumulate against Python-integer sums,
spg_cp_dist against a sequential float64 loop bit for bit, spg_cp_farthest against its definition; ops.cut_pursuit against itself
under exact power-of-two scalings, and against the restatement on scenes at the edges of its inputs and options.

Every assertion is exact (integers or bit patterns); the edge scenes against the restatement carry the assertions of
test_gpu_cutpursuit.py::test_cut_pursuit_equals_restatement as they stand there (partition, pulses and merge rounds exactly, values
and energies within its 1e-11 relative: float64 sums in another order).  Pulse counts come from the
restatement (test_cutpursuit_cases.py pins them to the closed forms on the host)."""
import numpy as np
import pytest
import torch

import cutpursuit_cases as CASES
import cutpursuit_restatement as R
from superpoint_graph_amd import ops

pytestmark = pytest.mark.gpu

GRAPH_KEYS = ('n', 'src', 'tgt', 'cap', 'cost0', 'cost1')
SOLVER = CASES.solver_cases()
EDGE_SCENES = CASES.edge_solver_cases()
_PLAIN = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _min_cut(c, **kw):
    g = ops.EdgeGraph(dev(c['src']), dev(c['tgt']), c['n'])
    label, info = ops.min_cut(g, dev(c['cap']), dev(c['cost0']), dev(c['cost1']), return_info=True, **kw)
    assert label.dtype == torch.uint8 and label.shape == (c['n'],)
    return label.cpu().numpy(), info


def _check(c, pulses=None, **kw):
    """the device's min cut of a case that carries its own 'label' and 'value'; pulses: the count to expect, default the restatement's"""
    label, info = _min_cut(c, **kw)
    assert np.array_equal(label, c['label'])
    assert R.cut_value(label, c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1']) == c['value']
    assert info['pulses'] == (R.min_cut(*(c[k] for k in GRAPH_KEYS))[1] if pulses is None else pulses)
    return info


# ---- A. the exhaustive oracle ----
def test_min_cut_of_the_union_equals_the_exhaustive_oracle():
    graphs = CASES.oracle_graphs()
    u = CASES.disjoint_union(graphs)
    label, info = _min_cut(u)
    wrong = [i for i, g in enumerate(graphs) if not np.array_equal(label[u['offsets'][i]:u['offsets'][i + 1]], g['label'])]
    assert not wrong, f'graphs {wrong} of the union differ from the oracle'
    assert R.cut_value(label, u['src'], u['tgt'], u['cap'], u['cost0'], u['cost1']) == u['value']
    assert info['pulses'] == R.min_cut(*(u[k] for k in GRAPH_KEYS))[1]


@pytest.mark.parametrize('i', CASES.ORACLE_ONE_BY_ONE)
def test_min_cut_equals_the_exhaustive_oracle(i):
    _check(CASES.oracle_graphs()[i])


# ---- B. host-loop and size edges, closed forms ----
@pytest.mark.parametrize('n', CASES.PATH_NS)
def test_through_path_takes_one_pulse_per_hop(n):
    c = CASES.path_case(n, 'through')
    _check(c, pulses=n)
    _check(c, pulses=n, max_pulses=n)
    with pytest.raises(RuntimeError, match=f'max_pulses = {n - 1} pulses'):
        _min_cut(c, max_pulses=n - 1)


@pytest.mark.parametrize('family', CASES.PATH_FAMILIES[1:])
@pytest.mark.parametrize('n', CASES.PATH_NS)
def test_path_closed_forms(n, family):
    _check(CASES.path_case(n, family))


@pytest.mark.parametrize('n', CASES.EDGELESS_NS)
def test_edgeless_closed_form(n):
    _check(CASES.edgeless_case(n))


def test_max_pulses_zero():
    for c in CASES.no_source_cases().values():
        info = _check(c, pulses=0, max_pulses=0)
        assert info['pulses'] == 0
    with pytest.raises(RuntimeError, match='max_pulses = 0 pulses'):
        _min_cut(CASES.path_case(2, 'through'), max_pulses=0)


@pytest.mark.parametrize('slack', [1, 0])
def test_double_star_excess_beyond_an_int(slack):
    _check(CASES.double_star(CASES.STAR_M - slack))


def test_union_of_the_through_paths():
    u = CASES.disjoint_union([CASES.path_case(n, 'through') for n in CASES.PATH_NS])
    _check(u)


# ---- C. the per-component entry points ----
def _rng(shape, salt):
    return np.random.default_rng([salt, CASES.CP_SHAPES.index(shape)])


def _accumulate(key, mq, q, K):
    """spg_cp_accumulate into W and S that hold garbage: the call clears them itself"""
    n, D = q.shape
    W = torch.full((K,), -0x0123456789abcdef, dtype=torch.int64, device='cuda')
    S = torch.full((K, D), 0x7edcba9876543210, dtype=torch.int64, device='cuda')
    key, mq, q = dev(key.astype(np.int32)), dev(mq.astype(np.int32)), dev(q.astype(np.int32))
    ops.check(ops.lib().spg_cp_accumulate(ops._ptr(key), ops._ptr(mq), ops._ptr(q), n, D, K, ops._ptr(W), ops._ptr(S), ops._stream()),
              'spg_cp_accumulate')
    return W.cpu().numpy(), S.cpu().numpy()


@pytest.mark.parametrize('shape', CASES.CP_SHAPES, ids=CASES.cp_shape_id)
def test_cp_accumulate_equals_integer_sums(shape):
    n, D, _, _ = shape
    rng = _rng(shape, 1)
    key, K = CASES.cp_keys(shape, rng)
    for pattern in CASES.CP_VALUE_PATTERNS:
        mq, q = CASES.cp_values(pattern, n, D, rng)
        W_w, S_w = CASES.cp_sums_ref(key, mq, q, K)
        W, S = _accumulate(key, mq, q, K)
        assert np.array_equal(W, W_w), pattern
        assert np.array_equal(S, S_w), pattern
        # the module's own wrapper is the same call
        W2, S2 = ops._cp_sums(dev(key), dev(mq.astype(np.int32)), dev(q.astype(np.int32)), K)
        assert np.array_equal(W2.cpu().numpy(), W_w) and np.array_equal(S2.cpu().numpy(), S_w), pattern


def test_cp_accumulate_forms_the_product_in_64_bits():
    lo, hi = CASES.I32_MIN, CASES.I32_MAX
    key = np.zeros(2, np.int32)
    mq = np.array([hi, hi], np.int64)
    q = np.array([[lo, hi, hi, lo], [hi, lo, hi, lo]], np.int64)
    W_w, S_w = CASES.cp_sums_ref(key, mq, q, 1)
    assert S_w.tolist() == [[hi * lo + hi * hi, hi * lo + hi * hi, 2 * hi * hi, 2 * hi * lo]] and W_w.tolist() == [2 * hi]
    W, S = _accumulate(key, mq, q, 1)
    assert np.array_equal(W, W_w) and np.array_equal(S, S_w)
    # and one vertex per lane path: the second vertex under a key of its own
    key = np.array([0, 1], np.int32)
    W_w, S_w = CASES.cp_sums_ref(key, mq, q, 2)
    W, S = _accumulate(key, mq, q, 2)
    assert np.array_equal(W, W_w) and np.array_equal(S, S_w)


def _dist(q, key, C):
    """spg_cp_dist into an out that holds NaN"""
    n, D = q.shape
    out = torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')
    q, key, C = dev(q.astype(np.int32)), dev(key.astype(np.int32)), dev(C)
    ops.check(ops.lib().spg_cp_dist(ops._ptr(q), ops._ptr(key), ops._ptr(C), n, D, int(C.shape[0]), ops._ptr(out), ops._stream()),
              'spg_cp_dist')
    return out.cpu().numpy()


@pytest.mark.parametrize('shape', CASES.CP_SHAPES, ids=CASES.cp_shape_id)
def test_cp_dist_equals_a_sequential_float64_loop_bit_for_bit(shape):
    n, D, _, _ = shape
    rng = _rng(shape, 2)
    key, K = CASES.cp_keys(shape, rng)
    mq, q = CASES.cp_values('random', n, D, rng)
    for scale in (1, 2):                                                  # |q| <= 2^20 as the solver has it, and 2^21
        C = CASES.cp_centres(key, mq, q * scale, K, rng)
        assert K * D < 8 or (C != np.rint(C)).any()
        want = CASES.cp_dist_ref(q * scale, key, C)
        got = _dist(q * scale, key, C)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), scale
        outside = (key < 0) | (key >= K)
        assert not got.view(np.int64)[outside].any()                      # exactly +0.0
        got2 = ops._cp_dist(dev((q * scale).astype(np.int32)), dev(key), dev(C)).cpu().numpy()
        assert np.array_equal(got2.view(np.int64), want.view(np.int64)), scale


def _farthest(dist, key, mq, K):
    """spg_cp_farthest into best and idx that hold garbage -> (idx, bits of best)"""
    n = len(dist)
    best = torch.full((K,), 0x7ff8dead0000beef, dtype=torch.int64, device='cuda')
    idx = torch.full((K,), -7, dtype=torch.int32, device='cuda')
    dist, key, mq = dev(dist), dev(key.astype(np.int32)), dev(mq.astype(np.int32))
    ops.check(ops.lib().spg_cp_farthest(ops._ptr(dist), ops._ptr(key), ops._ptr(mq), n, K, ops._ptr(best), ops._ptr(idx), ops._stream()),
              'spg_cp_farthest')
    return idx.cpu().numpy().astype(np.int64), best.cpu().numpy()


@pytest.mark.parametrize('shape', CASES.CP_SHAPES, ids=CASES.cp_shape_id)
def test_cp_farthest_equals_its_definition(shape):
    rng = _rng(shape, 3)
    key, K = CASES.cp_keys(shape, rng)
    for pattern in CASES.CP_FAR_PATTERNS:
        dist, mq = CASES.cp_far_inputs(pattern, key, K, rng)
        idx_w, best_w = CASES.cp_farthest_ref(dist, key, mq, K)
        idx, bits = _farthest(dist, key, mq, K)
        assert np.array_equal(idx, idx_w), pattern
        assert np.array_equal(bits, best_w.view(np.int64)), pattern
        idx2, best2 = ops._cp_farthest(dev(dist), dev(key), dev(mq.astype(np.int32)), K)
        assert np.array_equal(idx2.cpu().numpy(), idx_w) and np.array_equal(best2.cpu().numpy().view(np.int64), bits), pattern


# ---- D. exact power-of-two invariances, device against device ----
def _solve(c):
    g = ops.EdgeGraph(dev(np.asarray(c['src'], np.int64)), dev(np.asarray(c['tgt'], np.int64)), len(c['obs']))
    comp, ncom, values, energies, stats = ops.cut_pursuit(dev(c['obs']), g, dev(c['w']), None if c['m'] is None else dev(c['m']),
                                                          return_stats=True, **c['kw'])
    assert comp.dtype == torch.int32 and values.dtype == torch.float32
    return comp.cpu().numpy(), ncom, values.cpu().numpy(), energies, stats


def _plain(name):
    if name not in _PLAIN:
        _PLAIN[name] = _solve(SOLVER[name])
    return _PLAIN[name]


@pytest.mark.parametrize('variant', CASES.SCALINGS)
@pytest.mark.parametrize('name', CASES.SCALING_SCENES)
def test_cut_pursuit_follows_power_of_two_scalings_exactly(name, variant):
    comp, ncom, values, energies, stats = _plain(name)
    scaled, fv, fe = CASES.scaled_scene(SOLVER[name], variant)
    comp2, ncom2, values2, energies2, stats2 = _solve(scaled)
    assert ncom2 == ncom and np.array_equal(comp2, comp)
    assert stats2['pulses'] == stats['pulses'] and stats2['merge_rounds'] == stats['merge_rounds']
    assert np.array_equal(values2.view(np.int32), (values * np.float32(fv)).view(np.int32))
    assert energies2 == [e * fe for e in energies]


# ---- E. solver scenes at the edges of its inputs and options, against the restatement ----
@pytest.mark.parametrize('name', sorted(EDGE_SCENES))
def test_cut_pursuit_edge_scene_equals_restatement(name):
    c, stats_w = EDGE_SCENES[name], {}
    comp_w, ncom_w, values_w, energies_w = R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], c['m'], stats=stats_w, **c['kw'])
    comp, ncom, values, energies, stats = _solve(c)
    assert ncom == ncom_w and np.array_equal(comp, comp_w)
    assert stats['pulses'] == stats_w['pulses'] and stats['merge_rounds'] == stats_w['merge_rounds']
    assert values.shape == values_w.shape
    v, vw = values.astype(np.float64), values_w.astype(np.float64)
    print(name, 'ncom', ncom, 'pulses', stats['pulses'], 'energies', energies, energies_w, 'values max|d|', np.abs(v - vw).max(initial=0))
    assert np.all(np.abs(v - vw) <= 1e-11 * np.abs(vw))
    assert len(energies) == len(energies_w)
    assert all(abs(a - b) <= 1e-11 * abs(b) for a, b in zip(energies, energies_w))
    if name == 'grid_no_edges':
        assert ncom == 1                        # components are recomputed only after a new cut
    if name == 'grid_max_ite0':
        assert energies == [] and ncom == 1
