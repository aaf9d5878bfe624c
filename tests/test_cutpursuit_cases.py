"""The references of cutpursuit_cases.py that share no code with the kernels, on the host: the exhaustive min-cut oracle and the
closed forms against the restatement's min cut (labels, values, pulse counts), the power-of-two invariances of the restatement's
solver, and the self-checks of the case builders.  Everything asserted is an integer or a bit pattern."""
import numpy as np
import pytest

import cutpursuit_cases as CASES
import cutpursuit_restatement as R

GRAPH_KEYS = ('n', 'src', 'tgt', 'cap', 'cost0', 'cost1')


def _min_cut(c, **kw):
    return R.min_cut(*(c[k] for k in GRAPH_KEYS), **kw)


def _value(c, label):
    return R.cut_value(label, c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])


def _check(c, **kw):
    """the restatement's min cut of a case that carries its own 'label' and 'value' -> pulses"""
    label, pulses = _min_cut(c, **kw)
    assert label.dtype == np.uint8 and np.array_equal(label, c['label'])
    assert _value(c, label) == c['value']
    return pulses


# ---- A ----
def test_oracle_graphs_meet_their_conditions():
    graphs = CASES.oracle_graphs()
    assert len(graphs) >= 200
    assert {g['n'] for g in graphs} == set(range(1, 13))
    assert all(0 <= len(g['src']) <= 3 * g['n'] for g in graphs)
    assert 4 * sum(g['minimisers'] > 1 for g in graphs) >= len(graphs)                       # the tie share, on the oracle alone
    assert 3 * sum(bool(np.all((g['cost0'] > 0) & (g['cost1'] > 0))) for g in graphs) >= len(graphs)
    assert any((g['src'] == g['tgt']).any() for g in graphs)                                 # self-loops
    assert any(len(np.unique(np.stack([np.minimum(g['src'], g['tgt']), np.maximum(g['src'], g['tgt'])]), axis=1).T) < len(g['src'])
               for g in graphs)                                                              # parallel edges
    top = np.array([max(g['cap'].max(initial=0), g['cost0'].max(), g['cost1'].max()) for g in graphs])
    assert all(3 * (top < hi).sum() >= k * len(graphs) for k, hi in enumerate((2, 4, 1000), 1)) and (top >= 4).any()
    one = [graphs[i] for i in CASES.ORACLE_ONE_BY_ONE]
    assert 18 <= len(one) <= 24 and any(g['n'] == 1 for g in one) and any(g['n'] > 1 and len(g['src']) == 0 for g in one)
    assert 1000 <= sum(g['n'] for g in graphs) <= 2000


def test_oracle_is_right_on_graphs_done_by_hand():
    # two vertices, both minimisers {00, 11} of value 3 when the edge is dearer than either side: the one with fewer ones
    label, value, count = CASES.exhaustive_min_cut(2, [0], [1], [5], [3, 0], [0, 3])
    assert label.tolist() == [0, 0] and value == 3 and count == 2
    label, value, count = CASES.exhaustive_min_cut(2, [0], [1], [1], [3, 0], [0, 3])
    assert label.tolist() == [1, 0] and value == 1 and count == 1
    label, value, count = CASES.exhaustive_min_cut(1, [0], [0], [9], [4], [4])
    assert label.tolist() == [0] and value == 4 and count == 2


def test_restatement_min_cut_equals_the_exhaustive_oracle():
    for i, g in enumerate(CASES.oracle_graphs()):
        label, _ = _min_cut(g)
        assert np.array_equal(label, g['label']), i
        assert _value(g, label) == g['value'], i


def test_union_of_the_oracle_graphs_decomposes():
    u = CASES.disjoint_union(CASES.oracle_graphs())
    assert u['n'] == sum(g['n'] for g in CASES.oracle_graphs()) and len(u['label']) == u['n']
    assert _value(u, u['label']) == u['value']
    _check(u)


# ---- B ----
@pytest.mark.parametrize('n', CASES.PATH_NS)
def test_through_path_takes_one_pulse_per_hop(n):
    c = CASES.path_case(n, 'through')
    assert c['label'].all() and c['value'] == 5 and c['pulses'] == n
    assert _check(c) == n
    assert _check(c, max_pulses=n) == n
    with pytest.raises(RuntimeError, match=f'max_pulses = {n - 1} pulses'):
        _min_cut(c, max_pulses=n - 1)


@pytest.mark.parametrize('family', CASES.PATH_FAMILIES[1:])
@pytest.mark.parametrize('n', CASES.PATH_NS)
def test_path_closed_forms(n, family):
    c = CASES.path_case(n, family)
    if family == 'bottleneck':
        assert c['label'].tolist() == [0] * ((n - 2) // 2 + 1) + [1] * (n - 1 - (n - 2) // 2) and 0 < c['label'].sum() < n
    else:
        assert not c['label'].any()
    _check(c)


@pytest.mark.parametrize('n', CASES.EDGELESS_NS)
def test_edgeless_closed_form(n):
    c = CASES.edgeless_case(n)
    assert len(c['src']) == 0 and 0 < c['label'].sum() < n
    _check(c)


def test_no_source_needs_no_pulse():
    for c in CASES.no_source_cases().values():
        assert _check(c, max_pulses=0) == 0
    with pytest.raises(RuntimeError, match='max_pulses = 0 pulses'):
        _min_cut(CASES.path_case(2, 'through'), max_pulses=0)


@pytest.mark.parametrize('slack', [1, 0])
def test_double_star_closed_form(slack):
    M, a = CASES.STAR_M, CASES.STAR_ARMS
    assert a * M > 1 << 31                                         # the centre's excess does not fit an int
    c = CASES.double_star(M - slack)
    assert c['n'] == 1 + 2 * a and c['value'] == a * (M - slack) and c['label'].sum() == a * slack
    assert max(c['cap'].max(), c['cost0'].max(), c['cost1'].max()) < R.CAP_LIMIT
    assert _check(c) == 19


def test_union_of_the_through_paths():
    u = CASES.disjoint_union([CASES.path_case(n, 'through') for n in CASES.PATH_NS])
    assert u['label'].all() and u['value'] == 5 * len(CASES.PATH_NS)
    assert _check(u) == max(CASES.PATH_NS)


# ---- C ----
def test_cp_shapes_cover_every_axis_value():
    shapes = CASES.CP_SHAPES
    assert 20 <= len(shapes) <= 30 and len(set(shapes)) == len(shapes)
    assert {s[0] for s in shapes} == set(CASES.CP_NS)
    assert {s[1] for s in shapes} == set(CASES.CP_DS)
    assert {s[2] or 'n' for s in shapes} == set(CASES.CP_KS)
    assert {s[3] for s in shapes} == set(CASES.CP_KEY_PATTERNS)


def test_cp_inputs_have_the_properties_they_are_named_for():
    rng = np.random.default_rng(0)
    seen_cancel_to_zero = seen_negative = False
    for shape in CASES.CP_SHAPES:
        n, D, _, pattern = shape
        key, K = CASES.cp_keys(shape, rng)
        assert key.dtype == np.int32 and key.shape == (n,) and K >= 1
        inside = (key >= 0) & (key < K)
        if pattern == 'holes':
            assert key[0] == -1 and set(key.tolist()) <= {-1, K - 1}
        if pattern == 'wave_runs':
            assert all(len(set(key[i:i + 64].tolist())) == 1 for i in range(0, n, 64))
        if pattern == 'shifted_runs':
            assert all(len(set(key[i:i + 64].tolist())) == 2 for i in range(0, n - 63, 64)) or K == 1
        if pattern == 'all_minus1':
            assert (key == -1).all()
        if pattern == 'out_of_range':
            assert (key >= K).any() and ((key < -1).any() or n < 2)
        for vp in CASES.CP_VALUE_PATTERNS:
            mq, q = CASES.cp_values(vp, n, D, rng)
            assert mq.min() >= 0 and mq.max() <= 1 << 10 and np.abs(q).max(initial=0) <= 1 << 20
            W, S = CASES.cp_sums_ref(key, mq, q, K)
            # the Python-integer sums against np.int64 add.at
            W2, S2 = np.zeros(K, np.int64), np.zeros((K, D), np.int64)
            np.add.at(W2, key[inside], mq[inside])
            np.add.at(S2, key[inside], mq[inside, None] * q[inside])
            assert np.array_equal(W, W2) and np.array_equal(S, S2)
            seen_cancel_to_zero |= vp == 'cancel' and bool(((W > 0)[:, None] & (S == 0)).all()) and bool((W > 0).any()) and n >= 64
            seen_negative |= vp == 'negative' and bool((S.sum(0) < 0).all())
        for fp in CASES.CP_FAR_PATTERNS:
            dist, mq = CASES.cp_far_inputs(fp, key, K, rng)
            assert not np.signbit(dist).any() and not np.isnan(dist).any()
            idx, best = CASES.cp_farthest_ref(dist, key, mq, K)
            ok = inside & (mq > 0)
            for k in range(K):
                sel = np.nonzero(ok & (key == k))[0]
                if len(sel) == 0:
                    assert idx[k] == n and best[k] == 0.0
                else:
                    assert best[k] == dist[sel].max() and idx[k] == sel[np.argmax(dist[sel])]
            if fp == 'zero_weight_max' and inside.any():
                assert dist.max() == 1e6 and best.max() < 1e6
            if fp == 'weightless_key' and inside.any():
                assert idx[key[inside].min()] == n
    assert seen_cancel_to_zero and seen_negative


def test_cp_dist_ref_rounds_every_operation_on_its_own():
    # (2^27 + 1)^2 = 2^54 + 2^28 + 1 rounds to 2^54 + 2^28; adding 1.0 twice stays (half an ulp of 4, ties to even); a fused or
    # reordered sum would give another bit pattern
    q = np.array([[(1 << 27) + 1, 1, 1]], np.int64)
    out = CASES.cp_dist_ref(q, np.array([0], np.int32), np.zeros((1, 3)))
    assert out[0] == float((1 << 54) + (1 << 28))
    out = CASES.cp_dist_ref(q, np.array([1], np.int32), np.zeros((1, 3)))
    assert out.view(np.int64)[0] == 0


# ---- D ----
def _solve(c):
    stats = {}
    comp, ncom, values, energies = R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], c['m'], stats=stats, **c['kw'])
    return comp, ncom, values, energies, stats


@pytest.mark.parametrize('name', CASES.SCALING_SCENES)
def test_restatement_follows_power_of_two_scalings_exactly(name):
    c = CASES.solver_cases()[name]
    comp, ncom, values, energies, stats = _solve(c)
    assert ncom >= 2 and len(energies) >= 1 and len(stats['pulses']) >= 2
    for variant in CASES.SCALINGS:
        scaled, fv, fe = CASES.scaled_scene(c, variant)
        comp2, ncom2, values2, energies2, stats2 = _solve(scaled)
        assert ncom2 == ncom and np.array_equal(comp2, comp), variant
        assert stats2 == stats, variant
        assert np.array_equal(values2, values * np.float32(fv)), variant
        assert energies2 == [e * fe for e in energies], variant


# ---- E ----
def test_edge_scenes_run_and_pin_what_the_design_states():
    cases = CASES.edge_solver_cases()
    got = {name: _solve(c) for name, c in cases.items()}
    # nothing cut (no edge at all): one component, although the graph is disconnected; max_ite = 0: no energy is recorded
    assert got['grid_no_edges'][1] == 1 and not got['grid_no_edges'][0].any()
    assert got['grid_max_ite0'][1] == 1 and got['grid_max_ite0'][3] == [] and got['grid_max_ite0'][4]['pulses'] == []
    assert got['grid_obs_zero'][1] == 1 and got['grid_obs_zero'][3] == [0.0]
    assert got['grid_node_weight_zero'][1] == 1
    c = cases['grid_node_weight_zero']
    assert np.array_equal(got['grid_node_weight_zero'][2][0], R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], None, reg_strength=1e9)[2][0])
    assert got['random130'][1] > got['random130_cutoff5'][1] >= 1 and got['random130_cutoff5'][4]['merge_rounds'] >= 1
    for name in ('grid_reg_zero', 'grid_edge_weight_zero', 'grid_obs_1e-38', 'grid_obs_5e37', 'grid_edge_weight_3e38', 'grid_kmeans_ite0',
                 'grid_flow_steps1'):
        assert got[name][1] >= 2, name
    for name, (comp, ncom, values, energies, stats) in got.items():
        assert np.isfinite(values).all() and np.isfinite(energies).all(), name
