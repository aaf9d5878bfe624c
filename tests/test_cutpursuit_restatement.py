"""The numpy restatement of cut pursuit (cutpursuit_restatement.py) against an outside judge and its own properties: its min cut
against scipy's maximum_flow (value and the canonical sink side), the solver on planted grids."""
import numpy as np
import pytest

import cutpursuit_cases as CASES
import cutpursuit_restatement as R

MINCUT = CASES.mincut_cases()
SOLVER = CASES.solver_cases()


def _scipy_cut(c):
    """(max-flow value, the vertices that reach the sink in scipy's residual graph) of the flow model of ops.min_cut"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    n, s, t = c['n'], c['n'], c['n'] + 1
    keep = c['src'] != c['tgt']
    src, tgt, cap = c['src'][keep], c['tgt'][keep], c['cap'][keep]
    rows = np.concatenate([src, tgt, np.full(n, s), np.arange(n)])
    cols = np.concatenate([tgt, src, np.arange(n), np.full(n, t)])
    vals = np.concatenate([cap, cap, c['cost1'], c['cost0']])
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n + 2, n + 2)).tocsr()      # parallel edges add up
    assert A.max() < 2 ** 31
    A = A.astype(np.int32)
    out = maximum_flow(A, s, t)
    flow = out.flow if hasattr(out, 'flow') else out.residual
    resid = (A - flow).tocoo()                                               # residual capacity of every arc (flow is antisymmetric)
    ok = resid.data > 0
    tail, head = resid.row[ok], resid.col[ok]
    reach = np.zeros(n + 2, bool)
    reach[t] = True
    while True:
        new = reach.copy()
        new[tail[reach[head]]] = True
        if (new == reach).all():
            break
        reach = new
    return int(out.flow_value), reach[:n].astype(np.uint8)


@pytest.mark.parametrize('name', sorted(MINCUT))
def test_min_cut_against_scipy(name):
    c = MINCUT[name]
    label, pulses = R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])
    value, sink_side = _scipy_cut(c)
    assert R.cut_value(label, c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1']) == value
    assert np.array_equal(label, sink_side)


def test_min_cut_random_small_graphs_against_scipy():
    rng = np.random.default_rng(1)
    for _ in range(60):
        n = int(rng.integers(1, 40))
        c = CASES._random_graph(rng, n, int(rng.integers(0, 4 * n)), cap_hi=20, cost_hi=30)
        c = {k: (np.asarray(v, np.int64) if k != 'n' else v) for k, v in c.items()}
        label, _ = R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])
        value, sink_side = _scipy_cut(c)
        assert R.cut_value(label, c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1']) == value
        assert np.array_equal(label, sink_side)


def test_min_cut_pulse_cap_and_limits():
    c = MINCUT['path300']
    with pytest.raises(RuntimeError, match='max_pulses'):
        R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'], max_pulses=5)
    with pytest.raises(ValueError, match='2\\^28'):
        R.min_cut(2, [0], [1], [1 << 28], [0, 0], [0, 0])


def _run(c, **over):
    stats = {}
    kw = dict(c['kw'], **over)
    comp, ncom, values, energies = R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], c['m'], stats=stats, **kw)
    return comp, ncom, values, energies, stats


def _energy_of(c, comp, lam):
    q, kf, mq, km = R.quantise(c['obs'], c['m'])
    comp = np.asarray(comp, np.int64)
    return R.energy(q, kf, mq, km, comp, int(comp.max()) + 1, c['src'], c['tgt'], c['w'], lam)


def _same_partition(a, b):
    pairs = np.unique(np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


@pytest.mark.parametrize('name', sorted(k for k, c in SOLVER.items() if c['planted'] is not None))
def test_planted_grid_is_recovered(name):
    c = SOLVER[name]
    comp, ncom, values, energies, _ = _run(c)
    assert ncom == 4 and _same_partition(comp, c['planted'])
    assert all(b <= a for a, b in zip(energies, energies[1:])), energies
    lam = c['kw']['reg_strength']
    assert energies[-1] <= _energy_of(c, c['planted'], lam)
    assert energies[-1] <= _energy_of(c, np.zeros(len(comp)), lam)
    # numbered by smallest member, values are the weighted means
    first = [int(np.nonzero(comp == k)[0][0]) for k in range(ncom)]
    assert first == sorted(first)
    m = np.ones(len(comp)) if c['m'] is None else c['m'].astype(np.float64)
    for k in range(ncom):
        sel = comp == k
        mean = (m[sel, None] * c['obs'][sel].astype(np.float64)).sum(0) / m[sel].sum()
        assert np.allclose(values[k], mean, rtol=0, atol=4e-6 * np.abs(c['obs']).max())


@pytest.mark.parametrize('name', ['overseg', 'inpainting', 'decay07'])
def test_energy_never_rises(name):
    c = SOLVER[name]
    comp, ncom, values, energies, _ = _run(c, weight_decay=1.0)
    assert all(b <= a for a, b in zip(energies, energies[1:])), energies
    assert energies[-1] <= _energy_of(c, np.zeros(len(comp)), c['kw']['reg_strength'])


@pytest.mark.parametrize('name', ['overseg_cutoff10', 'decay07_cutoff10'])
def test_cutoff_leaves_no_small_component_with_a_neighbour(name):
    c = SOLVER[name]
    before = _run(c, cutoff=0)
    comp, ncom, values, energies, stats = _run(c)
    size = np.bincount(comp, minlength=ncom)
    assert np.bincount(before[0]).min() < 10 < before[1] and stats['merge_rounds'] >= 1      # the merge had work to do
    a, b = comp[c['src']], comp[c['tgt']]
    has_neighbour = np.zeros(ncom, bool)
    has_neighbour[a[a != b]] = True
    has_neighbour[b[a != b]] = True
    assert not (has_neighbour & (size < 10)).any()
    assert ncom < before[1]


def test_degenerate_scenes():
    comp, ncom, values, energies, _ = _run(SOLVER['duplicates'])
    assert ncom == 1 and not comp.any() and energies == [0.0]
    assert np.array_equal(values, SOLVER['duplicates']['obs'][:1])
    comp, ncom, values, energies, _ = _run(SOLVER['n1'])
    assert ncom == 1 and comp.tolist() == [0] and np.array_equal(values, SOLVER['n1']['obs'])


def test_inpainting_fills_every_vertex():
    c = SOLVER['inpainting']
    comp, ncom, values, energies, _ = _run(c)
    assert ncom >= 4 and values.shape == (ncom, 1)
    known = c['m'] > 0
    assert np.array_equal(values[comp[known], 0], c['obs'][known, 0])          # labels are reproduced where they are known
