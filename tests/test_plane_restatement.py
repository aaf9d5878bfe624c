"""CPU: the float64 restatement of the ground-plane elevation (tests/plane_restatement.py) and the host sampler
ops.ransac_subsets against sklearn's own RANSACRegressor, recorded in tests/golden/plane.npz by tools/gen_plane_golden.py.

1. The sampler: the restatement's `subsets` and ops.ransac_subsets against the recorded stream of sample_without_replacement at
   every size of plane_cases.SAMPLER_SIZES (both sides of 3 / n = 0.01 and of n = 3), and against sklearn itself where it imports.
2. Admission of the parity cases of tests/test_gpu_plane.py: the restatement and sklearn agree on the best trial, the number of
   trials and the inlier mask; no residual of an evaluated trial lies within 1e-9 (relative) of the threshold, and no trial ties the
   best count.  A case that fails is replaced in tests/plane_cases.py, not tolerated: none is left out.
3. The recorded distance between sklearn's float32 elevation and the restatement's, and the restatement's own edge rules."""
import os

import numpy as np
import pytest

import plane_cases as C
import plane_restatement as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'plane.npz'))


@pytest.mark.parametrize('n', C.SAMPLER_SIZES)
def test_sampler_against_the_record(rec, n):
    from superpoint_graph_amd import ops
    assert np.array_equal(R.subsets(n, 100, 0), rec[f'sampler/{n}'])
    got = ops.ransac_subsets(n, 100, 0)
    assert got.dtype == np.int64 and np.array_equal(got, rec[f'sampler/{n}'])
    assert np.array_equal(ops.ransac_subsets(n, 7, 0), rec[f'sampler/{n}'][:7])              # a prefix of the same stream


@pytest.mark.parametrize('n', C.SAMPLER_SIZES)
def test_sampler_against_sklearn(n):
    sklearn_random = pytest.importorskip('sklearn.utils.random')
    from superpoint_graph_amd import ops
    for seed in (0, 5):
        rs = np.random.RandomState(seed)
        want = np.stack([sklearn_random.sample_without_replacement(n, 3, random_state=rs) for _ in range(100)])
        assert np.array_equal(ops.ransac_subsets(n, 100, seed), want)
        assert np.array_equal(R.subsets(n, 100, seed), want)


def test_sampler_refuses_fewer_than_three():
    from superpoint_graph_amd import ops
    for f in (ops.ransac_subsets, R.subsets):
        with pytest.raises(ValueError, match='min_samples'):
            f(2, 100, 0)


@pytest.mark.parametrize('name', list(C.PARITY))
def test_admission(rec, name):
    xyz = C.PARITY[name]()
    r = R.plane_elevation(xyz)
    assert np.array_equal(r['subsets'], rec[f'{name}/subsets'])
    assert r['n_low'] == rec[f'{name}/inlier_mask'].size
    assert (r['n_trials'], r['best_trial']) == (int(rec[f'{name}/n_trials']), int(rec[f'{name}/best_trial']))
    assert np.array_equal(r['inlier_mask'], rec[f'{name}/inlier_mask'])
    assert r['margin'] >= 1e-9 and not r['tie'], (r['margin'], r['tie'])
    dist = float(np.abs(rec[f'{name}/elevation'].astype(np.float64) - r['elevation']).max())
    assert dist == float(rec[f'{name}/dist'])
    # sklearn fits and predicts in float32: a few float32 steps of the coordinates times the slope, and of z itself
    scale = float(np.abs(xyz).max())
    assert dist <= 64 * np.finfo(np.float32).eps * scale, (dist, scale)
    assert np.allclose(r['coef'], rec[f'{name}/coef'], rtol=0, atol=1e-3)


def test_every_case_is_recorded(rec):
    for name in list(C.PARITY) + list(C.UNPINNED):
        assert f'{name}/inlier_mask' in rec.files
    assert 'room200000_1000m/elevation' not in rec.files            # judged by the restatement alone


def test_flat_floor_has_threshold_zero(rec):
    r = R.plane_elevation(C.UNPINNED['flat_floor']())
    assert float(r['threshold']) == 0.0 and r['tie']
    assert np.array_equal(r['coef'], [0.0, 0.0]) and int(r['inlier_mask'].sum()) == 420
    assert np.array_equal(r['inlier_mask'], rec['flat_floor/inlier_mask'])


def test_degenerate_triples():
    """numpy's lstsq on centred data: x-collinear points give a slope along y only, coincident ones the zero plane"""
    P = np.array([[1.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 3.0, 5.0]])
    a, b, xr, yr, zr = R.triple_plane(P)
    ref = np.linalg.lstsq(P[:, :2] - P[:, :2].mean(0), P[:, 2] - P[:, 2].mean(), rcond=None)[0]
    assert a == 0.0 and abs(b - ref[1]) < 1e-14 and abs(ref[0]) < 1e-14
    assert R.triple_plane(np.repeat(P[1:2], 3, 0))[:2] == (0.0, 0.0)
    Q = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [3.0, 3.0, 2.0]])             # collinear along the diagonal
    a, b = R.triple_plane(Q)[:2]
    ref = np.linalg.lstsq(Q[:, :2] - Q[:, :2].mean(0), Q[:, 2] - Q[:, 2].mean(), rcond=None)[0]
    assert np.allclose([a, b], ref, rtol=0, atol=1e-14)
    G = np.array([[0.0, 0.0, 1.0], [2.0, 0.0, 2.0], [0.0, 4.0, -1.0]])            # in general position: the plane through the points
    a, b, xr, yr, zr = R.triple_plane(G)
    assert np.allclose([a, b], [0.5, -0.5], rtol=0, atol=1e-15) and np.allclose(R.residuals((a, b, xr, yr, zr), G[:, :2], G[:, 2]), 0, atol=1e-15)


def test_replay_rules():
    inf = float('inf')
    # a first trial without inliers is skipped; equal count and lower score is skipped, equal score is taken (the later trial)
    assert R.replay([0, 5, 5, 5], [0.0, 0.5, 0.4, 0.5], 10, 4) == (4, 3, True)
    assert R.replay([0, 0], [0.0, 0.0], 10, 2) == (2, -1, False)
    assert R.replay([10, 3], [1.0, 1.0], 10, 2) == (1, 0, False)                   # every sample an inlier: one trial suffices
    assert R.dynamic_max_trials(0, 10) == inf and R.dynamic_max_trials(5, 10) == 35.0


def test_explicit_subsets():
    cases = C.EXPLICIT()
    r = R.plane_elevation(*cases['same_twice'])
    assert r['tie'] and (r['n_trials'], r['best_trial']) == (2, 1) and r['scores'][0] == r['scores'][1]
    first = R.plane_elevation(cases['same_twice'][0], cases['same_twice'][1][:1])
    assert np.array_equal(first['elevation'], r['elevation']) and np.array_equal(first['inlier_mask'], r['inlier_mask'])
    r = R.plane_elevation(*cases['zero_first'])
    assert float(r['threshold']) == 0.0 and r['counts'][0] == 0 and r['best_trial'] == 1 and r['counts'][1] >= 420
    for name in ('x_collinear', 'coincident'):
        r = R.plane_elevation(*cases[name])
        assert r['best_trial'] > 0 and np.isfinite(r['elevation']).all()
    xyz, special = C.degenerate_floor()
    with pytest.raises(ValueError, match='consensus'):
        R.plane_elevation(xyz, [special, special])
