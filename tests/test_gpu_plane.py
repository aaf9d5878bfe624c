"""GPU: the ground-plane elevation on the device (csrc/spg_plane.hip through ops.plane_elevation; build_structure with
elevation='ransac') against the float64 restatement of tests/plane_restatement.py, which tests/test_plane_restatement.py admits
against sklearn's record on the CPU (tests/golden/plane.npz).

Per case: n_low, low_index and the threshold bit for bit; n_trials, best_trial and the inlier mask equal; the elevation per element
within 0.5 ulp_float32(|e64|) + 8 P of the restatement's float64 elevation e64, where P is the largest change of any element of e64
when the restatement takes the final fit's sums over the inliers in reversed and in a seeded shuffled order (computed on the CPU,
never from the device; the factor 8 because two other orders sample the spread of all orders thinly).  Two runs give the same bits.
The figures measured on an MI355X (device error, P, the recorded distance to sklearn):
`python tests/test_gpu_plane.py` prints them (profiles/plane_errors.txt), with the device time of the 200 000-point room."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

import plane_cases as C
import plane_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace
ORDERS = ('reversed', 7)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def explicit(name):
    return C.EXPLICIT()[name]


CLOUDS = {**{k: (lambda f=f: (f(), None)) for k, f in {**C.PARITY, **C.UNPINNED}.items()},
          **{k: functools.partial(explicit, k) for k in ('x_collinear', 'coincident', 'same_twice', 'zero_first')}}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(xyz, subsets or None, the restatement's result): computed once per case and left unchanged"""
    xyz, subsets = CLOUDS[name]()
    return xyz, subsets, R.plane_elevation(xyz, subsets, orders=ORDERS)


def ulp32(v):
    """the spacing of float32 at |v| (float64 in): 2^(e - 24) for |v| in [2^(e-1), 2^e), the subnormal step below 2^-126"""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(1.0, np.where(v == 0, -149, np.maximum(e - 24, -149)))


def measure(name):
    from superpoint_graph_amd import ops
    xyz, subsets, ref = reference(name)
    out = ops.plane_elevation(dev(xyz), subsets=subsets)
    again = ops.plane_elevation(dev(xyz), subsets=subsets)
    e64 = ref['elevation']
    P = max(float(np.abs(r - e64).max()) for r in ref['reordered'])
    err = np.abs(host(out['elevation']).astype(np.float64) - e64)
    bound = 0.5 * ulp32(e64) + 8 * P
    return types.SimpleNamespace(out=out, again=again, ref=ref, P=P, err=float(err.max()), ratio=float((err / bound).max()), xyz=xyz)


def check(name):
    m = measure(name)
    out, ref = m.out, m.ref
    print(f'{name}: n_low {out["n_low"]} trials {out["n_trials"]} best {out["best_trial"]} max error {m.err:.3e} error / bound {m.ratio:.3f} '
          f'P {m.P:.3e}')
    assert out['n_low'] == ref['n_low']
    assert out['low_index'].dtype == torch.int32 and np.array_equal(host(out['low_index']), ref['low_index'])
    assert out['threshold'].dtype == torch.float32
    assert host(out['threshold']).view(np.uint32) == np.asarray(ref['threshold']).view(np.uint32), (host(out['threshold']), ref['threshold'])
    assert (out['n_trials'], out['best_trial']) == (ref['n_trials'], ref['best_trial'])
    assert out['inlier_mask'].dtype == torch.uint8 and np.array_equal(host(out['inlier_mask']), ref['inlier_mask'])
    assert out['elevation'].dtype == torch.float32 and out['coef'].dtype == out['intercept'].dtype == torch.float64
    assert m.ratio <= 1.0, f'{name}: worst element at {m.ratio:.3f} of 0.5 ulp + 8 P (P = {m.P:.3e})'
    assert np.allclose(host(out['coef']), ref['coef'], rtol=1e-7, atol=1e-9) and abs(float(out['intercept']) - ref['intercept']) <= 1e-6
    for k in ('elevation', 'coef', 'intercept', 'threshold', 'low_index', 'inlier_mask'):
        assert np.array_equal(host(out[k]).reshape(-1).view(np.uint8), host(m.again[k]).reshape(-1).view(np.uint8)), f'{name}: {k} differs between two runs'
    assert (out['n_trials'], out['best_trial']) == (m.again['n_trials'], m.again['best_trial'])
    return m


@pytest.mark.parametrize('name', list(C.PARITY))
def test_parity_cases(hip, name):
    """the cases admitted against sklearn: the rooms, the sampler's branches (n_low 3, 4, 299, 300, 301), one workgroup of low points
    minus one / exactly / plus one, several workgroups, every point low"""
    m = check(name)
    rec = np.load(os.path.join(GOLDEN, 'plane.npz'))
    assert np.array_equal(host(m.out['inlier_mask']), rec[f'{name}/inlier_mask'])                   # sklearn's own consensus set
    assert (m.out['n_trials'], m.out['best_trial']) == (int(rec[f'{name}/n_trials']), int(rec[f'{name}/best_trial']))


@pytest.mark.parametrize('name', list(C.UNPINNED))
def test_cases_judged_by_the_restatement(hip, name):
    """the 200 000-point room 1000 m from the origin (sklearn fits in float32 there) and the exactly flat floor (threshold 0)"""
    m = check(name)
    if name == 'flat_floor':
        assert float(m.out['threshold']) == 0.0 and np.array_equal(host(m.out['coef']), [0.0, 0.0])


@pytest.mark.parametrize('name', ['x_collinear', 'coincident', 'same_twice', 'zero_first'])
def test_explicit_subsets(hip, name):
    m = check(name)
    if name == 'same_twice':                # a tie of count and score: the later trial, with the result of the earlier one alone
        from superpoint_graph_amd import ops
        xyz, subsets, _ = reference(name)
        assert (m.out['n_trials'], m.out['best_trial']) == (2, 1)
        first = ops.plane_elevation(dev(xyz), subsets=subsets[:1])
        assert first['best_trial'] == 0 and torch.equal(first['elevation'].view(torch.int32), m.out['elevation'].view(torch.int32))
    if name == 'zero_first':
        assert float(m.out['threshold']) == 0.0 and m.out['best_trial'] == 1
    if name in ('x_collinear', 'coincident'):
        assert m.out['best_trial'] > 0


def test_refusals(hip):
    from superpoint_graph_amd import ops
    xyz, special = C.degenerate_floor()
    with pytest.raises(ValueError, match='consensus'):
        ops.plane_elevation(dev(xyz), subsets=[special, special])
    two_low = np.array([[0, 0, 0], [1, 0, 0.1], [0, 1, 2], [1, 1, 3], [2, 2, 4]], np.float32)
    with pytest.raises(ValueError, match='min_samples'):
        ops.plane_elevation(dev(two_low))
    bad = C.PARITY['low299']()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match='NaN or infinity'):
        ops.plane_elevation(dev(bad))
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match='NaN or infinity'):
        ops.plane_elevation(dev(bad))
    with pytest.raises(IndexError, match='subset index'):
        ops.plane_elevation(dev(C.PARITY['low299']()), subsets=[[0, 1, 299]])
    with pytest.raises(ValueError, match='subsets'):
        ops.plane_elevation(dev(C.PARITY['low299']()), subsets=[[0, 1]])


def test_build_structure_with_the_ransac_elevation(hip):
    """on the raw scene of tests/golden/scene_structure.npz: the elevation is ops.plane_elevation of the pruned cloud bit for bit,
    every other field is that of the plane_model = 0 build"""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    rec = np.load(os.path.join(GOLDEN, 'scene_structure.npz'))
    i = 1
    raw = [rec[f'scene{i}/raw_{k}'] for k in ('xyz', 'rgb', 'labels', 'objects')]
    args = dict(k_nn_local=int(rec['k_nn_local']), k_nn_adj=int(rec['k_nn_adj']), voxel_width=float(rec['voxel_width'][i]), compute_geof=1,
                use_voronoi=0.0)
    assert args['voxel_width'] > 0
    dataset, n_labels = str(rec['datasets'][i]), int(rec['n_labels'])
    plain = GP.build_structure(*raw, NS(plane_model=0, **args), dataset, n_labels)
    scene = GP.build_structure(*raw, NS(plane_model=1, **args), dataset, n_labels, elevation='ransac')
    want = ops.plane_elevation(plain.xyz)
    assert scene.elevation.dtype == torch.float32 and torch.equal(scene.elevation.view(torch.int32), want['elevation'].view(torch.int32))
    assert not torch.equal(scene.elevation, plain.elevation)
    for k in ('xyz', 'rgb', 'nei', 'edg_source', 'edg_target', 'is_transition', 'labels', 'objects', 'xyn', 'geof'):
        a, b = getattr(scene, k), getattr(plain, k)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(host(a).view(np.uint8), host(b).view(np.uint8)), k
    # plane_model = 0 takes z - min z whatever the elevation asks for; another word is refused
    flat = GP.build_structure(*raw, NS(plane_model=0, **args), dataset, n_labels, elevation='ransac')
    assert torch.equal(flat.elevation.view(torch.int32), plain.elevation.view(torch.int32))
    with pytest.raises(ValueError, match='ransac'):
        GP.build_structure(*raw, NS(plane_model=1, **args), dataset, n_labels, elevation='plane')


def device_ms(xyz, repeats=20):
    """ops.plane_elevation end to end (its two host reads included), device events after warm-up -> median ms"""
    from superpoint_graph_amd import ops
    x = dev(xyz)
    for _ in range(3):
        ops.plane_elevation(x)
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.plane_elevation(x)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = np.load(os.path.join(GOLDEN, 'plane.npz'))
    print('# python tests/test_gpu_plane.py')
    print('# per case: worst |device elevation - float64 restatement| over all points, that error over its allowance 0.5 ulp_f32(|e64|) + 8 P,')
    print("# P (the restatement's own spread over two other summation orders of the final fit), and the recorded max |sklearn - e64|")
    print(f'{"case":<20}{"n":>8}{"n_low":>8}{"trials":>7}{"best":>5}{"abs error":>12}{"err/bound":>10}{"P":>11}{"sklearn":>11}')
    for name in CLOUDS:
        m = measure(name)
        dist = f'{float(rec[f"{name}/dist"]):.3e}' if f'{name}/dist' in rec.files else '-'
        print(f'{name:<20}{len(m.xyz):>8}{m.out["n_low"]:>8}{m.out["n_trials"]:>7}{m.out["best_trial"]:>5}{m.err:>12.3e}{m.ratio:>10.3f}{m.P:>11.3e}{dist:>11}')
    big = 'room200000_1000m'
    print(f'# time, {big}: ops.plane_elevation {device_ms(reference(big)[0]):.3f} ms on the device (events, median of 20 after 3 warm-up '
          f'calls, 100 trials evaluated); sklearn RANSACRegressor fit + predict {float(rec[f"sklearn_seconds/{big}"]) * 1e3:.1f} ms on the CPU of the '
          'machine that wrote the record')
