"""CPU: the case builders and float64 references of tests/partition_cases.py (run on the device by
tests/test_gpu_partition_edges.py) -- every builder reaches the branch it claims, the new superpoint reference agrees with the
oracle that is pinned to the reference goldens, the verticality mask excludes next to nothing, and the restatement of `prune`
gives a hand-written answer on points that lie on voxel faces and on a -0.0 minimum."""
import os

import numpy as np
import pytest

import partition_cases as C
from conftest import GOLDEN
from oracle import spg_partition_oracle as P
from test_gpu_spgraph import TOL      # max |a - b| / max |ref| per array: what the device is held to against the same goldens
from test_partition_oracle import golden_case


# ---------------------------------------------------------------------------------------------------------------------
# compute_geof
# ---------------------------------------------------------------------------------------------------------------------
def test_geof_cases_cover_the_claimed_shapes():
    cases = C.geof_cases()
    assert {c['k_nn'] for c in cases} >= {0, 1, 2, 45, 63, 64, 100, 150}
    assert {len(c['xyz']) for c in cases} >= {1, 255, 256, 257, 50_000}
    ks = [c['k_nn'] for c in cases]
    first_big = min(i for i, k in enumerate(ks) if k >= 64)
    assert first_big > 10 and all(k >= 64 for k in ks[first_big:])                  # the > 64 KB launches come last
    assert max(256 * (k + 1) * 4 for k in ks) == 154_624 and 256 * 65 * 4 > 65_536
    assert len({c['name'] for c in cases}) == len(cases)
    by = {c['name']: c for c in cases}
    c = by['repeats_and_self_n1000_k45']
    t = c['target'].reshape(-1, 45)
    assert (t[::2, 20] == np.arange(0, 1000, 2)).all() and (np.sort(t, 1)[:, 1:] == np.sort(t, 1)[:, :-1]).any(1).all()
    for name in ('collinear_n300_k8', 'coplanar_n384_k20', 'isotropic_lattice_n343_k6'):      # clamped windows: repeats and self
        t = by[name]['target'].reshape(len(by[name]['xyz']), -1)
        assert (t == np.arange(len(t))[:, None]).any() and (np.sort(t, 1)[:, 1:] == np.sort(t, 1)[:, :-1]).any()
    assert np.abs(by['shifted_1e5_n5000_k45']['xyz']).min(0).max() > 4e4
    assert len(np.unique(by['shifted_1e5_n5000_k45']['xyz'], axis=0)) == 5000


def test_geof_degenerate_cases_are_exactly_degenerate():
    by = {c['name']: c for c in C.geof_cases()}
    for c in by.values():                                                          # exact inputs: multiples of 1/8 survive float32
        if c['kind'] in ('exact', 'isotropic'):
            assert np.array_equal(c['xyz'] * 8, np.rint(c['xyz'] * 8)), c['name']
    lam = C.geof_reference_eigenvalues(**{k: by['collinear_n300_k8'][k] for k in ('xyz', 'target', 'k_nn')})
    assert (lam[:, 0] > 0.1).all() and (lam[:, 1] <= 1e-12 * lam[:, 0]).all()                       # rank 1
    lam = C.geof_reference_eigenvalues(**{k: by['coplanar_n384_k20'][k] for k in ('xyz', 'target', 'k_nn')})
    assert (lam[:, 1] > 1e-3 * lam[:, 0]).all() and (lam[:, 2] <= 1e-12 * lam[:, 0]).all()          # rank 2
    assert (lam[:, 0] - lam[:, 1] > 1e-2 * lam[:, 0]).all()                                         # two distinct in-plane eigenvalues
    c = by['isotropic_lattice_n343_k6']
    lam = C.geof_reference_eigenvalues(c['xyz'], c['target'], c['k_nn'])
    grid = np.rint((c['xyz'] + 1.5) * 2).astype(int)
    interior = ((grid > 0) & (grid < 6)).all(1)
    assert interior.sum() == 125 and np.array_equal(lam[interior], np.full((125, 3), 2 * 0.25 / 7))  # (2 h^2 / 7) I, exactly
    ref = P.geof(c['xyz'], c['target'], c['k_nn'])
    assert np.array_equal(ref[interior, :3], np.tile(np.float32([0, 0, 1]), (125, 1)))
    for name in ('n1_k0', 'n1_k2_self', 'n256_k0', 'all_coincident_n257_k45'):                      # 0/0: NaN in all four features
        c = by[name]
        assert c['kind'] == 'nan' and np.isnan(P.geof(c['xyz'], c['target'], c['k_nn'])).all(), name
    c = by['coincident_block_n300_k12']
    ref = P.geof(c['xyz'], c['target'], c['k_nn'])
    assert np.isnan(ref[:100]).all() and not np.isnan(ref[100:]).any()


def test_verticality_mask_excludes_next_to_nothing():
    """A condition on the inputs, checked with the restatement alone: at most 0.1 % of a random cloud, nothing of a constructed
    well-defined case.  (The exactly isotropic lattice may lose every point: it exists for the other three features.)"""
    for c in C.geof_cases():
        if c['kind'] == 'nan':
            continue
        lam = C.geof_reference_eigenvalues(c['xyz'], c['target'], c['k_nn'])
        live = lam[:, 0] > 0
        masked = 1.0 - C.verticality_mask(lam)[live].mean()
        if c['kind'] == 'random':
            assert masked <= 1e-3, (c['name'], masked)
        elif c['kind'] == 'exact':
            assert masked == 0.0, (c['name'], masked)
        else:
            assert c['kind'] == 'isotropic' and masked > 0.3


def test_geof_measure_sees_an_error_above_the_tolerance():
    by = {c['name']: c for c in C.geof_cases()}
    for name in ('random_n257_k45', 'coincident_block_n300_k12'):
        case = by[name]
        ref = P.geof(case['xyz'], case['target'], case['k_nn'])
        m = C.geof_measure(ref, case)
        assert m['nan_equal'] and not m['worst'].any()
        for f in range(4):
            bad = ref.copy()
            bad[-1, f] += np.float32(1e-4)
            assert C.geof_measure(bad, case)['worst'][f] > C.GEOF_ATOL
        bad = ref.copy()
        bad[0, 3] = 0.5 if np.isnan(ref[0, 3]) else np.nan
        assert not C.geof_measure(bad, case)['nan_equal']


def test_verticality_mask_rule():
    lam = np.array([[1.0, 0.5, 0.1], [1.0, 1.0 - 5e-7, 0.1], [1.0, 0.5, 0.5 - 1e-7], [1.0, 1e-8, 0.0], [1.0, 2e-6, 1.5e-6], [0.0, 0.0, 0.0]])
    assert C.verticality_mask(lam).tolist() == [True, False, False, True, False, False]


# ---------------------------------------------------------------------------------------------------------------------
# superpoints
# ---------------------------------------------------------------------------------------------------------------------
def test_superpoint_cases_reach_every_branch():
    for case in C.superpoint_cases():
        xyz, comp, n_com, claims = case['xyz'], case['comp'], case['n_com'], case['claims']
        f = C.superpoint_features_f64(xyz, comp, n_com)
        what = {v: k for k, v in claims.items()}
        nu, cnt = f['n_unique'], f['count']
        c = what['copies_of_one_point']
        assert nu[c] == 1 and cnt[c] == 40
        c = what['two_points_with_copies']
        assert nu[c] == 2 and cnt[c] == 12
        first = np.lexsort(xyz[comp == c].T[::-1])                                 # the copies of the first point sit between it and the second
        assert (xyz[comp == c][first[:5]] == xyz[comp == c][first[0]]).all()
        assert nu[what['three_points']] == 3 and cnt[what['three_points']] == 3
        assert nu[what['single_point']] == 1 and cnt[what['single_point']] == 1
        c = what['collinear']
        assert f['ev'][c, 0] > 1 and f['ev'][c, 1] <= 1e-13 * f['ev'][c, 0] and abs(f['surface'][c] - 1e-5) < 1e-9
        c = what['coplanar']
        assert f['ev'][c, 1] > 0.1 and f['ev'][c, 2] <= 1e-13 * f['ev'][c, 0] and abs(f['volume'][c] - 1e-5) < 1e-9
        c = what['signed_zero_two_unique']
        pts = xyz[comp == c]
        assert nu[c] == 2 and cnt[c] == 4 and np.signbit(pts[:, 0]).any() and ((pts[:, 0] == 0) & ~np.signbit(pts[:, 0])).any()
        c = what['signed_zero_five_unique']
        assert nu[c] == 5 and cnt[c] == 7
        for m in (65, 128, 129):
            assert nu[what[f'unique_{m}']] == m and cnt[what[f'unique_{m}']] == m + 2
        assert nu[what['unique_64_each_twice']] == 64 and cnt[what['unique_64_each_twice']] == 128
        small, big = what['thin_small'], what['large_blob']
        assert f['volume'][small] < 1e-4 * f['volume'][big] and f['surface'][small] < 1e-4 * f['surface'][big]
        assert f['ev'][small, 2] > 0
        if 'gaps' in case['name']:
            assert n_com == comp.max() + 2 and (cnt == 0).sum() == 2 and cnt[10] == 0 and cnt[15] == 0
            lab = case['labels']
            assert lab.ndim == 1 and (lab == case['n_labels'] + 1).sum() == 20 and (lab == 200).sum() == 20 and (lab < 0).sum() == 20
            ref = C.sp_graph_reference(case)
            assert ref['sp_labels'].sum() == len(xyz) - 60 and ref['sp_labels'].shape == (n_com, case['n_labels'] + 1)
            assert not ref['sp_labels'][[10, 15]].any() and not ref['sp_point_count'][[10, 15]].any()
        else:
            assert n_com == comp.max() + 1 and (cnt > 0).all()
        # without a length limit every non-empty component takes part in a superedge
        ref = C.sp_graph_reference(case)
        assert case['d_max'] > 0 or set(np.flatnonzero(cnt)) <= set(ref['source'][:, 0].tolist())
    a, b = C.superpoint_cases()[:2]
    assert len(C.sp_graph_reference(b)['source']) < len(C.sp_graph_reference(a)['source'])          # d_max = 6 removes superedges


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_superpoint_features_f64_agrees_with_the_pinned_oracle(tag):
    g = np.load(os.path.join(GOLDEN, 'sp_graph.npz'))
    (xyz, d_max, comp, components, labels, n_labels, tets), ref = golden_case(g, tag)
    n_com = len(components)
    f = C.superpoint_features_f64(xyz, comp, n_com)
    assert np.array_equal(f['count'], ref['sp_point_count'][:, 0])
    for key, name in (('sp_centroids', 'centroid'), ('sp_length', 'length'), ('sp_surface', 'surface'), ('sp_volume', 'volume')):
        a = ref[key].astype(np.float64).reshape(f[name].shape)
        mine = f[name] if name in ('centroid', 'length') else np.where(f['n_unique'] > 2, f[name], 0.0)
        assert np.abs(a - mine).max() <= TOL[key] * np.abs(a).max(), key
    # ... and the golden itself, which the reference computed, lies inside the per-component bounds except for the centroids:
    # the reference's pts.mean(0) is a float32 running mean (error ~ m eps32), not the rounded float64 mean the bound describes
    m = C.superpoint_measure(ref, xyz, comp, n_com)
    for name in ('length', 'surface', 'volume'):
        assert m[name][1] <= 1.0, (name, m[name])


def test_superpoint_bounds_catch_a_wrong_small_component():
    """What the array-relative compare() cannot see: the thin component's volume off by a factor, its second and third
    eigenvalue swapped -- both far outside the per-component bound, both below 2e-6 of the array's maximum."""
    case = C.superpoint_cases()[0]
    ref = C.sp_graph_reference(case)
    base = C.superpoint_measure(ref, case['xyz'], case['comp'], case['n_com'])
    assert all(base[k][1] <= 1.0 for k in ('length', 'surface', 'volume')), base
    what = {v: k for k, v in case['claims'].items()}
    f = C.superpoint_features_f64(case['xyz'], case['comp'], case['n_com'])
    c = what['thin_small']
    for key, wrong in (('sp_volume', f['volume'][c] * 1.5), ('sp_surface', np.sqrt(f['ev'][c, 0] * f['ev'][c, 2] + 1e-10))):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        bad[key][c, 0] = wrong
        assert 0 < np.abs(bad[key] - ref[key]).max() <= 2e-6 * np.abs(ref[key]).max()          # invisible to compare()
        got = C.superpoint_measure(bad, case['xyz'], case['comp'], case['n_com'])
        assert got[key[3:]][1] > 100 and got[key[3:]][2] == c


# ---------------------------------------------------------------------------------------------------------------------
# superedges
# ---------------------------------------------------------------------------------------------------------------------
def test_superedge_cases_reach_every_branch():
    by = {c['name']: c for c in C.superedge_cases()}
    for name in ('handbuilt_counts_dmax0', 'handbuilt_counts_dmax-1'):
        case = by[name]
        st = C.superedge_stats_f64(case)
        got = {(int(s), int(t)): int(c) for s, t, c in zip(st['source'], st['target'], st['count'])}
        assert got == case['expect']
        assert {1, 64, 65, 129} <= set(got.values()) and case['d_max'] <= 0
        ref = C.sp_graph_reference(case)
        one = np.flatnonzero(st['count'] == 1)
        assert len(one) == 2 and not ref['se_delta_std'][one].any()                               # std = 0 branch
        assert np.array_equal(ref['se_delta_mean'][one[0]], -ref['se_delta_mean'][one[1]])
        m = C.superedge_measure(ref, case)                                                        # the float32 oracle inside ~count eps32
        assert m['mean'][0] < 1e-5 and m['norm'][0] < 1e-5
    xyz = by['length_equals_dmax_5']['xyz']
    d = np.sqrt(((xyz[0] - xyz[1:7]) ** 2).sum(1))
    assert d.dtype == np.float32 and d.tolist() == [5.0, 5.0, 5.0, 2.5, 10.0, float(np.sqrt(np.float32(25.0625)))]
    assert by['length_equals_dmax_next']['d_max'] == float(np.float32(5.0) + np.float32(2.0 ** -21)) and d[5] > by['length_equals_dmax_next']['d_max']
    for name in ('length_equals_dmax_5', 'length_equals_dmax_next', 'length_equals_dmax_0', 'length_equals_dmax_neg'):
        case = by[name]
        e = P.interface_edges(case['tets'], case['comp'], case['xyz'], case['d_max'])
        assert set(e[1, e[0] == 0].tolist()) == case['expect_edges_from_0'], name
    assert by['length_equals_dmax_0']['d_max'] == 0.0 and by['length_equals_dmax_neg']['d_max'] == -1.0
    sizes = {}
    for name, case in by.items():
        if name.startswith('delaunay'):
            st = C.superedge_stats_f64(case)
            sizes[name] = len(st['count'])
            assert st['count'].max() > 64 and st['count'].min() < 8 and len(st['count']) >= 20
    assert len(sizes) == 3 and min(sizes.values()) < max(sizes.values())                         # d_max = 0.9 removes superedges; 0 and -1 do not
    assert sizes['delaunay_n4043_dmax0'] == sizes['delaunay_n4043_dmax-1']


def test_ratio_rows_from_own_features_reproduce_the_oracle_bitwise():
    """graphs.py:186-190 applied to a result's own superpoint features: bit-equal on the oracle (which is the reference's code
    path), so the device's rows can be held to the same."""
    for case in (C.superedge_cases()[0], C.superedge_cases()[-3], C.superpoint_cases()[0]):
        ref = C.sp_graph_reference(case)
        rows = C.ratio_rows_from_own_features(ref)
        for k, v in rows.items():
            assert v.dtype == np.float32 and np.array_equal(v.reshape(ref[k].shape), ref[k]), (case['name'], k)


# ---------------------------------------------------------------------------------------------------------------------
# prune
# ---------------------------------------------------------------------------------------------------------------------
def test_prune_cases_cover_the_claimed_sizes_and_edges():
    cases = {c['name']: c for c in C.prune_cases()}
    assert {len(c['xyz']) for c in cases.values()} >= {1, 262_143, 262_144, 1_000_000}
    assert len(cases['n262144']['xyz']) >= 262_144 and len(cases['n1000000']['xyz']) >= 262_144   # the grid-stride min / max launch
    assert len(cases['n262143']['xyz']) < 262_144                                                 # ... and the last one-pass size
    for name in ('n262143', 'n262144', 'n1000000'):
        c = cases[name]
        x = c['xyz']
        assert np.array_equal(x * 8, np.rint(x * 8))                                              # multiples of voxel / 2: exact
        assert (np.rint(x * 8).astype(np.int64) % 2 == 0).mean() > 0.4                            # ... half of them ON a face
        zero = x[:, 0] == 0
        assert x[:, 0].min() == 0 and zero.sum() > 100 and np.signbit(x[zero, 0]).all()           # the minimum along x is -0.0
        assert np.signbit(x[x[:, 2] == 0, 2]).any() and not np.signbit(x[x[:, 2] == 0, 2]).all()
        assert x[:, 1].min() == -5.0
        assert (c['rgb'] == 255).all(1).mean() > 0.4 and (c['labels'] == c['n_labels']).mean() > 0.3
        assert (c['objects'] == c['n_objects']).mean() > 0.3 and c['labels'].max() == 8 and c['objects'].max() == 40
    c = cases['n262144_eight_voxels_saturated']
    out = P.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], 8, 40)
    assert len(out[0]) == 8 and (out[1] == 255).all() and out[2][:, 8].sum() == 262_144 and out[3][:, 40].sum() == 262_144
    c = cases['n1']
    out = P.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], 8, 40)
    assert out[0].tolist() == [[3.125, -7.5, 0.25]] and out[1].tolist() == [[255] * 3] and out[2][0, 8] == 1 and out[3][0, 40] == 1


def test_prune_restatement_known_answer_on_faces_and_negative_zero():
    """Seven points, voxel 0.25, minimum (-0.0 | 0.0, 0.5, -1.0).  Bins floor((x - min) / 0.25):
       p0 ( 0.0,   0.5,   -1.0  ) -> (0,0,0)    p1 (-0.0, 0.5, -1.0) -> (0,0,0)    p2 (0.25, 0.5, -1.0) -> (1,0,0)  [on the face x = 0.25]
       p3 ( 0.125, 0.625, -0.875) -> (0,0,0)    p4 (0.375, 0.5, -0.75) -> (1,0,1)  [on the face z = -0.75]
       p5 ( 0.5,   0.75,  -1.0  ) -> (2,1,0)    p6 (0.25, 0.5, -0.875) -> (1,0,0)
    voxels in the order of their first point: {p0, p1, p3}, {p2, p6}, {p4}, {p5}."""
    c = {x['name']: x for x in C.prune_cases()}['on_face_known_answer']
    assert np.signbit(c['xyz'][1, 0]) and not np.signbit(c['xyz'][0, 0])
    x, rgb, lab, obj = P.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], c['n_labels'], c['n_objects'])
    want = np.array([[0.125, 0.5 + 0.5 + 0.625, -1.0 - 1.0 - 0.875], [0.75, 1.5, -2.8125], [1.125, 1.5, -2.25], [1.5, 2.25, -3.0]], np.float32)
    want[1:] /= np.float32(3.0)                                                    # (exact sums; rows 1-3 written as 3 x the value)
    want[0] /= np.float32(3.0)
    want[1] = [0.25, 0.5, -0.9375]
    assert x.dtype == np.float32 and np.array_equal(x, want)
    assert not np.signbit(x[0, 0])
    assert rgb.tolist() == [[255] * 3] * 4
    assert lab.tolist() == [[0, 0, 3], [1, 0, 1], [0, 1, 0], [0, 0, 1]]
    assert obj.tolist() == [[1, 0, 0, 2], [0, 0, 0, 2], [0, 0, 0, 1], [0, 1, 0, 0]]
