"""GPU: the partition kernels of csrc/spg_spgraph.hip (compute_geof, compute_sp_graph, prune) at their degenerate and scale
edges, element by element against the float64 references of tests/partition_cases.py (whose builders and bounds
tests/test_partition_cases.py checks on the CPU):

* compute_geof at k_nn 0 ... 150 (more than 64 KB of dynamic LDS from 64 upward), n around the workgroup size, exactly
  degenerate neighbourhoods (NaN pattern), a 1e5 offset, repeated / self neighbours: 2e-5 absolute, verticality under the
  conditioning mask, bit-identical second call;
* compute_sp_graph on components of 0 / 1 / 2 / 3 / collinear / coplanar / signed-zero / 64-lane-straddling unique points and on
  hand-built superedges of 1 / 64 / 65 / 129 edges, an edge of length exactly d_max, d_max <= 0: integers bit-exact, every float
  per element inside a bound derived from float64 perturbation, ratio rows bit-equal to graphs.py:186-190 on the device's own
  superpoint features;
* prune at 1 / 262 143 / 262 144 / 1 000 000 points on voxel faces with a -0.0 minimum: bit-exact.

`python tests/test_gpu_partition_edges.py` prints the measured figures (profiles/partition_edges_errors.txt)."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import partition_cases as C
from oracle import spg_partition_oracle as P
from test_gpu_spgraph import compare

pytestmark = pytest.mark.gpu

GEOF_NAMES = [c['name'] for c in C.geof_cases()]                # small k_nn first: an earlier result is on record before k_nn >= 64
SP_CASES = {c['name']: c for c in C.superpoint_cases() + C.superedge_cases()}
PRUNE_CASES = {c['name']: c for c in C.prune_cases()}
FEATURES = ('linearity', 'planarity', 'scattering', 'verticality')


# ---------------------------------------------------------------------------------------------------------------------
# compute_geof
# ---------------------------------------------------------------------------------------------------------------------
def geof_figures(case):
    from superpoint_graph_amd.partition import graphs
    dev = graphs.compute_geof(case['xyz'], case['target'], case['k_nn'])
    again = graphs.compute_geof(case['xyz'], case['target'], case['k_nn'])
    m = C.geof_measure(dev, case)
    m.update(shape=dev.shape, dtype=dev.dtype, repeat_equal=bool(np.array_equal(dev.view(np.uint32), again.view(np.uint32))))
    return m


@pytest.mark.parametrize('name', GEOF_NAMES)
def test_compute_geof_edges(hip, name):
    case = C.geof_cases()[GEOF_NAMES.index(name)]
    m = geof_figures(case)
    print(name, 'worst', ' '.join(f'{v:.2e}' for v in m['worst']), 'masked', f"{m['masked']:.2%}", 'nan rows', m['nan_rows'])
    assert m['shape'] == (len(case['xyz']), 4) and m['dtype'] == np.float32
    assert m['nan_equal'], 'NaN pattern differs from the reference'
    assert (m['worst'] < C.GEOF_ATOL).all(), dict(zip(FEATURES, m['worst']))
    assert m['repeat_equal'], 'second call differs'
    if case['kind'] == 'nan':
        assert m['nan_rows'] == len(case['xyz'])
    if case['kind'] == 'random':
        assert m['masked'] <= 1e-3 + (m['nan_rows'] / len(case['xyz']))


def test_compute_geof_refuses_k_nn_151(hip):
    from superpoint_graph_amd.partition import graphs
    xyz = np.random.default_rng(0).normal(size=(300, 3)).astype(np.float32)
    target = np.random.default_rng(1).integers(0, 300, 300 * 151).astype(np.uint32)
    with pytest.raises(RuntimeError, match='k_nn too large'):
        graphs.compute_geof(xyz, target, 151)
    ok = graphs.compute_geof(xyz, target[:300 * 150], 150)                          # the library still works afterwards
    assert ok.shape == (300, 4) and np.abs(ok - P.geof(xyz, target[:300 * 150], 150)).max() < C.GEOF_ATOL


# ---------------------------------------------------------------------------------------------------------------------
# compute_sp_graph
# ---------------------------------------------------------------------------------------------------------------------
def run_sp_graph(case):
    """compute_sp_graph with the reference's signature; a case with a TRAILING empty component (n_com = max + 2, which that
    signature cannot express) goes through ops.sp_graph with the wrapper's own conversions."""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.partition import graphs
    xyz, comp, n_com, labels = case['xyz'], case['comp'], case['n_com'], case['labels']
    if n_com == int(comp.max()) + 1:
        return graphs.compute_sp_graph(xyz, case['d_max'], comp, [None] * n_com, labels, case['n_labels'], tetrahedra=case['tets'])
    dev = torch.device('cuda')
    up = lambda a, t: ops.upload(torch.from_numpy(np.ascontiguousarray(a, dtype=t)), dev)
    lab = up(labels, np.int32) if len(labels) > 1 else None
    g = ops.sp_graph(up(xyz, np.float32), up(comp, np.int32), n_com, up(case['tets'], np.int32), float(case['d_max']), lab, None, case['n_labels'])
    views = {'sp_point_count': np.uint64, 'source': np.uint32, 'target': np.uint32, 'sp_labels': np.uint32}
    out = {k: (v.cpu().numpy().view(views[k]) if k in views else v.cpu().numpy()) for k, v in g.items()
           if v is not None and k not in ('edges', 'seg_off')}
    out['is_nn'] = False
    if lab is None:
        out['sp_labels'] = []
    return out


def sp_graph_figures(case):
    """-> (device result, oracle result, superpoint figures, superedge figures, names of the ratio rows that are not bit-equal)."""
    mine = run_sp_graph(case)
    ref = C.sp_graph_reference(case)
    sp = C.superpoint_measure(mine, case['xyz'], case['comp'], case['n_com'])
    se = C.superedge_measure(mine, case)
    rows = C.ratio_rows_from_own_features(mine)
    unequal = [k for k, v in rows.items() if not np.array_equal(v.reshape(mine[k].shape).view(np.uint32), mine[k].view(np.uint32))]
    return mine, ref, sp, se, unequal


@pytest.mark.parametrize('name', list(SP_CASES))
def test_sp_graph_edges(hip, name):
    case = SP_CASES[name]
    mine, ref, sp, se, unequal = sp_graph_figures(case)
    print(name, 'superpoints', {k: (f'{v[0]:.2e}', f'{v[1]:.3f}', v[2]) for k, v in sp.items()},
          'superedges', {k: (f'{v[0]:.2e}', f'{v[1]:.3f}') for k, v in se.items()})
    # integers bit-exact (compare()), including the histogram rows that lost their out-of-range labels; floats array-relative
    assert mine['is_nn'] is False
    if len(case['labels']) > 1:
        assert mine['sp_labels'].sum() == ((case['labels'] >= 0) & (case['labels'] <= case['n_labels'])).sum()
    else:
        assert mine['sp_labels'] == []
    compare({k: v for k, v in mine.items() if k in ref and k != 'is_nn' and not isinstance(ref[k], list)},
            {k: v for k, v in ref.items() if k != 'is_nn' and not isinstance(v, list)}, name)
    # every float per element
    for k, v in sp.items():
        assert v[1] <= 1.0, f'{name}: sp {k} of component {v[2]}: error {v[0]:.3e} is {v[1]:.2f} x its bound'
    for k, v in se.items():
        assert v[1] <= 1.0, f'{name}: se_delta_{k}: error {v[0]:.3e} is {v[1]:.2f} x its bound'
    assert not unequal, f'{name}: {unequal} differ from graphs.py:186-190 applied to the device\'s own superpoint features'
    for k in ('sp_length', 'sp_surface', 'sp_volume', 'sp_centroids'):
        assert not mine[k][np.bincount(case['comp'], minlength=case['n_com']) == 0].any(), 'empty component: zeros'
    if 'expect' in case:
        counts = C.superedge_stats_f64(case)['count']
        assert not mine['se_delta_std'][counts == 1].any()                           # one Delaunay edge: std exactly 0
        one = np.flatnonzero(counts == 1)[0]
        e = P.interface_edges(case['tets'], case['comp'], case['xyz'], case['d_max'])
        a, b = e[:, (case['comp'][e[0]] == mine['source'][one, 0]) & (case['comp'][e[1]] == mine['target'][one, 0])][:, 0]
        assert np.array_equal(mine['se_delta_mean'][one], case['xyz'][a] - case['xyz'][b])      # ... and the mean IS the offset
    again = run_sp_graph(case)
    for k, v in mine.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v.view(np.uint8), again[k].view(np.uint8)), f'{name}: {k} differs on a second call'


# ---------------------------------------------------------------------------------------------------------------------
# prune
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(PRUNE_CASES))
def test_prune_edges(hip, name):
    from superpoint_graph_amd.partition import libply_c
    c = PRUNE_CASES[name]
    for n_labels, n_objects in ((c['n_labels'], c['n_objects']), (c['n_labels'], 0)):
        got = libply_c.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], n_labels, n_objects)
        ref = P.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], n_labels, n_objects)
        for a, b, what in zip(got, ref, ('xyz', 'rgb', 'labels', 'objects')):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
            assert np.array_equal(a, b), f'{name}: {what} differs (n_labels {n_labels}, n_objects {n_objects})'
        assert got[2].sum() == len(c['xyz']) and got[3].sum() == (len(c['xyz']) if n_objects else 0)
        assert got[2][:, n_labels].sum() == (c['labels'] == n_labels).sum()                       # the upper-bound ids are counted
        if n_objects:
            assert got[3][:, n_objects].sum() == (c['objects'] == n_objects).sum()


def test_prune_known_answer_on_faces_and_negative_zero(hip):
    from superpoint_graph_amd.partition import libply_c
    c = PRUNE_CASES['on_face_known_answer']
    x, rgb, lab, obj = libply_c.prune(c['xyz'], c['voxel'], c['rgb'], c['labels'], c['objects'], c['n_labels'], c['n_objects'])
    third = np.float32(3.0)
    want = np.array([[np.float32(0.125) / third, np.float32(1.625) / third, np.float32(-2.875) / third], [0.25, 0.5, -0.9375],
                     [0.375, 0.5, -0.75], [0.5, 0.75, -1.0]], np.float32)
    assert np.array_equal(x.view(np.uint32), want.view(np.uint32))                                # (+0.0 + -0.0 = +0.0 included)
    assert rgb.tolist() == [[255] * 3] * 4 and lab.tolist() == [[0, 0, 3], [1, 0, 1], [0, 1, 0], [0, 0, 1]]
    assert obj.tolist() == [[1, 0, 0, 2], [0, 0, 0, 2], [0, 0, 0, 1], [0, 1, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    lines = ['compute_geof: worst |device - float64 restatement| on the comparable entries (bound 2e-5), share of points masked from verticality',
             f"{'case':34s} {'n':>7s} {'k_nn':>4s}  " + ' '.join(f'{f:>11s}' for f in FEATURES) + '  err/bound   masked  NaN rows  NaN==  repeat==']
    for case in C.geof_cases():
        m = geof_figures(case)
        lines.append(f"{case['name']:34s} {len(case['xyz']):7d} {case['k_nn']:4d}  " + ' '.join(f'{v:11.3e}' for v in m['worst']) +
                     f"  {m['worst'].max() / C.GEOF_ATOL:9.2e}  {m['masked']:7.3%}  {m['nan_rows']:8d}  {str(m['nan_equal']):5s}  {m['repeat_equal']}")
    lines += ['', 'compute_sp_graph: per element, worst absolute error | worst error / per-component (per-superedge) bound [component]']
    for name, case in SP_CASES.items():
        _, _, sp, se, unequal = sp_graph_figures(case)
        lines.append(f'{name:28s} ' + '  '.join(f'{k} {v[0]:.2e} | {v[1]:.3f} [{v[2]}]' for k, v in sp.items()))
        lines.append(f"{'':28s} " + '  '.join(f'delta_{k} {v[0]:.2e} | {v[1]:.3f}' for k, v in se.items()) +
                     f"  ratio rows not bit-equal: {unequal or 'none'}")
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
