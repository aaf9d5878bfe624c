"""GPU: exact k-nearest neighbours (csrc/spg_knn.hip through ops.knn, partition/graphs.compute_graph_nn*, and
partition/provider.interpolate_labels).

* against the REFERENCE's graphs (tests/golden/knn_graph.npz): source and distances bit-exact, targets equal outside groups of
  equal distance, inside them at the reference's distance and in (d2, index) order;
* against the float64 restatement (tests/knn_restatement.py) on sampled rows of a 200 000-point cloud with planes, lines, exact
  duplicates, a grid-snapped region and a 1e5 coordinate offset at millimetre spacing;
* invariance to the cell size, determinism, edge cases, the prune -> kNN -> geof chain and interpolate_labels."""
import os

import numpy as np
import pytest
import torch

import knn_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'knn_graph.npz'))


def assert_rows(xyz, idx, dist, rows=None, query=None):
    """device rows == restatement rows: indices, float32 distances, no self loops."""
    k = idx.shape[1]
    idx_r, d2_r = R.knn(xyz, k, query=query, rows=rows)
    sel = slice(None) if rows is None else rows
    assert np.array_equal(idx[sel].astype(np.int64), idx_r)
    if dist is not None:
        assert np.array_equal(dist[sel].view(np.uint32), R.dist32(d2_r).view(np.uint32))
    if query is None:
        r = np.arange(len(xyz)) if rows is None else rows
        assert not np.any(idx[sel] == r[:, None])


def big_cloud(n=200_000, seed=3):
    rng = np.random.default_rng(seed)
    parts = []
    m = n // 5
    parts.append(np.stack([rng.uniform(0, 20, m), rng.uniform(0, 20, m), np.zeros(m)], 1))            # plane
    parts.append(np.stack([rng.uniform(0, 20, m), np.full(m, 3.0), np.full(m, 1.0)], 1))               # line
    g = rng.integers(0, 40, size=(m, 3)) * 0.05                                                        # grid-snapped
    parts.append(g + np.array([5.0, 5.0, 2.0]))
    s = np.stack([rng.uniform(0, 2, m), rng.uniform(0, 2, m), rng.uniform(0, 0.01, m)], 1)            # Semantic3D-like
    parts.append(s + np.array([1e5, 2e5, 10.0]))
    rest = n - 4 * m
    parts.append(np.stack([rng.uniform(0, 20, rest), 0.5 * rng.uniform(0, 20, rest), rng.uniform(0, 20, rest)], 1))
    xyz = np.concatenate(parts).astype(np.float32)
    dup = rng.choice(n, 2000, replace=False)
    xyz[dup[:1000]] = xyz[dup[1000:]]                                                                  # exact duplicates
    return xyz


def test_graphs_vs_reference_golden(hip, golden):
    from superpoint_graph_amd.partition import graphs
    for tag in ('a', 'b'):
        xyz = golden[f'{tag}_xyz']
        g2, t2 = graphs.compute_graph_nn_2(xyz, 10, 45)
        g1 = graphs.compute_graph_nn(xyz, 10)
        assert g2['is_nn'] is True and g1['is_nn'] is True
        n = len(xyz)
        for g, pre in ((g2, 'nn2'), (g1, 'nn1')):
            assert set(g) == {'is_nn', 'source', 'target', 'distances'}
            for k in ('source', 'target', 'distances'):
                ref = golden[f'{tag}_{pre}_{k}']
                assert g[k].dtype == ref.dtype and g[k].shape == ref.shape, (tag, pre, k)
            assert np.array_equal(g['source'], golden[f'{tag}_{pre}_source'])
            assert np.array_equal(g['distances'].view(np.uint32), golden[f'{tag}_{pre}_distances'].view(np.uint32))
        assert t2.dtype == np.uint32 and t2.shape == golden[f'{tag}_nn2_target2'].shape
        d2_all = R.d2_rows(xyz, xyz)
        for mine, ref, k in ((t2, golden[f'{tag}_nn2_target2'], 45), (g2['target'], golden[f'{tag}_nn2_target'], 10),
                             (g1['target'], golden[f'{tag}_nn1_target'], 10)):
            mine, ref = mine.reshape(n, k).astype(np.int64), ref.reshape(n, k).astype(np.int64)
            ar = np.arange(n)[:, None]
            assert np.array_equal(d2_all[ar, mine], d2_all[ar, ref])        # same distance at every position
            for i, j in zip(*np.nonzero(mine != ref)):                        # differences only inside tie groups
                assert np.sum(d2_all[i] == d2_all[i, mine[i, j]]) > 1
            assert_rows(xyz, mine, None)                                      # and in (self, d2, index) order


def test_knn_vs_restatement_200k(hip):
    from superpoint_graph_amd import ops
    xyz = big_cloud()
    x = torch.from_numpy(xyz).cuda()
    idx, dist = ops.knn(x, 45)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    rows = np.random.default_rng(0).choice(len(xyz), 1500, replace=False)
    rows = np.concatenate([rows, np.arange(160_000, 160_300)])               # the offset region
    assert_rows(xyz, idx, dist, rows)
    i1, d1 = ops.knn(x, 1)
    assert np.array_equal(i1.cpu().numpy()[:, 0], idx[:, 0])
    assert np.array_equal(d1.cpu().numpy()[:, 0].view(np.uint32), dist[:, 0].view(np.uint32))


def spaced_cloud(n, seed):
    """planes, a line, a grid-snapped block and a sparse volume over ~20 units, no offset: point spacing 0.05 - 1."""
    rng = np.random.default_rng(seed)
    m = n // 4
    parts = [np.stack([rng.uniform(0, 8, m), rng.uniform(0, 8, m), np.zeros(m)], 1),
             np.stack([rng.uniform(0, 20, m), np.full(m, 3.0), np.full(m, 1.0)], 1),
             rng.integers(0, 12, size=(m, 3)) * 0.25 + np.array([5.0, 5.0, 2.0]),
             np.stack([rng.uniform(0, 20, n - 3 * m), rng.uniform(0, 10, n - 3 * m), rng.uniform(0, 20, n - 3 * m)], 1)]
    xyz = np.concatenate(parts).astype(np.float32)
    dup = rng.choice(n, 400, replace=False)
    xyz[dup[:200]] = xyz[dup[200:]]
    return xyz


def check_invariance(xyz, k, cell_sizes, min_rings):
    from superpoint_graph_amd import ops
    x = torch.from_numpy(xyz).cuda()
    ref_i, ref_d = [t.cpu().numpy() for t in ops.knn(x, k)]
    # the tiny cell makes lanes walk many Chebyshev rings: the slab bound and the strict stop rule decide every row
    assert float(ref_d[:, -1].max()) / min(cell_sizes) >= min_rings
    for cs in cell_sizes + [float((xyz.max(0) - xyz.min(0)).max()) * 4]:
        i, d = [t.cpu().numpy() for t in ops.knn(x, k, cell_size=cs)]
        assert np.array_equal(i, ref_i) and np.array_equal(d.view(np.uint32), ref_d.view(np.uint32)), cs
    again = [t.cpu().numpy() for t in ops.knn(x, k)]
    assert np.array_equal(again[0], ref_i) and np.array_equal(again[1].view(np.uint32), ref_d.view(np.uint32))
    return ref_i, ref_d


def test_cell_size_invariance_and_determinism(hip):
    from superpoint_graph_amd.partition import graphs
    xyz = spaced_cloud(20_000, seed=5)
    ref_i, ref_d = check_invariance(xyz, 20, [0.07, 0.37], min_rings=10)
    g, t2 = graphs.compute_graph_nn_2(xyz, 5, 20)
    assert np.array_equal(t2.reshape(-1, 20).view(np.int32), ref_i)
    assert np.array_equal(g['distances'].reshape(-1, 5).view(np.uint32), ref_d[:, :5].view(np.uint32))
    assert_rows(xyz, ref_i, ref_d, np.arange(0, 20_000, 37))


def test_cell_size_invariance_at_a_large_offset(hip):
    # Semantic3D-like: 1e5 offset (float32 spacing 2^-7 there), points a few millimetres to centimetres apart
    rng = np.random.default_rng(8)
    n = 6000
    xyz = (np.stack([rng.uniform(0, 2, n), rng.uniform(0, 2, n), rng.uniform(0, 0.01, n)], 1) +
           np.array([1e5, 2e5, 10.0])).astype(np.float32)
    i, d = check_invariance(xyz, 10, [0.004, 0.03], min_rings=8)
    assert_rows(xyz, i, d, np.arange(0, n, 23))


def test_isolated_points_far_from_the_cloud(hip):
    # points hundreds of cells away from everything else: the rings between them and the cloud are empty and are jumped
    from superpoint_graph_amd import ops
    xyz = spaced_cloud(20_000, seed=9)
    far = np.array([[400.0, 5.0, 5.0], [-300.0, -250.0, 8.0], [10.0, 5.0, 350.0], [401.0, 5.5, 5.0]], dtype=np.float32)
    xyz = np.concatenate([xyz[:10_000], far, xyz[10_000:]])
    x = torch.from_numpy(xyz).cuda()
    i, d = [t.cpu().numpy() for t in ops.knn(x, 10)]
    rows = np.concatenate([np.arange(10_000, 10_004), np.arange(0, len(xyz), 211)])
    assert_rows(xyz, i, d, rows)
    i2, d2 = [t.cpu().numpy() for t in ops.knn(x, 10, cell_size=0.5)]
    assert np.array_equal(i, i2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    q = np.array([[900.0, 900.0, 0.0], [-500.0, 3.0, 2.0], [5.0, 5.0, -700.0]], dtype=np.float32)    # far queries
    iq, dq = [t.cpu().numpy() for t in ops.knn(x, 10, query_xyz=torch.from_numpy(q).cuda())]
    assert_rows(xyz, iq, dq, query=q)


def test_query_set_in_several_chunks(hip):
    from superpoint_graph_amd import ops
    rng = np.random.default_rng(4)
    ref = rng.uniform(0, 10, size=(1000, 3)).astype(np.float32)
    q = rng.uniform(-1, 11, size=(200_000, 3)).astype(np.float32)
    index = ops.KnnIndex(torch.from_numpy(ref).cuda(), query_capacity=1000)
    m = index.query_chunk(len(q))
    n_chunks = -(-len(q) // m)
    assert 64 <= m <= 1000 and n_chunks >= 100 and len(q) % m != 0        # many chunks and a short last one
    i, d = [t.cpu().numpy() for t in index.query(torch.from_numpy(q).cuda(), 5)]
    starts = np.arange(0, len(q), m)
    rows = np.unique(np.concatenate([starts, np.minimum(starts + m - 1, len(q) - 1), np.arange(len(q) - 50, len(q)),
                                     rng.choice(len(q), 1500, replace=False)]))
    assert_rows(ref, i, d, rows, query=q)
    i1, d1 = [t.cpu().numpy() for t in ops.knn(torch.from_numpy(ref).cuda(), 5, query_xyz=torch.from_numpy(q).cuda())]
    assert ops.KnnIndex(torch.from_numpy(ref).cuda(), query_capacity=len(q)).query_chunk(len(q)) == len(q)   # one chunk
    assert np.array_equal(i, i1) and np.array_equal(d.view(np.uint32), d1.view(np.uint32))


def test_edge_cases(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.partition import graphs
    rng = np.random.default_rng(1)
    xyz = rng.normal(size=(11, 3)).astype(np.float32)                          # n = k + 1
    g = graphs.compute_graph_nn(xyz, 10)
    assert_rows(xyz, g['target'].reshape(11, 10).view(np.int32), g['distances'].reshape(11, 10))
    same = np.full((300, 3), 1.5, dtype=np.float32)                            # all identical: by index, self dropped
    i, d = [t.cpu().numpy() for t in ops.knn(torch.from_numpy(same).cuda(), 7)]
    for r in (0, 5, 299):
        assert list(i[r]) == [j for j in range(9) if j != r][:7]
    assert not d.any()
    line = np.stack([np.arange(500) * 0.1, np.zeros(500), np.zeros(500)], 1).astype(np.float32)   # collinear
    i, d = [t.cpu().numpy() for t in ops.knn(torch.from_numpy(line).cuda(), 6)]
    assert_rows(line, i, d)
    with pytest.raises(ValueError):
        graphs.compute_graph_nn(xyz, 11)                                      # n <= k
    with pytest.raises(AssertionError):
        graphs.compute_graph_nn_2(xyz, 5, 3)
    with pytest.raises(NotImplementedError):
        graphs.compute_graph_nn_2(xyz, 3, 5, voronoi=1.0)
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        graphs.compute_graph_nn(bad, 3)
    with pytest.raises(ValueError):
        ops.knn(torch.from_numpy(bad).cuda(), 3)
    index = ops.KnnIndex(torch.from_numpy(line).cuda())
    for v in (np.nan, np.inf, -np.inf):
        badq = line[:10].copy()
        badq[4, 2] = v
        with pytest.raises(ValueError):
            index.query(torch.from_numpy(badq).cuda(), 3)
        i, d = [t.cpu().numpy() for t in index.query(torch.from_numpy(line[:10].copy()).cuda(), 3)]
        assert_rows(line, i, d, query=line[:10])
    badref = line.copy()
    badref[7, 0] = -np.inf
    with pytest.raises(ValueError):
        ops.knn(torch.from_numpy(badref).cuda(), 3)
    big = rng.normal(size=(100, 3)).astype(np.float32)
    with pytest.raises(ValueError, match='limit'):
        ops.knn(torch.from_numpy(big).cuda(), ops.KNN_MAX_K + 1)


def test_prune_knn_geof_chain(hip, golden):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.partition import graphs, libply_c
    xyz = golden['a_xyz']
    n = len(xyz)
    # the host chain: the reference's target fed to compute_geof; rows whose 45-neighbour SET differs (a tie at the 45th
    # position) are left out, the rest agree up to the float64 summation order of the covariance
    _, t2 = graphs.compute_graph_nn_2(xyz, 10, 45)
    f_dev = libply_c.compute_geof(xyz, t2, 45)
    t_ref = golden['a_nn2_target2']
    f_ref = libply_c.compute_geof(xyz, t_ref, 45)
    same = np.array([set(a) == set(b) for a, b in zip(t2.reshape(n, 45), t_ref.reshape(n, 45))])
    assert same.mean() > 0.95
    assert np.abs(f_dev[same] - f_ref[same]).max() < 1e-5
    # prune -> kNN -> geof, all on the device, against the numpy-level entry points on the pruned cloud
    x = torch.from_numpy(xyz).cuda()
    px, _, _, _ = ops.prune(x, 0.05)
    idx, _ = ops.knn(px, 45, distances=False)
    geof = ops.compute_geof(px, idx.reshape(-1), 45)
    assert geof.is_cuda and idx.is_cuda and idx.dtype == torch.int32
    ph = px.cpu().numpy()
    _, t2p = graphs.compute_graph_nn_2(ph, 10, 45)
    assert np.array_equal(t2p.view(np.int32), idx.cpu().numpy().reshape(-1))
    assert np.array_equal(geof.cpu().numpy(), libply_c.compute_geof(ph, t2p, 45))


def test_interpolate_labels(hip, golden):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.partition import provider
    xyz, up, hist = golden['interp_xyz'], golden['interp_up'], golden['interp_hist']
    lab = provider.interpolate_labels(up, xyz, hist, 1000)
    lab1 = provider.interpolate_labels(up, xyz, np.argmax(hist, axis=1), 1000)          # 1-D labels
    assert np.array_equal(lab, lab1)
    idx_r, d2_r = R.knn(xyz, 1, query=up)
    unique = (R.d2_rows(up, xyz) == d2_r).sum(1) == 1
    assert np.array_equal(lab[unique], golden['interp_labels'][unique])
    assert np.array_equal(lab, np.argmax(hist, axis=1)[idx_r[:, 0]])                    # lowest index on exact ties
    # more queries than one internal chunk (2^22 queries): properties on sampled rows, chunk edges included
    rng = np.random.default_rng(4)
    ref = rng.uniform(0, 10, size=(20_000, 3)).astype(np.float32)
    labels = rng.integers(0, 13, size=20_000)
    q = rng.uniform(-0.5, 10.5, size=(5_000_000, 3)).astype(np.float32)
    index = ops.KnnIndex(torch.from_numpy(ref).cuda(), query_capacity=len(q))
    m = index.query_chunk(len(q))
    assert m < len(q)
    up = provider.interpolate_labels(q, ref, labels, 0)
    assert up.shape == (len(q),)
    rows = np.unique(np.concatenate([np.arange(m - 100, m + 100), np.arange(len(q) - 100, len(q)),
                                     rng.choice(len(q), 800, replace=False)]))
    idx_r, _ = R.knn(ref, 1, query=q, rows=rows)
    assert np.array_equal(up[rows], labels[idx_r[:, 0]])
