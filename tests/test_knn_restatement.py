"""CPU: the float64 restatement of the device kNN order (tests/knn_restatement.py) against the REFERENCE's kNN graphs
(tests/golden/knn_graph.npz, written by tools/gen_knn_golden.py from partition/graphs.py with scikit-learn's kd-tree):
distances bit for bit, targets equal outside groups of equal distance, and inside such a group the same distance at every
position.  This pins the comparator the GPU tests use to the reference without the GPU machine reading the reference."""
import os

import numpy as np
import pytest

import knn_restatement as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'knn_graph.npz'))


def check_rows(xyz, tgt, dist, k, idx_r, d2_r):
    n = len(xyz)
    tgt = tgt.reshape(n, k).astype(np.int64)
    dist = dist.reshape(n, k)
    assert np.array_equal(R.dist32(d2_r).view(np.uint32), dist.view(np.uint32)), 'distances differ'
    # the reference's own neighbours sit at the restated distance (ties may be ordered differently)
    ar = np.arange(n)[:, None]
    d2_ref = R.d2_rows(xyz, xyz)[ar, tgt]
    assert np.array_equal(d2_ref, d2_r), 'reference neighbours at other keys'
    differ = tgt != idx_r
    d2_all = R.d2_rows(xyz, xyz)
    for i, j in zip(*np.nonzero(differ)):            # only inside groups of equal distance (or a dropped duplicate of self)
        assert np.sum(d2_all[i] == d2_r[i, j]) > 1, (i, j)
    return int(differ.any(1).sum())


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_restatement_matches_reference_graph(golden, tag):
    xyz = golden[f'{tag}_xyz']
    idx_r, d2_r = R.knn(xyz, 45)
    tied = check_rows(xyz, golden[f'{tag}_nn2_target2'], np.sqrt(R.d2_rows(xyz, xyz)[np.arange(len(xyz))[:, None],
                      golden[f'{tag}_nn2_target2'].reshape(len(xyz), 45).astype(np.int64)]).astype(np.float32), 45, idx_r, d2_r)
    check_rows(xyz, golden[f'{tag}_nn2_target'], golden[f'{tag}_nn2_distances'], 10, idx_r[:, :10], d2_r[:, :10])
    check_rows(xyz, golden[f'{tag}_nn1_target'], golden[f'{tag}_nn1_distances'], 10, idx_r[:, :10], d2_r[:, :10])
    assert np.array_equal(golden[f'{tag}_nn2_source'], np.repeat(np.arange(len(xyz), dtype=np.uint32), 10))
    assert not np.any(idx_r == np.arange(len(xyz))[:, None]), 'self loop'
    if tag == 'b':
        assert tied > 0                                  # the grid-snapped cloud does exercise ties


def test_restatement_interpolate_labels(golden):
    xyz, up, hist = golden['interp_xyz'], golden['interp_up'], golden['interp_hist']
    idx, d2 = R.knn(xyz, 1, query=up)
    mine = np.argmax(hist, axis=1)[idx[:, 0]]
    d2_all = R.d2_rows(up, xyz)
    unique = (d2_all == d2[:, :1]).sum(1) == 1
    assert unique.mean() > 0.9
    assert np.array_equal(mine[unique], golden['interp_labels'][unique])
