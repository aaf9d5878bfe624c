"""Evaluation of a predicted partition and the SEAL weights on the device (csrc/spg_parteval.hip: ops.PartitionIndex /
component_label_majority / component_mode / seal_weights / relax_edges / boundary_counts / partition_scores, the
reference-signature functions of supervized_partition.losses, partition.provider and learning.metrics) against the REFERENCE's
recorded results (tests/golden/partition_eval.npz, written by tools/gen_parteval_golden.py) and, at other sizes, against the
numpy restatements pinned to that record (tests/partition_eval_restatement.py, tests/test_partition_eval_restatement.py).
Everything is exact: integer arrays equal, SEAL weights bit for bit, boundary recall / precision as equal float64."""
import os
import types

import numpy as np
import pytest
import torch

import partition_eval_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'partition_eval.npz'))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def scene(g):
    pred = g['pred_in_component']
    return g['src'].astype(np.int64), g['tgt'].astype(np.int64), len(pred), pred, int(pred.max()) + 1


def graph_of(src, tgt, n):
    from superpoint_graph_amd import ops
    return ops.EdgeGraph(dev(src, torch.int64), dev(tgt, torch.int64), n)


def check_index(index, pred, n_com):
    order, offsets, size = R.partition_index(pred, n_com)
    assert np.array_equal(host(index.order), order) and np.array_equal(host(index.offsets), offsets)
    assert np.array_equal(host(index.size), size)


def check_majority(out, pred, n_com, labels):
    sums, label_com, full_pred, confusion = R.label_majority(pred, n_com, labels)
    assert np.array_equal(host(out['sums']), sums) and np.array_equal(host(out['label_com']), label_com)
    assert np.array_equal(host(out['full_pred']).astype(np.uint32), full_pred)
    assert out['confusion'].dtype == torch.int64 and np.array_equal(host(out['confusion']), confusion)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's record
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_vs_reference(hip, golden):
    from superpoint_graph_amd import ops
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    graph = graph_of(src, tgt, n)
    index = ops.PartitionIndex(dev(pred), n_com)
    check_index(index, pred, n_com)
    out = ops.component_label_majority(index, dev(g['labels'].astype(np.int64)))
    assert np.array_equal(host(out['full_pred']).astype(np.uint32), g['full_pred'])
    assert np.array_equal(host(out['confusion']), g['confusion'])
    check_majority(out, pred, n_com, g['labels'])
    freq, value = ops.component_mode(index, dev(g['objects']))
    assert np.array_equal(host(freq), g['mode_freq']) and np.array_equal(host(value), g['mode_value'])
    w = ops.seal_weights(graph, index, dev(g['objects']), dev(g['is_transition']), float(g['seal_factor']))
    assert w.dtype == torch.float32 and bits_equal(host(w), g['w_seal'])
    for tol in g['tolerances']:
        tol = int(tol)
        rp = ops.relax_edges(graph, dev(g['pred_transition']), tol)
        rt = ops.relax_edges(graph, dev(g['is_transition']), tol)
        assert rp.dtype == torch.bool and np.array_equal(host(rp), g[f'relaxed_pred_{tol}'])
        assert rt.dtype == torch.uint8 and np.array_equal(host(rt), g[f'relaxed_trans_{tol}'])
        br = host(ops.boundary_counts(dev(g['is_transition']), rp))
        bp = host(ops.boundary_counts(rt, dev(g['pred_transition'])))
        assert br.dtype == np.int64 and np.array_equal(br, g[f'br_counts_{tol}']) and np.array_equal(bp, g[f'bp_counts_{tol}'])
        for mode in ('reference', 'symmetric'):
            r = ops.relax_edges(graph, dev(g['is_transition']), tol, mode=mode)
            assert np.array_equal(host(r), R.relax(g['is_transition'], src, tgt, n, tol, mode))


def test_reference_signatures_vs_reference(hip, golden):
    from superpoint_graph_amd.learning import metrics
    from superpoint_graph_amd.partition import provider
    from superpoint_graph_amd.supervized_partition import losses
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    comps = [np.flatnonzero(pred == c) for c in range(n_com)]
    trans, pred_trans = g['is_transition'], g['pred_transition']
    for in_component in (None, pred):
        per_pred = provider.perfect_prediction(comps, g['labels'], in_component)
        assert per_pred.dtype == np.uint32 and np.array_equal(per_pred, g['full_pred'])
        ooa = metrics.compute_OOA(comps, g['labels'], in_component)
        assert isinstance(ooa, np.float64) and ooa == g['ooa']
        full = provider.reduced_labels2full(np.arange(n_com) % 7 + 1, comps, n, in_component)
        assert full.dtype == np.uint8 and np.array_equal(full, (pred % 7 + 1).astype(np.uint8))
    # vertices in no component keep 0
    part = provider.perfect_prediction(comps[:-1], g['labels'])
    assert np.array_equal(part, np.where(pred == n_com - 1, 0, g['full_pred']))
    w = losses.compute_weights_SEAL(comps, pred, g['objects'], src, tgt, trans, int(g['seal_factor']))
    assert isinstance(w, np.ndarray) and w.dtype == np.float32 and bits_equal(w, g['w_seal'])
    for c in (0, n_com // 2, n_com - 1):
        value, freq = losses.mode(g['objects'][comps[c]])
        assert (value, freq) == (g['mode_value'][c], g['mode_freq'][c])
        assert losses.mode(g['objects'][comps[c]], only_frequency=True) == g['mode_freq'][c]
    for tol in g['tolerances']:
        tol = int(tol)
        rp = losses.relax_edge_binary(pred_trans, src, tgt, n, tol)
        rt = losses.relax_edge_binary(torch.from_numpy(trans), src, tgt, n, tol)
        assert rp.dtype == np.bool_ and np.array_equal(rp, g[f'relaxed_pred_{tol}'])
        assert rt.dtype == np.uint8 and np.array_equal(rt, g[f'relaxed_trans_{tol}'])
        br, bp = metrics.compute_boundary_recall(trans, rp), metrics.compute_boundary_precision(rt, pred_trans)
        assert isinstance(br, np.float64) and br == g[f'br_{tol}'] and bp == g[f'bp_{tol}']


def test_partition_scores_vs_pieces_and_reference(hip, golden):
    from superpoint_graph_amd import ops
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    graph = graph_of(src, tgt, n)
    for tol in g['tolerances']:
        tol = int(tol)
        s = ops.partition_scores(graph, dev(pred), n_com, dev(g['is_transition']), dev(g['labels'].astype(np.int32)), tol)
        assert s['n_clusters'] == n_com
        assert np.array_equal(host(s['confusion']), g['confusion'])
        assert np.array_equal(host(s['full_pred']).astype(np.uint32), g['full_pred'])
        assert np.array_equal(host(s['br_counts']), g[f'br_counts_{tol}']) and np.array_equal(host(s['bp_counts']), g[f'bp_counts_{tol}'])
        # the pieces
        pt = dev(g['pred_transition'])
        assert torch.equal(s['br_counts'], ops.boundary_counts(dev(g['is_transition']), ops.relax_edges(graph, pt, tol)))
        assert torch.equal(s['bp_counts'], ops.boundary_counts(ops.relax_edges(graph, dev(g['is_transition']), tol), pt))
        br = host(s['br_counts'])
        assert np.float64(100 * br[1, 1]) / np.float64(br[1, 0] + br[1, 1]) == g[f'br_{tol}']


def test_compute_weight_loss_seal(hip, golden):
    from superpoint_graph_amd.supervized_partition import losses
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    comps = [np.flatnonzero(pred == c) for c in range(n_com)]
    args = types.SimpleNamespace(loss_weight='seal', transition_factor=float(g['seal_factor']), k_nn_adj=5)
    emb = torch.zeros(n, 4, device='cuda')
    w = losses.compute_weight_loss(args, emb, dev(g['objects']), src, tgt, dev(g['is_transition']), None, False, partition=(comps, pred))
    assert w.is_cuda and w.dtype == torch.float32 and bits_equal(host(w), g['w_seal'])
    w2, pc, pic = losses.compute_weight_loss(args, emb, g['objects'], src, tgt, dev(g['is_transition']), None, True, partition=(comps, pred))
    assert bits_equal(host(w2), g['w_seal']) and pc is comps and pic is pred
    with pytest.raises(NotImplementedError):
        losses.compute_weight_loss(args, emb, dev(g['objects']), src, tgt, dev(g['is_transition']), None, False)


# ---------------------------------------------------------------------------------------------------------------------
# other sizes: the restatement
# ---------------------------------------------------------------------------------------------------------------------
def random_case(n, k, n_com, C, seed, max_object=50):
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    tgt = (src + rng.integers(1, 200, n * k)) % n
    # components: runs of vertices (so that most edges stay inside one) with 10 % of the vertices scattered
    pred = (np.arange(n, dtype=np.int64) * n_com // n)
    scatter = rng.uniform(size=n) < 0.1
    pred[scatter] = rng.integers(0, n_com, int(scatter.sum()))
    objects = (np.arange(n, dtype=np.int64) * max(n_com // 3, 1) // n) * (max_object // max(n_com // 3, 1) or 1)
    noise = rng.uniform(size=n) < 0.2
    objects[noise] = rng.integers(0, max_object + 1, int(noise.sum()))
    trans = (objects[src] != objects[tgt]).astype(np.uint8)
    labels = np.zeros((n, C + 1), np.uint32)
    labels[np.arange(n), rng.integers(0, C + 1, n)] = rng.integers(1, 9, n)
    labels[np.arange(n), rng.integers(0, C + 1, n)] += rng.integers(0, 4, n).astype(np.uint32)
    return src, tgt, pred.astype(np.int32), objects.astype(np.int32), trans, labels


@pytest.mark.parametrize('n,k,n_com,C,max_object', [
    (100_000, 5, 1, 8, 50), (100_000, 5, 37, 13, 2 ** 31 - 1), (100_000, 5, 5000, 8, 1000), (100_000, 5, 100_000, 3, 50),
    (1_000_000, 5, 2000, 8, 2 ** 31 - 1), (1_000_000, 5, 300_000, 20, 5000)])
def test_vs_restatement_at_scale(hip, n, k, n_com, C, max_object):
    from superpoint_graph_amd import ops
    src, tgt, pred, objects, trans, labels = random_case(n, k, n_com, C, seed=n_com + C, max_object=max_object)
    graph = graph_of(src, tgt, n)
    index = ops.PartitionIndex(dev(pred), n_com)
    check_index(index, pred, n_com)
    check_majority(ops.component_label_majority(index, dev(labels.astype(np.int32))), pred, n_com, labels)
    freq, value = ops.component_mode(index, dev(objects))
    rf, rv = R.component_mode(pred, n_com, objects)
    assert np.array_equal(host(freq), rf) and np.array_equal(host(value), rv)
    w = ops.seal_weights(graph, index, dev(objects), dev(trans), 5.0)
    assert bits_equal(host(w), R.seal_weights(src, tgt, pred, n_com, objects, trans, 5.0))
    pred_trans = pred[src] != pred[tgt]
    for tol, mode in ((1, 'reference'), (3, 'reference'), (2, 'symmetric')):
        assert np.array_equal(host(ops.relax_edges(graph, dev(pred_trans), tol, mode)), R.relax(pred_trans, src, tgt, n, tol, mode))
    s = ops.partition_scores(graph, dev(pred), n_com, dev(trans), dev(labels.astype(np.int32)), 2)
    r = R.partition_scores(src, tgt, n, pred, n_com, trans, labels, 2)
    for key in ('confusion', 'br_counts', 'bp_counts'):
        assert np.array_equal(host(s[key]), r[key]), key
    assert np.array_equal(host(s['full_pred']).astype(np.uint32), r['full_pred'])


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_one_component_and_singletons(hip):
    from superpoint_graph_amd import ops
    n, C = 1000, 5
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 6, (n, C + 1)).astype(np.uint32)
    values = rng.integers(0, 4, n).astype(np.int32)
    for pred, n_com in ((np.zeros(n, np.int32), 1), (rng.permutation(n).astype(np.int32), n)):
        index = ops.PartitionIndex(dev(pred), n_com)
        check_index(index, pred, n_com)
        check_majority(ops.component_label_majority(index, dev(labels.astype(np.int32))), pred, n_com, labels)
        freq, value = ops.component_mode(index, dev(values))
        rf, rv = R.component_mode(pred, n_com, values)
        assert np.array_equal(host(freq), rf) and np.array_equal(host(value), rv)
    assert host(freq).tolist() == [1] * n                                   # singletons: their own value, once


def test_skipped_component_id_and_ties(hip):
    from superpoint_graph_amd import ops
    pred = np.array([0, 0, 2, 2, 2, 2, 3], np.int32)                            # id 1 carries no vertex
    index = ops.PartitionIndex(dev(pred), 4)
    assert host(index.size).tolist() == [2, 0, 4, 1] and host(index.offsets).tolist() == [0, 2, 2, 6, 7]
    freq, value = ops.component_mode(index, dev(np.array([7, 3, 9, 5, 9, 5, 2 ** 31 - 1], np.int32)))
    assert host(freq).tolist() == [1, 0, 2, 1] and host(value).tolist() == [3, -1, 5, 2 ** 31 - 1]       # the smallest value wins
    labels = np.array([[9, 0, 2, 1], [0, 0, 0, 1], [1, 3, 0, 0], [0, 0, 0, 3], [5, 0, 0, 0], [0, 0, 0, 0], [4, 0, 0, 0]], np.int32)
    out = ops.component_label_majority(index, dev(labels))
    # component 0: classes 1 and 2 tie at 2 -> the first; 1: empty -> 0; 2: classes 0 and 2 tie at 3 -> 0; 3: unlabelled -> 0
    assert host(out['label_com']).tolist() == [1, 0, 0, 0]
    assert host(out['sums']).tolist() == [[0, 2, 2], [0, 0, 0], [3, 0, 3], [0, 0, 0]]
    assert host(out['confusion']).tolist() == [[3, 0, 0], [0, 2, 0], [3, 2, 0]]
    check_majority(out, pred, 4, labels)


@pytest.mark.parametrize('C', [1, 64])
def test_class_count_limits(hip, C):
    from superpoint_graph_amd import ops
    n, n_com = 5000, 40
    rng = np.random.default_rng(C)
    pred = rng.integers(0, n_com, n).astype(np.int32)
    labels = rng.integers(0, 3, (n, C + 1)).astype(np.uint32)
    labels[:, 1:] *= (rng.uniform(size=(n, C)) < 0.1)
    index = ops.PartitionIndex(dev(pred), n_com)
    check_majority(ops.component_label_majority(index, dev(labels.astype(np.int32))), pred, n_com, labels)


def test_tolerance_zero_two_edges_and_dtypes(hip):
    from superpoint_graph_amd import ops
    src, tgt = np.array([0, 2]), np.array([1, 3])
    graph = graph_of(src, tgt, 4)
    for b in (np.array([True, False]), np.array([1, 0], np.uint8), np.array([0, 0], np.uint8), np.array([True, True])):
        for tol in (0, 1, 2):
            for mode in ('reference', 'symmetric'):
                r = ops.relax_edges(graph, dev(b), tol, mode)
                assert r.dtype == dev(b).dtype and r.data_ptr() != dev(b).data_ptr()
                assert np.array_equal(host(r), R.relax(b, src, tgt, 4, tol, mode)), (b, tol, mode)
    # the reference's rule on two edges: nothing marked -> every source is "not marked" -> edge 0 is set
    assert host(ops.relax_edges(graph, dev(np.array([0, 0], np.uint8)), 1)).tolist() == [1, 0]
    assert host(ops.relax_edges(graph, dev(np.array([0, 0], np.uint8)), 1, 'symmetric')).tolist() == [0, 0]
    a, b = np.array([1, 0, 1, 0, 1], np.uint8), np.array([1, 1, 0, 0, 1], np.uint8)
    for x, y in ((a, b), (a != 0, b), (a, b != 0), (a != 0, b != 0)):
        assert host(ops.boundary_counts(dev(x), dev(y))).tolist() == [[1, 1], [1, 2]]


def test_no_transition_at_all_gives_nan(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import metrics
    E = 1000
    zero, one = np.zeros(E, np.uint8), np.ones(E, bool)
    assert host(ops.boundary_counts(dev(zero), dev(one))).tolist() == [[0, E], [0, 0]]
    assert np.isnan(metrics.compute_boundary_recall(zero, one))
    assert np.isnan(metrics.compute_boundary_precision(one, zero))
    assert metrics.compute_boundary_precision(zero, one) == 0.0 and metrics.compute_boundary_recall(one, one) == 100.0
    src = np.arange(E, dtype=np.int64)
    graph = graph_of(src, (src + 1) % E, E)
    s = ops.partition_scores(graph, dev(np.zeros(E, np.int32)), 1, dev(zero), dev(np.ones((E, 3), np.int32)), 2)
    # no predicted and no true transition; the reference's rule still sets edge 0 in round 1, then edge 1 and the edge into vertex 0
    assert host(s['br_counts']).tolist() == [[E - 3, 3], [0, 0]] and host(s['bp_counts']).tolist() == [[E - 3, 0], [3, 0]]


def test_symmetric_relaxation_grows_by_one_edge_per_side(hip):
    from superpoint_graph_amd import ops
    n = 200_001
    src = np.arange(n - 1, dtype=np.int64)
    graph = graph_of(src, src + 1, n)
    b = np.zeros(n - 1, np.uint8)
    b[100_000] = 1
    for tol in (1, 2, 3, 4):
        r = host(ops.relax_edges(graph, dev(b), tol, 'symmetric'))
        assert np.flatnonzero(r).tolist() == list(range(100_000 - tol, 100_001 + tol))


def test_determinism(hip):
    from superpoint_graph_amd import ops
    n, k, n_com, C = 200_000, 5, 3000, 8
    src, tgt, pred, objects, trans, labels = random_case(n, k, n_com, C, seed=11)
    graph = graph_of(src, tgt, n)

    def run():
        index = ops.PartitionIndex(dev(pred), n_com)
        maj = ops.component_label_majority(index, dev(labels.astype(np.int32)))
        freq, value = ops.component_mode(index, dev(objects))
        w = ops.seal_weights(graph, index, dev(objects), dev(trans), 5.0)
        rr = ops.relax_edges(graph, dev(trans), 3)
        rs = ops.relax_edges(graph, dev(trans), 3, 'symmetric')
        s = ops.partition_scores(graph, dev(pred), n_com, dev(trans), dev(labels.astype(np.int32)), 2)
        return [index.order, index.offsets, index.size, maj['sums'], maj['label_com'], maj['full_pred'], maj['confusion'], freq, value,
                w.view(torch.int32), rr, rs, ops.boundary_counts(dev(trans), rr), s['confusion'], s['br_counts'], s['bp_counts'], s['full_pred']]
    a, b = run(), run()
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


def test_argument_errors(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import losses
    pred = np.array([0, 1, 1, 2], np.int32)
    graph = graph_of(np.array([0, 1, 2]), np.array([1, 2, 3]), 4)
    index = ops.PartitionIndex(dev(pred), 3)
    labels = dev(np.ones((4, 3), np.int32))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.PartitionIndex(torch.from_numpy(pred), 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.component_label_majority(index, labels.cpu())
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.component_mode(index, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.relax_edges(graph, torch.zeros(3, dtype=torch.uint8), 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.boundary_counts(torch.zeros(3, dtype=torch.uint8), dev(np.zeros(3, np.uint8)))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.partition_scores(graph, torch.from_numpy(pred), 3, dev(np.zeros(3, np.uint8)), labels, 1)
    with pytest.raises(IndexError):
        ops.PartitionIndex(dev(pred), 2)
    with pytest.raises(IndexError):
        ops.PartitionIndex(dev(np.array([0, -1, 1, 2], np.int32)), 3)
    with pytest.raises(IndexError):
        ops.partition_scores(graph, dev(pred), 2, dev(np.zeros(3, np.uint8)), labels, 1)
    with pytest.raises(ValueError, match='non-negative'):
        ops.component_mode(index, dev(np.array([0, 1, -1, 2], np.int32)))
    with pytest.raises(ValueError, match='at most 64 classes'):
        ops.component_label_majority(index, dev(np.ones((4, 66), np.int32)))
    with pytest.raises(ValueError):
        ops.component_label_majority(index, dev(np.ones((5, 3), np.int32)))                    # a wrong length
    with pytest.raises(ValueError):
        ops.component_mode(index, dev(np.zeros(5, np.int32)))
    with pytest.raises(ValueError):
        ops.relax_edges(graph, dev(np.zeros(4, np.uint8)), 1)
    with pytest.raises(ValueError):
        ops.boundary_counts(dev(np.zeros(3, np.uint8)), dev(np.zeros(4, np.uint8)))
    with pytest.raises(ValueError):
        ops.seal_weights(graph, ops.PartitionIndex(dev(np.zeros(5, np.int32)), 1), dev(np.zeros(5, np.int32)), dev(np.zeros(3, np.uint8)), 5)
    with pytest.raises(ValueError, match='mode'):
        ops.relax_edges(graph, dev(np.zeros(3, np.uint8)), 1, mode='both')
    with pytest.raises(ValueError):
        ops.relax_edges(graph, dev(np.zeros(3, np.uint8)), -1)
    with pytest.raises(TypeError):
        ops.relax_edges(graph, dev(np.zeros(3, np.float32)), 1)
    one = graph_of(np.array([0]), np.array([1]), 2)
    with pytest.raises(ValueError, match='E >= 2'):
        ops.relax_edges(one, dev(np.ones(1, np.uint8)), 1)
    with pytest.raises(ValueError, match='E >= 2'):
        losses.relax_edge_binary(np.ones(1, np.uint8), np.array([0]), np.array([1]), 2, 1)
    assert host(ops.relax_edges(one, dev(np.ones(1, np.uint8)), 0)).tolist() == [1]
    assert host(ops.relax_edges(one, dev(np.zeros(1, np.uint8)), 2, 'symmetric')).tolist() == [0]
    # after the errors everything still works
    assert host(ops.PartitionIndex(dev(pred), 3).size).tolist() == [1, 2, 1]
