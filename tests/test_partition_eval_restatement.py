"""The numpy restatements of tests/partition_eval_restatement.py against the REFERENCE's recorded results
(tests/golden/partition_eval.npz, written by tools/gen_parteval_golden.py): integer arrays equal, SEAL weights bit for bit,
boundary recall / precision as equal float64.  CPU only; the GPU tests use the restatements at sizes the record does not have."""
import os
import types

import numpy as np
import pytest

import partition_eval_restatement as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'partition_eval.npz'))


def scene(g):
    pred = g['pred_in_component']
    return g['src'].astype(np.int64), g['tgt'].astype(np.int64), len(pred), pred, int(pred.max()) + 1


def test_record_is_not_degenerate(golden):
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    E = len(src)
    assert list(g['tolerances'][:3]) == [0, 1, 2]
    for tol in g['tolerances']:
        for name, start in (('relaxed_pred', g['pred_transition']), ('relaxed_trans', g['is_transition'])):
            r = g[f'{name}_{tol}']
            assert r.dtype == start.dtype
            if tol == 0:
                assert np.array_equal(r, start)
            else:
                assert int((start != 0).sum()) < int((r != 0).sum()) < E
    assert len(np.unique(g['w_seal'])) >= 5
    sums = R.label_majority(pred, n_com, g['labels'])[0]
    top = np.sort(sums, 1)[:, ::-1]
    assert ((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).any(), 'no label tie'
    assert (sums.sum(1) == 0).any(), 'no component without labels'
    assert (g['labels'][:, 1:].sum(1) == 0).mean() > 0.02


def test_partition_index(golden):
    src, tgt, n, pred, n_com = scene(golden)
    order, offsets, size = R.partition_index(pred, n_com)
    for c in range(n_com):
        assert np.array_equal(order[offsets[c]:offsets[c + 1]], np.flatnonzero(pred == c))
        assert size[c] == (pred == c).sum()
    with pytest.raises(IndexError):
        R.partition_index(pred, n_com - 1)


def test_majority_confusion_ooa(golden):
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    sums, label_com, full_pred, confusion = R.label_majority(pred, n_com, g['labels'])
    assert full_pred.dtype == np.uint32 and np.array_equal(full_pred, g['full_pred'])
    assert confusion.dtype == np.int64 and np.array_equal(confusion, g['confusion'])
    assert confusion.sum() == g['labels'][:, 1:].astype(np.int64).sum()
    ooa = R.ooa(pred, n_com, g['labels'])
    assert isinstance(ooa, np.float64) and ooa == g['ooa']


def test_mode_and_seal_weights(golden):
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    freq, value = R.component_mode(pred, n_com, g['objects'])
    assert np.array_equal(freq, g['mode_freq']) and np.array_equal(value, g['mode_value'])
    w = R.seal_weights(src, tgt, pred, n_com, g['objects'], g['is_transition'], float(g['seal_factor']))
    assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), g['w_seal'].view(np.uint32))
    # a skipped id is an empty component; the smallest of the most frequent values wins
    freq, value = R.component_mode(np.array([0, 0, 2, 2, 2, 2]), 3, np.array([7, 3, 9, 5, 9, 5]))
    assert freq.tolist() == [1, 0, 2] and value.tolist() == [3, -1, 5]


def test_relaxation_and_boundary_scores(golden):
    g = golden
    src, tgt, n, pred, n_com = scene(g)
    for tol in g['tolerances']:
        tol = int(tol)
        rp = R.relax(g['pred_transition'], src, tgt, n, tol)
        rt = R.relax(g['is_transition'], src, tgt, n, tol)
        assert rp.dtype == np.bool_ and np.array_equal(rp, g[f'relaxed_pred_{tol}'])
        assert rt.dtype == np.uint8 and np.array_equal(rt, g[f'relaxed_trans_{tol}'])
        br, bp = R.boundary_counts(g['is_transition'], rp), R.boundary_counts(rt, g['pred_transition'])
        assert np.array_equal(br, g[f'br_counts_{tol}']) and np.array_equal(bp, g[f'bp_counts_{tol}'])
        assert R.boundary_recall(br) == g[f'br_{tol}'] and R.boundary_precision(bp) == g[f'bp_{tol}']
        s = R.partition_scores(src, tgt, n, pred, n_com, g['is_transition'], g['labels'], tol)
        assert np.array_equal(s['br_counts'], br) and np.array_equal(s['bp_counts'], bp)
        if tol:
            sym = R.relax(g['pred_transition'], src, tgt, n, tol, 'symmetric')
            assert (sym & ~rp).sum() > 0, 'the two rules must differ on the record'


def test_symmetric_rule_on_a_path():
    n = 41
    src, tgt = np.arange(n - 1), np.arange(1, n)
    b = np.zeros(n - 1, bool)
    b[20] = True
    for tol in range(5):
        r = R.relax(b, src, tgt, n, tol, 'symmetric')
        assert np.flatnonzero(r).tolist() == list(range(20 - tol, 21 + tol))
    assert np.isnan(R.boundary_recall(R.boundary_counts(np.zeros(4, bool), np.ones(4, bool))))
    with pytest.raises(ValueError):
        R.relax(np.ones(1, bool), np.array([0]), np.array([1]), 2, 1)


def test_seal_without_partition_still_not_implemented():
    import torch
    from superpoint_graph_amd.supervized_partition import losses
    args = types.SimpleNamespace(loss_weight='seal', transition_factor=5, k_nn_adj=5)
    with pytest.raises(NotImplementedError, match='libcp is not part of this package'):
        losses.compute_weight_loss(args, torch.zeros(3, 4), None, np.array([0, 1]), np.array([1, 2]), torch.zeros(2, dtype=torch.uint8), None, False)
    for name in ('compute_weights_SEAL', 'mode', 'relax_edge_binary'):
        assert callable(getattr(losses, name))
