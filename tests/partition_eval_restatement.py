"""Vectorised numpy restatements of what csrc/spg_parteval.hip computes (reference supervized_partition/losses.py:119-128
compute_weights_SEAL, :168-186 mode / relax_edge_binary, partition/provider.py:689-695 perfect_prediction, learning/metrics.py
:16-22, :87-108): no Python loop over components or edges, so they serve where the recorded reference results
(tests/golden/partition_eval.npz, written by tools/gen_parteval_golden.py) are too small.  tests/test_partition_eval_restatement.py
checks them against those records exactly."""
import numpy as np


def partition_index(in_component, n_com):
    """-> (order: the vertices by component, ascending inside one; offsets [n_com + 1]; size [n_com])."""
    comp = np.asarray(in_component).astype(np.int64)
    if comp.size and (comp.min() < 0 or comp.max() >= n_com):
        raise IndexError('component id out of range')
    order = np.argsort(comp, kind='stable').astype(np.int32)
    size = np.bincount(comp, minlength=n_com).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
    return order, offsets, size


def label_majority(in_component, n_com, labels):
    """labels [n, C + 1] -> (sums i64 [n_com, C], label_com i32 [n_com], full_pred u32 [n], confusion i64 [C, C])."""
    comp = np.asarray(in_component).astype(np.int64)
    lab = np.asarray(labels)[:, 1:].astype(np.int64)
    C = lab.shape[1]
    sums = np.zeros((n_com, C), np.int64)
    np.add.at(sums, comp, lab)
    label_com = sums.argmax(1).astype(np.int32)
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion.T, label_com, sums)               # confusion[:, label_com[c]] += sums[c, :]
    return sums, label_com, label_com[comp].astype(np.uint32), confusion


def component_mode(in_component, n_com, values):
    """-> (freq i32 [n_com], value i32 [n_com]): the count of the most frequent value of every component and the smallest of
    the most frequent; an empty component: 0 and -1."""
    comp = np.asarray(in_component).astype(np.uint64)
    val = np.asarray(values).astype(np.uint64)
    keys, counts = np.unique((comp << np.uint64(32)) | val, return_counts=True)
    kc, kv = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    o = np.lexsort((kv, -counts, kc))                      # by component, then the larger count, then the smaller value
    first = np.ones(len(o), bool)
    first[1:] = kc[o][1:] != kc[o][:-1]
    freq, value = np.zeros(n_com, np.int32), np.full(n_com, -1, np.int32)
    freq[kc[o][first]] = counts[o][first]
    value[kc[o][first]] = kv[o][first]
    return freq, value


def seal_weights(src, tgt, pred_in_component, n_com, objects, is_transition, factor):
    """float32 [E]: float32(1 + float64(max over both ends of size - freq) * factor) on transition edges, 1 elsewhere."""
    pred = np.asarray(pred_in_component).astype(np.int64)
    size = np.bincount(pred, minlength=n_com).astype(np.int64)
    freq, _ = component_mode(pred, n_com, objects)
    wpc = (size - freq).astype(np.uint32)
    t = np.asarray(is_transition) != 0
    w = np.ones(len(src), np.float32)
    w[t] = (1.0 + np.maximum(wpc[pred[src[t]]], wpc[pred[tgt[t]]]).astype(np.float64) * float(factor)).astype(np.float32)
    return w


def relax(binary, src, tgt, n, tolerance, mode='reference'):
    """The indicator after `tolerance` rounds, in the input's dtype.  'symmetric': an edge is set if either end is marked.
    'reference': an edge is set if its target is marked; edge 1 if any source is marked, edge 0 if any source is not (the
    reference indexes the edge array with its uint8 vertex marks)."""
    r = np.array(binary, copy=True)
    if mode == 'reference' and tolerance > 0 and len(r) < 2:
        raise ValueError('E >= 2')
    marks = np.zeros(n, bool)
    for _ in range(tolerance):
        on = r != 0
        marks[src[on]] = True
        marks[tgt[on]] = True
        ms, mt = marks[src], marks[tgt]
        if mode == 'symmetric':
            r[ms | mt] = True
        else:
            if ms.any():
                r[1] = True
            if not ms.all():
                r[0] = True
            r[mt] = True
    return r


def boundary_counts(a, b):
    """i64 [2, 2]: counts[a != 0][b != 0]."""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return np.bincount(a.astype(np.int64) * 2 + b, minlength=4).reshape(2, 2).astype(np.int64)


def boundary_recall(counts):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(100 * counts[1, 1]) / np.float64(counts[1, 0] + counts[1, 1])


def boundary_precision(counts):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(100 * counts[1, 1]) / np.float64(counts[0, 1] + counts[1, 1])


def ooa(in_component, n_com, labels):
    """metrics.py:102-108 with the components given by their membership vector."""
    freq, _ = component_mode(in_component, n_com, np.asarray(labels).argmax(1))
    return 100 * np.int64(freq.sum()) / len(labels)


def partition_scores(src, tgt, n, pred_in_component, n_com, is_transition, labels, tolerance):
    pred = np.asarray(pred_in_component)
    pred_trans = pred[src] != pred[tgt]
    _, _, full_pred, confusion = label_majority(pred, n_com, labels)
    return dict(n_clusters=n_com, confusion=confusion, full_pred=full_pred,
                br_counts=boundary_counts(is_transition, relax(pred_trans, src, tgt, n, tolerance)),
                bp_counts=boundary_counts(relax(is_transition, src, tgt, n, tolerance), pred_trans))
