"""Evaluation of a predicted partition and the SEAL weights (csrc/spg_parteval.hip)."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._core import _as_vec, _indicator, _int_vec, _on_gpu, _ptr, _raise_flagged, _req, _stream, _workspace
from .edges import EdgeGraph


# --------------------------------------------------------------------------------------------------
# evaluation of a predicted partition and the SEAL weights (csrc/spg_parteval.hip; reference supervized_partition/
# supervized_partition.py:248-375, partition/provider.py:689-695, learning/metrics.py:87-108, losses.py:119-128, :168-186)
# --------------------------------------------------------------------------------------------------
PARTEVAL_MAX_CLASSES = 64
_RELAX_MODES = {'reference': 0, 'symmetric': 1}
_COMPONENT_RANGE, _NEGATIVE_VALUE = 1, 2      # bits of the flag word of spg_partition_index and spg_component_mode


def _raise_partition_flag(flag, n_com):
    _raise_flagged(int(flag.item()), {_COMPONENT_RANGE: (IndexError, f'a component id is outside [0, {n_com})'),
                                      _NEGATIVE_VALUE: (ValueError, 'values must be non-negative')})


class PartitionIndex:
    """A partition of n vertices given by in_component integer [n] (device) and n_com: order i32 [n] = the vertices by
    component, ascending inside a component (np.flatnonzero(in_component == c) is order[offsets[c]:offsets[c + 1]]), offsets
    i32 [n_com + 1], size i32 [n_com].  An id no vertex carries is a component of size 0; an id outside [0, n_com) raises
    IndexError (one host synchronisation; _flag: a device int32 the caller reads later instead)."""

    def __init__(self, in_component, n_com: int, _flag=None):
        if not torch.is_tensor(in_component) or in_component.dim() != 1:
            raise ValueError('PartitionIndex: in_component must be a [n] tensor')
        n, n_com = int(in_component.numel()), int(n_com)
        if not (1 <= n < 2 ** 31 - 1 and 1 <= n_com < 2 ** 31 - 1):
            raise ValueError(f'PartitionIndex: 1 <= n, n_com < 2^31 - 1 expected, got n = {n}, n_com = {n_com}')
        comp = _int_vec(in_component, n, torch.int32, 'in_component')
        L, dev = lib(), comp.device
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if _flag is None else _flag
        order = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n_com + 1, dtype=torch.int32, device=dev)
        size = torch.empty(n_com, dtype=torch.int32, device=dev)
        ws = _workspace(L.spg_partition_index_workspace_bytes, n, n_com, dev=dev)
        check(L.spg_partition_index(_ptr(comp), n, n_com, _ptr(order), _ptr(offsets), _ptr(size), _ptr(flag), _ptr(ws), ws.numel(),
                                    _stream()), 'spg_partition_index')
        if _flag is None:
            _raise_partition_flag(flag, n_com)
        self.n, self.n_com, self.device = n, n_com, dev
        self.in_component, self.order, self.offsets, self.size = comp, order, offsets, size


def _label_majority(index, labels):
    _on_gpu(labels, 'labels')
    if labels.dim() != 2 or labels.shape[0] != index.n or labels.shape[1] < 2:
        raise ValueError(f'labels must be [{index.n}, C + 1] (column 0 = unlabelled), got {tuple(labels.shape)}')
    C = int(labels.shape[1]) - 1
    if C > PARTEVAL_MAX_CLASSES:
        raise ValueError(f'labels: at most {PARTEVAL_MAX_CLASSES} classes, got C = {C}')
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f'labels must be an integer tensor, got {labels.dtype}')
    # uint32 counts: int32 storage holds the same 32 bits (torch has no uint32 arithmetic)
    lab = _req(labels.contiguous() if labels.dtype in (torch.int32, getattr(torch, 'uint32', torch.int32)) else labels.to(torch.int32).contiguous(), None, 'labels')
    dev, n_com = index.device, index.n_com
    sums = torch.empty(n_com, C, dtype=torch.int64, device=dev)
    label_com = torch.empty(n_com, dtype=torch.int32, device=dev)
    full_pred = torch.empty(index.n, dtype=torch.int32, device=dev)
    confusion = torch.empty(C, C, dtype=torch.int64, device=dev)
    check(lib().spg_component_label_majority(_ptr(lab), index.n, C, _ptr(index.in_component), _ptr(index.order), n_com, _ptr(sums),
                                             _ptr(label_com), _ptr(full_pred), _ptr(confusion), _stream()), 'spg_component_label_majority')
    return dict(sums=sums, label_com=label_com, full_pred=full_pred, confusion=confusion)


def component_label_majority(index: PartitionIndex, labels):
    """perfect_prediction (partition/provider.py:689-695) and its confusion matrix: labels integer [n, C + 1] per-point label
    histograms (column 0 = unlabelled, left out), C <= 64 -> dict(sums i64 [n_com, C], label_com i32 [n_com] = first arg-max
    (0 for an all-zero row), full_pred i32 [n] (the uint32 labels of the reference), confusion i64 [C, C] with
    confusion[:, label_com[c]] += sums[c, :] = ConfusionMatrix.count_predicted_batch(labels[:, 1:], full_pred))."""
    if not isinstance(index, PartitionIndex):
        raise TypeError('component_label_majority: index must be a PartitionIndex')
    return _label_majority(index, labels)


def _component_mode(in_component, values, n_com, flag):
    n = int(in_component.numel())
    vals = _int_vec(values, n, torch.int32, 'values')
    L, dev = lib(), in_component.device
    freq = torch.empty(n_com, dtype=torch.int32, device=dev)
    value = torch.empty(n_com, dtype=torch.int32, device=dev)
    ws = _workspace(L.spg_component_mode_workspace_bytes, n, n_com, dev=dev)
    check(L.spg_component_mode(_ptr(in_component), _ptr(vals), n, n_com, _ptr(freq), _ptr(value), _ptr(flag), _ptr(ws), ws.numel(),
                               _stream()), 'spg_component_mode')
    return freq, value


def component_mode(index: PartitionIndex, values):
    """mode() of every component (losses.py:168-173, metrics.py:95-100): values integer [n], 0 <= value < 2^31 ->
    (freq i32 [n_com] = count of the most frequent value, value i32 [n_com] = the smallest of the most frequent); an empty
    component gives 0 and -1.  One host synchronisation (negative values raise ValueError)."""
    if not isinstance(index, PartitionIndex):
        raise TypeError('component_mode: index must be a PartitionIndex')
    flag = torch.zeros(1, dtype=torch.int32, device=index.device)
    freq, value = _component_mode(index.in_component, values, index.n_com, flag)
    _raise_partition_flag(flag, index.n_com)
    return freq, value


def seal_weights(graph: EdgeGraph, index: PartitionIndex, objects, is_transition, factor):
    """compute_weights_SEAL (losses.py:119-128): index = the predicted partition, objects integer [n] >= 0 (the true object of
    every vertex), is_transition [E] -> weights f32 [E]: float32(1 + double(max over both ends of size - mode frequency of
    their predicted component) * factor) on transition edges (float64, rounded once), 1 elsewhere.  One host synchronisation."""
    graph._use()
    if not isinstance(index, PartitionIndex):
        raise TypeError('seal_weights: index must be a PartitionIndex')
    if index.n != graph.n:
        raise ValueError(f'seal_weights: the partition has {index.n} vertices, the graph {graph.n}')
    is_transition = _as_vec(is_transition, torch.uint8, graph.E, 'is_transition')
    flag = torch.zeros(1, dtype=torch.int32, device=index.device)
    freq, _ = _component_mode(index.in_component, objects, index.n_com, flag)
    w = torch.empty(graph.E, dtype=torch.float32, device=graph.device)
    check(lib().spg_seal_weights(_ptr(graph.ends), graph.E, graph.n, _ptr(index.in_component), _ptr(index.size), _ptr(freq), index.n_com,
                                 _ptr(is_transition), float(factor), _ptr(w), _stream()), 'spg_seal_weights')
    _raise_partition_flag(flag, index.n_com)
    return w


def _relax(graph, binary_u8, tolerance, mode_code):
    L, dev = lib(), graph.device
    out = torch.empty(graph.E, dtype=torch.uint8, device=dev)
    ws = _workspace(L.spg_relax_edges_workspace_bytes, graph.n, dev=dev)
    check(L.spg_relax_edges(_ptr(graph.ends), graph.E, graph.n, _ptr(binary_u8), tolerance, mode_code, _ptr(out), _ptr(ws), ws.numel(),
                            _stream()), 'spg_relax_edges')
    return out


def relax_edges(graph: EdgeGraph, binary, tolerance: int, mode='reference'):
    """relax_edge_binary (losses.py:175-186): binary bool / uint8 [E] -> the indicator after `tolerance` rounds of "mark both ends
    of every set edge, then set edges from the marks" (same dtype; tolerance 0 is a copy).
    mode 'symmetric': an edge is set if either of its ends is marked -- what the reference's text describes.
    mode 'reference': what the reference's function computes.  Its vertex marks are a uint8 array, so
    `relaxed_binary[transition_vertex[edg_source]] = True` is integer indexing with the values 0 and 1, not a mask: every
    round sets EDGE 1 if any edge's source is marked and EDGE 0 if any edge's source is not, and the relaxation itself spreads
    through the target ends only.  Reproduced as it is; needs E >= 2 when tolerance > 0 (ValueError), where the reference
    raises an IndexError or not, depending on the data."""
    graph._use()
    if mode not in _RELAX_MODES:
        raise ValueError(f"relax_edges: mode must be 'reference' or 'symmetric', got {mode!r}")
    tolerance = int(tolerance)
    if tolerance < 0:
        raise ValueError(f'relax_edges: tolerance >= 0 expected, got {tolerance}')
    b = _indicator(binary, graph.E, 'binary')
    if mode == 'reference' and tolerance > 0 and graph.E < 2:
        raise ValueError("relax_edges: mode 'reference' writes edges 0 and 1 and needs E >= 2")
    out = _relax(graph, b, tolerance, _RELAX_MODES[mode])
    return out.view(torch.bool) if binary.dtype == torch.bool else out


def _boundary_counts(a, b):
    counts = torch.empty(2, 2, dtype=torch.int64, device=a.device)
    check(lib().spg_boundary_counts(_ptr(a), _ptr(b), a.numel(), _ptr(counts), _stream()), 'spg_boundary_counts')
    return counts


def boundary_counts(a, b):
    """a (truth), b (prediction): bool / uint8 [E] -> counts i64 [2, 2], counts[a != 0][b != 0] (the count_predicted_batch_hard
    matrix of evaluate_final; metrics.py:87-92: recall = 100 * counts[1, 1] / (counts[1, 0] + counts[1, 1]), precision =
    100 * counts[1, 1] / (counts[0, 1] + counts[1, 1]))."""
    if not torch.is_tensor(a) or a.dim() != 1:
        raise ValueError('boundary_counts: a and b must be [E] tensors')
    E = int(a.numel())
    return _boundary_counts(_indicator(a, E, 'a'), _indicator(b, E, 'b'))


def partition_scores(graph: EdgeGraph, pred_in_component, n_com: int, is_transition, labels, tolerance: int):
    """What the body of evaluate() / evaluate_final() does with a predicted partition (supervized_partition.py:282-293,
    :335-343), on the device: -> dict(n_clusters = n_com, confusion i64 [C, C] (the ASA matrix of perfect_prediction),
    br_counts i64 [2, 2] = boundary_counts(is_transition, relaxed predicted transitions), bp_counts i64 [2, 2] =
    boundary_counts(relaxed is_transition, predicted transitions), full_pred i32 [n]); the relaxation is the reference's
    (relax_edges mode 'reference').  One host synchronisation (the range check of the component ids)."""
    graph._use()
    tolerance = int(tolerance)
    if tolerance < 0:
        raise ValueError(f'partition_scores: tolerance >= 0 expected, got {tolerance}')
    if tolerance > 0 and graph.E < 2:
        raise ValueError('partition_scores: the reference relaxation needs E >= 2')
    if not torch.is_tensor(pred_in_component) or pred_in_component.shape != (graph.n,):
        raise ValueError(f'pred_in_component must be a [{graph.n}] tensor')
    trans = _indicator(is_transition, graph.E, 'is_transition')
    dev = graph.device
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    index = PartitionIndex(pred_in_component, n_com, _flag=flag)
    maj = _label_majority(index, labels)
    pred_trans = torch.empty(graph.E, dtype=torch.uint8, device=dev)
    check(lib().spg_pred_transition(_ptr(graph.ends), graph.E, graph.n, _ptr(index.in_component), _ptr(pred_trans), _stream()),
          'spg_pred_transition')
    br = _boundary_counts(trans, _relax(graph, pred_trans, tolerance, 0))
    bp = _boundary_counts(_relax(graph, trans, tolerance, 0), pred_trans)
    _raise_partition_flag(flag, index.n_com)
    return dict(n_clusters=index.n_com, confusion=maj['confusion'], br_counts=br, bp_counts=bp, full_pred=maj['full_pred'])
