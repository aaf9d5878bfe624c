"""`interpolate_labels` with the reference's signature (partition/provider.py:681-687): the labels of a pruned cloud carried to
the full cloud through the 1-nearest neighbour, found on the device (csrc/spg_knn.hip; sklearn's kd-tree in the reference).
Ties between equidistant points go to the lowest index.
`perfect_prediction` (:689-695) and `reduced_labels2full` (:630-635): the majority label of every component and labels of
components carried to their vertices (csrc/spg_parteval.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .graphs import _dev

_HOST_CHUNK = 1 << 24          # query rows uploaded at a time: query sets larger than device memory stream through


def interpolate_labels(xyz_up, xyz, labels, ver_batch):
    """interpolate the labels of the pruned cloud to the full cloud.  labels [n] or label histograms [n, c] (argmax first);
    ver_batch is accepted and ignored, as in the reference."""
    del ver_batch
    labels = np.asarray(labels)
    if len(labels.shape) > 1 and labels.shape[1] > 1:
        labels = np.argmax(labels, axis=1)
    labels = labels.reshape(-1)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    xyz_up = np.ascontiguousarray(xyz_up, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz_up.ndim != 2 or xyz_up.shape[1] != 3:
        raise ValueError('interpolate_labels: xyz_up [m, 3] and xyz [n, 3] expected')
    if len(labels) != len(xyz):
        raise ValueError(f'interpolate_labels: {len(labels)} labels for {len(xyz)} points')
    if not (np.all(np.isfinite(xyz)) and np.all(np.isfinite(xyz_up))):
        raise ValueError('Input contains NaN or infinity.')
    dev = _dev()
    m = len(xyz_up)
    index = ops.KnnIndex(ops.upload(torch.from_numpy(xyz), dev), query_capacity=min(max(m, 1), _HOST_CHUNK))
    neighbor = np.empty(m, dtype=np.int64)
    for a in range(0, m, _HOST_CHUNK):
        q = ops.upload(torch.from_numpy(xyz_up[a:a + _HOST_CHUNK]), dev)
        idx, _ = index.query(q, 1, distances=False)
        neighbor[a:a + len(q)] = idx.reshape(-1).cpu().numpy()
    return labels[neighbor].flatten()


def _membership(components, n_ver, in_component):
    """(in_component int32 [n_ver] with the vertices of no component in an extra component len(components), n_com + 1)."""
    n_com = len(components)
    if in_component is None:
        comp = np.full(n_ver, n_com, dtype=np.int32)
        for i, c in enumerate(components):
            comp[np.asarray(c, dtype=np.int64)] = i
    else:
        comp = np.ascontiguousarray(in_component.cpu().numpy() if torch.is_tensor(in_component) else in_component).astype(np.int32)
        if comp.shape != (n_ver,):
            raise ValueError(f'in_component must be [{n_ver}], got {comp.shape}')
    return comp, n_com + 1


def perfect_prediction(components, labels, in_component=None):
    """assign each superpoint with the majority label: labels [n, C + 1] label histograms (column 0 = unlabelled) -> uint32 [n],
    the first arg-max of the summed histograms of the vertex's component; vertices in no component keep 0.  components is the
    list of vertex index arrays (disjoint); with in_component (its membership vector) the list is only counted."""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[1] < 2:
        raise ValueError('perfect_prediction: labels [n, C + 1] expected')
    n = labels.shape[0]
    comp, n_com = _membership(components, n, in_component)
    dev = _dev()
    index = ops.PartitionIndex(ops.upload(torch.from_numpy(comp), dev), n_com)
    out = ops.component_label_majority(index, ops.upload(torch.from_numpy(np.ascontiguousarray(labels).astype(np.int32)), dev))
    full_pred = out['full_pred'].cpu().numpy().astype(np.uint32)
    full_pred[comp == n_com - 1] = 0
    return full_pred


def reduced_labels2full(labels_red, components, n_ver, in_component=None):
    """distribute the labels of superpoints to their respective points -> uint8 [n_ver]; vertices in no component keep 0."""
    comp, n_com = _membership(components, n_ver, in_component)
    red = np.zeros(n_com, dtype=np.uint8)
    red[:n_com - 1] = np.asarray(labels_red).reshape(-1)[:n_com - 1]
    return red[comp]
