"""`interpolate_labels` with the reference's signature (partition/provider.py:681-687): the labels of a pruned cloud carried to
the full cloud through the 1-nearest neighbour, found on the device (csrc/spg_knn.hip; sklearn's kd-tree in the reference).
Ties between equidistant points go to the lowest index."""
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
