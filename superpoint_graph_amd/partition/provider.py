"""`interpolate_labels` with the reference's signature (partition/provider.py:681-687): the labels of a pruned cloud carried to
the full cloud through the 1-nearest neighbour, found on the device (csrc/spg_knn.hip; sklearn's kd-tree in the reference).
Ties between equidistant points go to the lowest index.
`perfect_prediction` (:689-695) and `reduced_labels2full` (:630-635): the majority label of every component and labels of
components carried to their vertices (csrc/spg_parteval.hip).
The raw readers `read_s3dis_format` (:185-217), `read_semantic3d_format` (:250-303) and `interpolate_labels_batch` (:637-679):
the text is parsed on the device (csrc/spg_text.hip through ops.CloudTextReader) instead of by pandas.read_csv, bit for bit
inside the grammar of ops.parse_cloud_text; a line outside it raises ValueError instead of being guessed.
Not built: read_semantic3d_format2, the ply / las / pcd readers, read_vkitti_format, the writers, exponent notation."""
from __future__ import annotations

import glob
import os

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


_WHOLE_FILE = 1 << 62        # `rows` of a CloudTextReader that yields one batch


def _read_whole(path, n_cols, xyz_cols, rgb_cols, dev):
    """(xyz, rgb | None) of every line of a text cloud, on the device."""
    for xyz, rgb, _ in ops.CloudTextReader(path, n_cols, xyz_cols, rgb_cols, rows=_WHOLE_FILE, device=dev):
        return xyz, rgb
    return (torch.empty(0, 3, dtype=torch.float32, device=dev),
            None if rgb_cols is None else torch.empty(0, 3, dtype=torch.uint8, device=dev))


def object_name_to_label(object_class):
    """convert from object name in S3DIS to an int (partition/provider.py:229-247)"""
    return {'ceiling': 1, 'floor': 2, 'wall': 3, 'column': 4, 'beam': 5, 'window': 6, 'door': 7, 'table': 8, 'chair': 9,
            'bookcase': 10, 'sofa': 11, 'board': 12, 'clutter': 13, 'stairs': 0}.get(object_class, 0)


def read_s3dis_format(raw_path, label_out=True, device=False):
    """extract data from a room folder (partition/provider.py:185-217): the room file `x y z r g b` and, with label_out, every
    Annotations/*.txt next to it in glob.glob order, all parsed on the device (ops.CloudTextReader) -> xyz float32 [n, 3], rgb
    uint8 [n, 3], room_labels uint8 [n], room_object_indices uint32 [n].  Every point of object i (1, 2, ...) gives its label
    and i to its nearest room point (one ops.KnnIndex over the room); later objects overwrite earlier ones.  Between exactly
    equidistant room points the lowest index wins (the reference leaves this to the kd-tree).  A line outside the grammar of
    ops.parse_cloud_text raises ValueError naming it; the reference's fallback to a black room on unreadable colours is not
    reproduced.  device=True: the device tensors (room_object_indices as int32)."""
    dev = _dev()
    xyz, rgb = _read_whole(raw_path, 6, (0, 1, 2), (3, 4, 5), dev)
    if not label_out:
        return (xyz, rgb) if device else (xyz.cpu().numpy(), rgb.cpu().numpy())
    n_ver = int(xyz.shape[0])
    room_labels = torch.zeros(n_ver, dtype=torch.uint8, device=dev)
    room_object_indices = torch.zeros(n_ver, dtype=torch.int32, device=dev)
    objects = glob.glob(os.path.dirname(raw_path) + "/Annotations/*.txt")
    index = ops.KnnIndex(xyz) if objects else None
    for i_object, single_object in enumerate(objects, 1):
        object_name = os.path.splitext(os.path.basename(single_object))[0]
        object_label = object_name_to_label(object_name.split('_')[0])
        obj_xyz, _ = _read_whole(single_object, 6, (0, 1, 2), None, dev)
        if obj_xyz.shape[0] == 0:
            continue
        obj_ind = index.query(obj_xyz, 1, distances=False)[0].reshape(-1).long()
        room_labels[obj_ind] = object_label
        room_object_indices[obj_ind] = i_object
    if device:
        return xyz, rgb, room_labels, room_object_indices
    return xyz.cpu().numpy(), rgb.cpu().numpy(), room_labels.cpu().numpy(), room_object_indices.cpu().numpy().astype(np.uint32)


def read_semantic3d_format(data_file, n_class, file_label_path, voxel_width, ver_batch, first_line='reference', device=False):
    """read the format of semantic3d (partition/provider.py:250-303): `x y z i r g b` lines, ver_batch at a time, each chunk pruned
    on a voxel_width grid (ops.prune) and the chunks stacked -> xyz float32 [V, 3], rgb uint8 [V, 3] and, with n_class > 0, the
    label histograms uint32 [V, n_class + 1] from the one-label-per-line file file_label_path.
    first_line, with n_class > 0 only: the reference's read_csv call for the labelled case has no header=None, so pandas
    consumes the FIRST LINE of data_file as column names: that point is lost and point k (file line k + 1) is paired with
    label line k.  'reference' (the default) reproduces exactly that; 'data' reads every line and pairs line k with label k.
    With n_class == 0 the reference passes header=None and both modes read every line.
    voxel_width <= 0 raises NotImplementedError: the reference then returns only the last chunk, with rgb = xyz (:283-286);
    read the raw rows with ops.CloudTextReader instead.  device=True: the device tensors (labels as int32)."""
    if first_line not in ('reference', 'data'):
        raise ValueError("read_semantic3d_format: first_line is 'reference' or 'data'")
    if not voxel_width > 0:
        raise NotImplementedError('read_semantic3d_format: voxel_width <= 0 makes the reference return its last chunk only, with '
                                  'rgb = xyz; iterate over ops.CloudTextReader(data_file, 7, (0, 1, 2), (4, 5, 6)) for the raw rows')
    ver_batch, n_class = int(ver_batch), int(n_class)
    if ver_batch < 1:
        raise ValueError('read_semantic3d_format: ver_batch >= 1 expected (the chunk size of the reference`s read_csv)')
    dev = _dev()
    skip = 1 if n_class > 0 and first_line == 'reference' else 0
    points = ops.CloudTextReader(data_file, 7, (0, 1, 2), (4, 5, 6), rows=ver_batch, skip_lines=skip, device=dev)
    xyz, rgb, labels = [], [], []
    if n_class > 0:
        label_lines = ops.CloudTextReader(file_label_path, 1, None, None, 0, rows=ver_batch, device=dev)
        for (xyz_full, rgb_full, _), (_, _, labels_full) in zip(points, label_lines):
            if len(labels_full) < len(xyz_full):
                raise ValueError(f'read_semantic3d_format: {len(labels_full)} labels for a chunk of {len(xyz_full)} points')
            xyz_sub, rgb_sub, labels_sub, _ = ops.prune(xyz_full, float(voxel_width), rgb_full,
                                                        labels_full[:len(xyz_full)].contiguous(), None, n_class, 0)
            xyz.append(xyz_sub); rgb.append(rgb_sub); labels.append(labels_sub)
    else:
        for xyz_full, rgb_full, _ in points:
            xyz_sub, rgb_sub, _, _ = ops.prune(xyz_full, float(voxel_width), rgb_full)
            xyz.append(xyz_sub); rgb.append(rgb_sub)
    xyz = torch.cat(xyz) if xyz else torch.empty(0, 3, dtype=torch.float32, device=dev)
    rgb = torch.cat(rgb) if rgb else torch.empty(0, 3, dtype=torch.uint8, device=dev)
    if n_class == 0:
        return (xyz, rgb) if device else (xyz.cpu().numpy(), rgb.cpu().numpy())
    labels = torch.cat(labels) if labels else torch.empty(0, n_class + 1, dtype=torch.int32, device=dev)
    if device:
        return xyz, rgb, labels
    return xyz.cpu().numpy(), rgb.cpu().numpy(), labels.cpu().numpy().astype(np.uint32)


def interpolate_labels_batch(data_file, xyz, labels, ver_batch, device=False, n_cols=7):
    """interpolate the labels of the pruned cloud to the full cloud (partition/provider.py:637-679): every line of data_file
    (n_cols fields, x y z first), ver_batch lines at a time, takes the label of its nearest point of xyz [n, 3] (one
    ops.KnnIndex; ties to the lowest index).  labels [n] or label histograms [n, c] (argmax first).  -> the labels of all lines,
    in the dtype np.hstack gives the reference: np.result_type(np.uint8, labels.dtype).
    ver_batch <= 0 raises NotImplementedError: the reference then reads the whole file, leaves its loop before the search
    and returns an empty array.  device=True: the labels as a device tensor (int64)."""
    labels = np.asarray(labels)
    if len(labels.shape) > 1 and labels.shape[1] > 1:
        labels = np.argmax(labels, axis=1)
    labels = labels.reshape(-1)
    if int(ver_batch) < 1:
        raise NotImplementedError('interpolate_labels_batch: with ver_batch <= 0 the reference returns an empty array; pass the '
                                  'chunk size (the result does not depend on it)')
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError('interpolate_labels_batch: xyz [n, 3] expected')
    if len(labels) != len(xyz):
        raise ValueError(f'interpolate_labels_batch: {len(labels)} labels for {len(xyz)} points')
    if not np.all(np.isfinite(xyz)):
        raise ValueError('Input contains NaN or infinity.')
    dev = _dev()
    index = ops.KnnIndex(ops.upload(torch.from_numpy(xyz), dev), query_capacity=min(int(ver_batch), _HOST_CHUNK))
    neighbor = [index.query(xyz_full, 1, distances=False)[0].reshape(-1).long()
                for xyz_full, _, _ in ops.CloudTextReader(data_file, int(n_cols), (0, 1, 2), rows=int(ver_batch), device=dev)]
    neighbor = torch.cat(neighbor) if neighbor else torch.empty(0, dtype=torch.int64, device=dev)
    if device:
        return ops.upload(torch.from_numpy(labels.astype(np.int64)), dev)[neighbor]
    return labels[neighbor.cpu().numpy()].astype(np.result_type(np.uint8, labels.dtype))


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
