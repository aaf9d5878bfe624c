"""`interpolate_labels` with the reference's signature (partition/provider.py:681-687): the labels of a pruned cloud carried to
the full cloud through the 1-nearest neighbour, found on the device (csrc/spg_knn.hip; sklearn's kd-tree in the reference).
Ties between equidistant points go to the lowest index.
`perfect_prediction` (:689-695) and `reduced_labels2full` (:630-635): the majority label of every component and labels of
components carried to their vertices (csrc/spg_parteval.hip).
The raw readers `read_s3dis_format` (:185-217), `read_semantic3d_format` (:250-303) and `interpolate_labels_batch` (:637-679):
the text is parsed on the device (csrc/spg_text.hip through ops.CloudTextReader) instead of by pandas.read_csv, bit for bit
inside the grammar of ops.parse_cloud_text; a line outside it raises ValueError instead of being guessed.
The ASCII PLY writers `write_ply`, `write_ply_labels`, `write_ply_obj` (:424-437, :492-514), `partition2ply`, `geof2ply`,
`prediction2ply`, `error2ply`, `spg2ply`, `scalar2ply` and `get_color_from_label` (:28-182), and the label file of
partition/write_Semantic3d.py (`write_label_file`, and `write_semantic3d_labels`, which streams the raw cloud through the
1-NN and never holds the full cloud's labels): the numbers become text on the device (csrc/spg_format.hip through
ops.text.format_table), a block of rows at a time.  Status: UNPINNED against plyfile, which is not installed where this was
built; pinned are the arrays the reference's own functions hand to plyfile (tests/golden/result_text.npz) and the text
numpy.savetxt gives for them with '%.18g' per record, which is what plyfile's text writer calls, and with '%d' (DESIGN.md 4.11k).
Not built: read_semantic3d_format2, the ply / las / pcd readers, read_vkitti_format, exponent notation, embedding2ply (sklearn's
PCA), edge_class2ply2, the HDF5 readers and writers and the two command-line scripts on top of them (h5py)."""
from __future__ import annotations

import glob
import os
import random

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


# --------------------------------------------------------------------------------------------------
# writers: ASCII PLY and label files, the text formatted on the device (ops.text.format_table)
# --------------------------------------------------------------------------------------------------
_WRITE_BLOCK = 1 << 20       # rows formatted, copied to the host and written at a time
# numpy dtype code of a PLY property -> (its name in the header, the dtype the column has on the device; uint32 travels as int64)
_PLY_TYPES = {'f4': ('float', np.float32, torch.float32), 'u1': ('uchar', np.uint8, torch.uint8), 'u4': ('uint', np.uint32, torch.int64),
              'i4': ('int', np.int32, torch.int32)}
_VERTEX_COLOUR = [('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]

# the class colours of get_color_from_label (partition/provider.py:124-182), label 0 (unlabelled, black) first
_CLASS_COLOURS = {
    's3dis': [[0, 0, 0], [233, 229, 107], [95, 156, 196], [179, 116, 81], [81, 163, 148], [241, 149, 131], [77, 174, 84], [108, 135, 75],
              [79, 79, 76], [41, 49, 101], [223, 52, 52], [89, 47, 95], [81, 109, 114], [233, 233, 229]],
    'sema3d': [[0, 0, 0], [200, 200, 200], [0, 70, 0], [0, 255, 0], [255, 255, 0], [255, 0, 0], [148, 0, 211], [0, 255, 255], [255, 8, 127]],
    'vkitti': [[0, 0, 0], [200, 90, 0], [0, 128, 50], [0, 220, 0], [255, 0, 0], [100, 100, 100], [200, 200, 200], [255, 0, 255],
               [255, 255, 0], [128, 0, 255], [255, 200, 150], [0, 128, 255], [0, 200, 255], [255, 128, 0]],
    'custom_dataset': [[0, 0, 0], [255, 0, 0], [0, 255, 0]]}


def get_color_from_label(object_label, dataset):
    """associate the color corresponding to the class"""
    if dataset not in _CLASS_COLOURS:
        raise ValueError('Unknown dataset: %s' % (dataset))
    table = _CLASS_COLOURS[dataset]
    if not (isinstance(object_label, (int, float, np.number)) and int(object_label) == object_label and 0 <= object_label < len(table)):
        raise ValueError('Type not recognized: %s' % (-1))
    return list(table[int(object_label)])


def _column(a, code, dev, n=None):
    """A numpy array or tensor as the device column of a PLY property of this dtype code, converted as the reference's
    assignment into the structured array converts it."""
    _, np_dtype, dtype = _PLY_TYPES[code]
    if torch.is_tensor(a):
        t = a.to(dev)
        t = (t.to(torch.int64) & 0xffffffff) if code == 'u4' else t.to(dtype)
    else:
        a = np.asarray(a).astype(np_dtype)
        if a.size == 0:
            return torch.empty(a.shape, dtype=dtype, device=dev)
        t = ops.upload(torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) if code == 'u4' else a)), dev)
    if n is not None and tuple(t.shape) != (n,):
        raise ValueError(f'a column of {n} values expected, got {tuple(t.shape)}')
    return t


def _xyz_columns(xyz, dev):
    xyz = _column(xyz, 'f4', dev)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f'xyz [n, 3] expected, got {tuple(xyz.shape)}')
    return [xyz[:, 0], xyz[:, 1], xyz[:, 2]]


def _colour_columns(rgb, dev, n):
    rgb = _column(rgb, 'u1', dev)
    if tuple(rgb.shape) != (n, 3):
        raise ValueError(f'colours [{n}, 3] expected, got {tuple(rgb.shape)}')
    return [rgb[:, 0], rgb[:, 1], rgb[:, 2]]


def _ply_header(elements):
    """elements: [(name, count, [(property, dtype code), ...]), ...] -> the header plyfile writes for text=True"""
    lines = ['ply', 'format ascii 1.0']
    for name, count, props in elements:
        lines.append(f'element {name} {count}')
        lines += [f'property {_PLY_TYPES[code][0]} {prop}' for prop, code in props]
    return '\n'.join(lines + ['end_header']) + '\n'


class _RowWriter:
    """Appends tables to an open binary file: at most block_rows rows are formatted on the device, copied into one page-locked
    buffer and written at a time, so device and host memory are bounded by the block."""

    def __init__(self, f, block_rows=_WRITE_BLOCK):
        if int(block_rows) < 1:
            raise ValueError('block_rows >= 1 expected')
        self.f, self.block_rows, self.device_buffer, self.pinned = f, int(block_rows), None, None

    def write(self, columns):
        n = int(columns[0].shape[0])
        for a in range(0, n, self.block_rows):
            part = [c[a:a + self.block_rows] for c in columns]
            need = ops.text.format_table_capacity(part)
            if self.device_buffer is None or self.device_buffer.numel() < need:
                self.device_buffer = torch.empty(need, dtype=torch.uint8, device=part[0].device)
                self.pinned = torch.empty(need, dtype=torch.uint8).pin_memory()
            text, _ = ops.text.format_table(part, out=self.device_buffer)
            total = int(text.numel())
            self.pinned[:total].copy_(text)                                  # (synchronous: the bytes are on the host when it returns)
            self.f.write(memoryview(self.pinned.numpy())[:total])


def _write_ply(filename, elements, block_rows=_WRITE_BLOCK):
    """The one writer behind every *ply function.  elements: [(name, [(property, dtype code, device column [n]), ...]), ...]"""
    with open(filename, 'wb') as f:
        f.write(_ply_header([(name, int(props[0][2].shape[0]), [(p, code) for p, code, _ in props]) for name, props in elements])
                .encode('ascii'))
        rows = _RowWriter(f, block_rows)
        for _, props in elements:
            rows.write([c for _, _, c in props])


def _vertex(props, columns):
    return [('vertex', [(p, code, c) for (p, code), c in zip(props, columns)])]


def _class_vector(values):
    """labels [n] or histograms / scores [n, c] (c > 1: arg-max first), as the reference's writers take them -> [n]"""
    if torch.is_tensor(values):
        return values.argmax(1) if values.dim() > 1 and values.shape[1] > 1 else values.reshape(-1)
    values = np.asarray(values)
    return np.argmax(values, axis=1) if len(values.shape) > 1 and values.shape[1] > 1 else values.reshape(-1)


def write_ply(filename, xyz, rgb):
    """write into a ply file"""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    _write_ply(filename, _vertex(_VERTEX_COLOUR, cols + _colour_columns(rgb, dev, len(cols[0]))))


def write_ply_labels(filename, xyz, rgb, labels):
    """write into a ply file. include the label"""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    n = len(cols[0])
    _write_ply(filename, _vertex(_VERTEX_COLOUR + [('label', 'u1')], cols + _colour_columns(rgb, dev, n) + [_column(labels, 'u1', dev, n)]))


def write_ply_obj(filename, xyz, rgb, labels, object_indices):
    """write into a ply file. include the label and the object number"""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    n = len(cols[0])
    _write_ply(filename, _vertex(_VERTEX_COLOUR + [('label', 'u1'), ('object_index', 'u4')],
                                 cols + _colour_columns(rgb, dev, n) + [_column(labels, 'u1', dev, n), _column(object_indices, 'u4', dev, n)]))


def scalar2ply(filename, xyz, scalar):
    """write a ply with a float scalar field"""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    _write_ply(filename, _vertex(_VERTEX_COLOUR[:3] + [('scalar', 'f4')], cols + [_column(scalar, 'f4', dev).reshape(-1)]))


def spg2ply(filename, spg_graph):
    """write a ply displaying the SPG by adding edges between its centroid: the elements vertex (sp_centroids) and edge (source, target)"""
    dev = _dev()
    cols = _xyz_columns(spg_graph['sp_centroids'], dev)
    source, target = (_column(spg_graph[k], 'i4', dev).reshape(-1) for k in ('source', 'target'))
    _write_ply(filename, _vertex(_VERTEX_COLOUR[:3], cols) + [('edge', [('vertex1', 'i4', source), ('vertex2', 'i4', target)])])


def prediction2ply(filename, xyz, prediction, n_label, dataset):
    """write a ply with colors for each class: prediction [n] or scores [n, c] (arg-max first).  A label outside 0 ... n_label keeps
    the black the reference's zero-initialised colours have; a dataset or a label <= n_label without a colour raises ValueError."""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    n_label = int(n_label)
    table = [get_color_from_label(i, dataset) for i in range(n_label + 1)] + [[0, 0, 0]]
    pred = _class_vector(prediction)
    pred = (pred.to(dev) if torch.is_tensor(pred) else ops.upload(torch.from_numpy(np.ascontiguousarray(pred).astype(np.int64)), dev)).long()
    table = ops.upload(torch.tensor(table, dtype=torch.uint8), dev)
    colour = table[torch.where((pred >= 0) & (pred <= n_label), pred, torch.full_like(pred, n_label + 1))]
    _write_ply(filename, _vertex(_VERTEX_COLOUR, cols + _colour_columns(colour, dev, len(cols[0]))))


def error2ply(filename, xyz, rgb, labels, prediction):
    """write a ply with green hue for correct classifcation and red for error (ops.text.error_colours: colorsys in float64 on
    the device, equal to the reference's loop)"""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    n = len(cols[0])
    labels, prediction = (v.to(dev).long() if torch.is_tensor(v) else ops.upload(torch.from_numpy(np.ascontiguousarray(v).astype(np.int64)), dev)
                          for v in (_class_vector(labels), _class_vector(prediction)))
    colour = ops.text.error_colours(_column(rgb, 'u1', dev).contiguous(), labels, prediction)
    _write_ply(filename, _vertex(_VERTEX_COLOUR, cols + _colour_columns(colour, dev, n)))


def geof2ply(filename, xyz, geof):
    """write a ply with colors corresponding to geometric features: 255 * geof[:, [0, 1, 3]] truncated to uint8, in geof's own
    precision.  Bit-equal to the reference's numpy expression wherever 255 * v lies in [0, 256); outside it the colour is the low
    byte of the value truncated to int32, which is what numpy's conversion gives on x86-64.  NaN, or a magnitude of 2^31 or more,
    raises ValueError (numpy's result there is the platform's)."""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    geof = geof.to(dev) if torch.is_tensor(geof) else ops.upload(torch.from_numpy(np.ascontiguousarray(geof)), dev)
    if geof.dim() != 2 or geof.shape[1] < 4 or not geof.dtype.is_floating_point:
        raise ValueError('geof2ply: geof [n, >= 4] of floats expected')
    scaled = 255 * geof[:, [0, 1, 3]]
    if bool(((scaled != scaled) | (scaled.abs() >= 2.0 ** 31)).any()):
        raise ValueError('geof2ply: 255 * geof is NaN or at least 2^31 in magnitude: no uint8 colour is defined for it')
    colour = (scaled.to(torch.int32) & 255).to(torch.uint8)
    _write_ply(filename, _vertex(_VERTEX_COLOUR, cols + _colour_columns(colour, dev, len(cols[0]))))


def partition2ply(filename, xyz, components, colors=None, in_component=None):
    """write a ply with random colors for each components.  colors: uint8 [n_com, 3]; without it three random.randint(0, 255) per
    component in component order, as in the reference (reproducible under random.seed).  Where components overlap the later
    one wins; a vertex in no component stays black.  in_component: the membership vector, as in perfect_prediction."""
    dev = _dev()
    cols = _xyz_columns(xyz, dev)
    n = len(cols[0])
    comp, n_com = _membership(components, n, in_component)
    if colors is None:
        colors = np.array([[random.randint(0, 255) for _ in range(3)] for _ in range(n_com - 1)], dtype=np.uint8).reshape(-1, 3)
    colors = colors.cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
    if colors.shape != (n_com - 1, 3):
        raise ValueError(f'partition2ply: colors [{n_com - 1}, 3] expected, got {colors.shape}')
    table = ops.upload(torch.from_numpy(np.vstack((colors.astype(np.uint8), np.zeros((1, 3), np.uint8)))), dev)
    comp = ops.upload(torch.from_numpy(comp), dev).long()
    if n and (int(comp.min()) < 0 or int(comp.max()) >= n_com):
        raise ValueError(f'partition2ply: in_component outside 0 ... {n_com - 1}')
    _write_ply(filename, _vertex(_VERTEX_COLOUR, cols + _colour_columns(table[comp], dev, n)))


def _label_values(values, offset):
    """values + offset as numpy computes it (a uint8 vector wraps), in a dtype the formatter takes"""
    values = np.asarray(values)
    if values.ndim != 1 or values.dtype.kind not in 'iu':
        raise ValueError('a one-dimensional integer label vector expected')
    values = values + offset
    if values.dtype.kind not in 'iu':
        raise ValueError('an integer offset expected')
    if values.dtype not in (np.uint8, np.int32, np.uint32, np.int64):
        if values.dtype == np.uint64 and values.size and int(values.max()) >= 1 << 63:
            raise ValueError('a label of 2^63 or more')
        values = values.astype(np.int64)
    return np.ascontiguousarray(values)


def write_label_file(label_file, labels, offset=1, block_rows=_WRITE_BLOCK):
    """The label file of the reference's partition/write_Semantic3d.py: the bytes of
    np.savetxt(label_file, labels + offset, delimiter=' ', fmt='%d'), one label per line, formatted on the device.
    labels: an integer numpy vector or device tensor."""
    dev = _dev()
    with open(label_file, 'wb') as f:
        rows = _RowWriter(f, block_rows)
        if torch.is_tensor(labels):
            if labels.dim() != 1 or labels.dtype.is_floating_point:
                raise ValueError('a one-dimensional integer label vector expected')
            labels = labels.to(dev)
            for a in range(0, int(labels.shape[0]), rows.block_rows):
                part = labels[a:a + rows.block_rows] + offset
                rows.write([part if part.dtype in ops.text.FORMAT_KINDS else part.long()])
        else:
            values = _label_values(labels, offset)
            for a in range(0, len(values), rows.block_rows):
                rows.write([ops.upload(torch.from_numpy(values[a:a + rows.block_rows]), dev)])


def write_semantic3d_labels(data_file, xyz, labels, label_file, ver_batch, n_cols=7, offset=1):
    """partition/write_Semantic3d.py's last two steps in one pass: every line of data_file (n_cols fields, x y z first), ver_batch
    lines at a time, is parsed on the device, takes the label of its nearest point of xyz [n, 3] (one ops.KnnIndex), and its
    label + offset is formatted and appended to label_file.  Neither the lines nor the labels of more than one batch are held.
    The file is byte for byte write_label_file(label_file, interpolate_labels_batch(data_file, xyz, labels, ver_batch), offset).
    labels [n] or label histograms [n, c] (arg-max first); ver_batch < 1 is refused as in interpolate_labels_batch.
    -> the number of lines written."""
    labels = _class_vector(labels.cpu().numpy() if torch.is_tensor(labels) else labels)
    if int(ver_batch) < 1:
        raise NotImplementedError('write_semantic3d_labels: with ver_batch <= 0 the reference returns an empty array; pass the '
                                  'chunk size (the result does not depend on it)')
    xyz = np.ascontiguousarray(xyz.cpu().numpy() if torch.is_tensor(xyz) else xyz, dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError('write_semantic3d_labels: xyz [n, 3] expected')
    if len(labels) != len(xyz):
        raise ValueError(f'write_semantic3d_labels: {len(labels)} labels for {len(xyz)} points')
    if not np.all(np.isfinite(xyz)):
        raise ValueError('Input contains NaN or infinity.')
    dev = _dev()
    # (what interpolate_labels_batch returns is labels[neighbour] in this dtype; adding the offset first is the same value)
    values = ops.upload(torch.from_numpy(_label_values(labels.astype(np.result_type(np.uint8, labels.dtype)), offset)), dev)
    index = ops.KnnIndex(ops.upload(torch.from_numpy(xyz), dev), query_capacity=min(int(ver_batch), _HOST_CHUNK))
    lines = 0
    with open(label_file, 'wb') as f:
        rows = _RowWriter(f)
        for xyz_full, _, _ in ops.CloudTextReader(data_file, int(n_cols), (0, 1, 2), rows=int(ver_batch), device=dev):
            neighbor = index.query(xyz_full, 1, distances=False)[0].reshape(-1).long()
            rows.write([values[neighbor]])
            lines += int(neighbor.shape[0])
    return lines
