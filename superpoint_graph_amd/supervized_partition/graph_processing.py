"""`graph_loader` / `graph_collate` / `augment_cloud_whole` with the reference's signatures (supervized_partition/
graph_processing.py:347-472, :534-546), made on the device (csrc/spg_tiles.hip through ops.neighbourhood_tiles, ops.augment_whole,
ops.random_subgraph, ops.induced_subgraph): a scene (xyz, rgb, the neighbour table, the edges, the per-vertex attributes) is
uploaded once as a `DeviceScene` and every batch is built from it there -- no host gather `xyz[nei]`, no copy of the tiles, no
adjacency list rebuilt per sample.  The output of `graph_collate` feeds `LocalCloudEmbedder.run_batch` and
`losses.compute_dist` / `compute_loss` as it is: a training step of the learned partition stays on the device.

The scene itself is made here too: `build_structure` restates the per-file body of the reference's main() (:120-190) on the
device (ops.prune, ops.knn, ops.compute_geof, ops.scene_structure: csrc/spg_structure.hip) and returns a `DeviceScene` without a
host copy; `structure_arrays` brings it to the host in write_structure's order and dtypes (:198-221).

Vertex values: the learned embeddings (`args.learned_embeddings` with ver_value 'ptn') and the hand-crafted ones ('geof' /
'geofrgb' with learned_embeddings 0: `clouds` is the geof array, with the colours appended for 'geofrgb'; `spatialEmbedder`
returns it).  What the reference draws at random stays on the host and in the reference's order (numpy's global stream, or
`rng`); only the seed vertices of the subgraph differ: the reference takes them from an unseeded C rand(), here they come from
`seeds` or from the same numpy stream.  No CPU path."""
from __future__ import annotations

import math
import os
import types

import numpy as np
import torch

from .. import ops
from ..ops import EdgeGraph

STRUCTURE_KEYS = ('xyz', 'rgb', 'edg_source', 'edg_target', 'is_transition', 'local_geometry', 'labels', 'objects', 'elevation', 'xyn')
SEED_BATCH = 64          # seed vertices drawn per call of ops.random_subgraph when the caller gives none


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError('superpoint_graph_amd.supervized_partition has no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


def _up(a, dtype, dev):
    # (a plain copy: scenes are uploaded once and are far larger than the staging ring of ops.upload)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False))).to(dev)


class DeviceScene:
    """One scene of features_supervision/ on the device: xyz f32 [n, 3], rgb f32 [n, 3] (divided by 255 on the host, in float32, as
    graph_loader does), nei i32 [n, K] (target_local_geometry), edg_source / edg_target i64 [E] and their EdgeGraph, is_transition
    u8 [E], labels, objects i64 [n], elevation f32 [n], xyn f32 [n, 2], geof f32 [n, 4] or None (the hand-crafted vertex values,
    column 3 already doubled as write_structure stores it)."""

    def __init__(self, xyz, rgb, edg_source, edg_target, is_transition, local_geometry, labels, objects, elevation, xyn, device=None,
                 geof=None):
        dev = _dev() if device is None else device
        xyz = np.asarray(xyz, np.float32)
        self.n = int(xyz.shape[0])
        self.device = dev
        self.xyz = _up(xyz, np.float32, dev)
        self.rgb = _up(np.asarray(rgb, np.float32) / 255, np.float32, dev)                 # graph_processing.py:353
        nei = np.asarray(local_geometry)
        if nei.ndim != 2 or nei.shape[0] != self.n:
            raise ValueError(f'local_geometry must be [{self.n}, K] (the neighbour table), got {list(nei.shape)}')
        self.nei = _up(nei, np.int32, dev)
        self.edg_source = _up(np.asarray(edg_source).reshape(-1), np.int64, dev)
        self.edg_target = _up(np.asarray(edg_target).reshape(-1), np.int64, dev)
        self.graph = EdgeGraph(self.edg_source, self.edg_target, self.n)
        self.is_transition = _up(np.asarray(is_transition).reshape(-1), np.uint8, dev)
        labels = np.asarray(labels)
        self.labels = _up(labels, labels.dtype if labels.dtype != np.uint32 else np.int64, dev)
        self.objects = _up(np.asarray(objects).reshape(-1), np.int64, dev)
        self.elevation = _up(np.asarray(elevation).reshape(-1), np.float32, dev)
        self.xyn = _up(xyn, np.float32, dev)
        self.geof = None if geof is None else _up(np.asarray(geof, np.float32).reshape(self.n, 4), np.float32, dev)

    @classmethod
    def from_device(cls, xyz, rgb, edg_source, edg_target, is_transition, nei, labels, objects, elevation, xyn, geof=None, graph=None):
        """Adopts device tensors as they are (no host copy, no conversion): xyz f32 [n, 3], rgb f32 [n, 3] ALREADY divided by 255,
        edg_source / edg_target i64 [E], is_transition u8 [E], nei i32 [n, K], labels (any integer dtype, [n] or [n, C]), objects
        i64 [n], elevation f32 [n], xyn f32 [n, 2], geof f32 [n, 4] or None; graph: the EdgeGraph of the edges if the caller has
        it already (ops.scene_structure returns one)."""
        n = int(xyz.shape[0])
        for t, dtype, shape, name in ((xyz, torch.float32, (n, 3), 'xyz'), (rgb, torch.float32, (n, 3), 'rgb'),
                                      (edg_source, torch.int64, tuple(edg_target.shape), 'edg_source'),
                                      (edg_target, torch.int64, (int(edg_target.numel()),), 'edg_target'),
                                      (is_transition, torch.uint8, tuple(edg_target.shape), 'is_transition'),
                                      (nei, torch.int32, (n, int(nei.shape[-1])), 'nei'), (objects, torch.int64, (n,), 'objects'),
                                      (elevation, torch.float32, (n,), 'elevation'), (xyn, torch.float32, (n, 2), 'xyn'),
                                      (geof, torch.float32, (n, 4), 'geof')):
            if t is None and name == 'geof':
                continue
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f'DeviceScene.from_device: {name} must be a contiguous {dtype} device tensor of shape {list(shape)}')
        if not torch.is_tensor(labels) or labels.device != xyz.device:
            raise ValueError('DeviceScene.from_device: labels must be a device tensor')
        self = cls.__new__(cls)
        self.n, self.device = n, xyz.device
        self.xyz, self.rgb, self.nei = xyz, rgb, nei
        self.edg_source, self.edg_target, self.is_transition = edg_source, edg_target, is_transition
        self.graph = graph if graph is not None else EdgeGraph(edg_source, edg_target, n)
        self.labels, self.objects, self.elevation, self.xyn, self.geof = labels, objects, elevation, xyn, geof
        return self


class _SceneStore:
    """entry -> read_structure's ten values (host arrays) and the DeviceScene made of them, uploaded once.  With read_geof the
    scene also holds the geof array (read_structure returns it in the place of the neighbour table)."""

    def __init__(self):
        self._device = {}

    def scene(self, entry, read_geof=False):
        have = self._device.get(entry)
        if have is None or (read_geof and have.geof is None):
            geof = self.read_structure(entry, True)[5] if read_geof else None
            self._device[entry] = DeviceScene(*self.read_structure(entry, False), geof=geof)
        return self._device[entry]

    def drop(self, entry=None):
        if entry is None:
            self._device.clear()
        else:
            self._device.pop(entry, None)


class MemorySceneStore(_SceneStore):
    """features_supervision/ in memory: {entry: dict with the STRUCTURE_KEYS (and 'geof' for the hand-crafted vertex values), the
    ten arrays in read_structure's order, or a DeviceScene (of build_structure), which is used as it is}."""

    def __init__(self, scenes):
        super().__init__()
        self._scenes = scenes

    def scene(self, entry, read_geof=False):
        s = self._scenes[entry]
        if isinstance(s, DeviceScene):
            if read_geof and s.geof is None:
                raise KeyError(f"MemorySceneStore: the DeviceScene of {entry!r} holds no geof")
            return s
        return super().scene(entry, read_geof)

    def read_structure(self, entry, read_geof):
        s = self._scenes[entry]
        if isinstance(s, DeviceScene):
            s = structure_arrays(s)
        if not isinstance(s, dict):
            if read_geof:
                raise KeyError(f"MemorySceneStore: {entry!r} is a tuple of read_structure's ten values and holds no geof; use a dict")
            return tuple(s)
        if read_geof and s.get('geof') is None:
            raise KeyError(f"MemorySceneStore: {entry!r} has no 'geof'")
        return tuple(s['geof' if (read_geof and k == 'local_geometry') else k] for k in STRUCTURE_KEYS)


class H5SceneStore(_SceneStore):
    """<ROOT_PATH>/features_supervision/<folder>/<scene>.h5 as write_structure stores it (graph_processing.py:198-247; needs h5py)."""

    def read_structure(self, entry, read_geof):
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError('H5SceneStore needs h5py; use MemorySceneStore with arrays of your own') from e
        f = h5py.File(entry, 'r')
        labels = np.array(f['labels']).squeeze()
        is_transition = np.array(f['is_transition'])
        if len(labels.shape) == 0:
            labels = np.array([0])
        if len(is_transition.shape) == 0:
            is_transition = np.array([0])
        local_geometry = np.array(f['geof'], dtype='float32') if read_geof else np.array(f['target_local_geometry'], dtype='uint32')
        return (np.array(f['xyz'], dtype='float32'), np.array(f['rgb'], dtype='float32'), np.array(f['source'], dtype='int').squeeze(),
                np.array(f['target'], dtype='int').squeeze(), is_transition, local_geometry, labels,
                np.array(f['objects'][()]), np.array(f['elevation'], dtype='float32'), np.array(f['xyn'], dtype='float32'))


_default_store = None


def _store(store):
    global _default_store
    if store is not None:
        return store
    if _default_store is None:
        _default_store = H5SceneStore()
    return _default_store


def axangle_z(theta):
    """transforms3d.axangles.axangle2mat([0, 0, 1], theta) (its expressions for the unit z axis), float64 [3, 3]."""
    c, s = math.cos(theta), math.sin(theta)
    C = 1 - c
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, C + c]])


def augment_cloud_whole(args, xyz, rgb, rng=None):
    """graph_processing.py:534-546 on device tensors -> (xyz, rgb).  The random quantities are drawn on the host in the reference's
    order (reference vertex, angle, xyz noise, rgb noise when args.use_rgb) from numpy's global stream or from `rng` (a
    np.random.RandomState), the arithmetic is ops.augment_whole.  As in the reference, the reference point is a VIEW of its vertex:
    setting its z to 0 also moves that vertex onto the plane z = 0 before the rotation."""
    rng = np.random if rng is None else rng
    n = int(xyz.shape[0])
    M = ref_point = noise_xyz = noise_rgb = None
    if args.pc_augm_rot:
        i = int(rng.randint(n))
        xyz = xyz.clone()
        xyz[i, 2] = 0
        ref_point = xyz[i].cpu().numpy()
        M = axangle_z(rng.uniform(0, 2 * math.pi)).astype('f4')
    if args.pc_augm_jitter:
        sigma, clip = 0.002, 0.005
        noise_xyz = _up(np.clip(sigma * rng.standard_normal((n, 3)), -1 * clip, clip), np.float32, xyz.device)
        if args.use_rgb:
            noise_rgb = _up(np.clip(sigma * rng.standard_normal((n, 3)), -1 * clip, clip), np.float32, xyz.device)
    return ops.augment_whole(xyz, rgb, ref_point, M, noise_xyz, noise_rgb)


def subgraph_sampling(scene: DeviceScene, max_ver: int, seeds=None, rng=None):
    """libply_c.random_subgraph on the scene's EdgeGraph -> (selected_edg u8 [E], selected_ver u8 [n]).  seeds: the seed vertices in
    order (ValueError when they run out); None draws them SEED_BATCH at a time from `rng` / numpy's global stream."""
    if seeds is not None:
        se, sv, seen, _, _ = ops.random_subgraph(scene.graph, max_ver, seeds)
        if seen < max_ver:
            raise ValueError(f'subgraph_sampling: the {len(seeds)} seeds reach {seen} of {max_ver} vertices')
        return se, sv
    rng = np.random if rng is None else rng
    state = None
    while True:
        se, sv, seen, _, state = ops.random_subgraph(scene.graph, max_ver, rng.randint(scene.n, size=SEED_BATCH), state)
        if seen >= max_ver:
            return se, sv


def graph_loader(entry, train, args, db_path, test_seed_offset=0, full_cpu=False, store=None, seeds=None, rng=None):
    """graph_processing.py:347-436 -> (short_name, edg_source, edg_target, is_transition, labels, objects, clouds, clouds_global, nei,
    xyz): device tensors (edg_* i64, is_transition u8, objects i64, clouds f32 [m, 3 or 6, k], clouds_global f32 [m, G], xyz f32
    [m, 3]), short_name a string, nei the host array [0] the reference returns.  store: a MemorySceneStore / H5SceneStore (default:
    one H5SceneStore for the process); seeds / rng: see subgraph_sampling and augment_cloud_whole.  full_cpu is accepted and
    ignored (the batch is made where the scene lives).
    ver_value 'geof' / 'geofrgb' (learned_embeddings 0, :415-424): clouds f32 [n, 4] = the scene's geof, or [n, 7] with rgb
    appended, and clouds_global the host tensor [0] of the reference."""
    hand_crafted = args.ver_value in ('geof', 'geofrgb')
    if hand_crafted == bool(args.learned_embeddings):
        raise NotImplementedError(f"graph_loader: ver_value 'ptn' with learned_embeddings 1, or 'geof' / 'geofrgb' with learned_embeddings 0 "
                                  f"(what the reference's parser derives), got {args.ver_value!r} with learned_embeddings {args.learned_embeddings!r}")
    scene = _store(store).scene(entry, hand_crafted)
    short_name = entry.split(os.sep)[-2] + '/' + entry.split(os.sep)[-1]
    xyz, rgb = scene.xyz, scene.rgb
    if hand_crafted and train and (0 < args.max_ver_train < scene.n):
        raise ValueError(f"graph_loader: ver_value {args.ver_value!r} with train and 0 < max_ver_train < n is inconsistent in the reference "
                         "(graph_processing.py:417-422 does not select the rows of local_geometry) and never runs there (the epoch loop "
                         "breaks at once when learned_embeddings is 0): pass max_ver_train = 0")
    if train:
        xyz, rgb = augment_cloud_whole(args, xyz, rgb, rng)
    if hand_crafted:
        clouds = scene.geof if args.ver_value == 'geof' else torch.cat([scene.geof, rgb], 1)
        return (short_name, scene.edg_source, scene.edg_target, scene.is_transition, scene.labels, scene.objects, clouds, torch.tensor([0]),
                np.array([0]), xyz)
    edg_source, edg_target, is_transition = scene.edg_source, scene.edg_target, scene.is_transition
    labels, objects, rows = scene.labels, scene.objects, None
    if train and (0 < args.max_ver_train < scene.n):
        selected_edg, selected_ver = subgraph_sampling(scene, int(args.max_ver_train), seeds, rng)
        rows, _, kept, edg_source, edg_target = ops.induced_subgraph(scene.graph, selected_ver, selected_edg)
        is_transition = is_transition[kept]
        labels, objects = labels[rows], objects[rows]
    clouds, clouds_global, _ = ops.neighbourhood_tiles(xyz, scene.nei, int(args.k_nn_local), rows=rows, rgb=rgb, global_feat=args.global_feat,
                                                       elevation=scene.elevation, xyn=scene.xyn, cloud_rgb=bool(args.use_rgb))
    nei = np.array([0])
    return short_name, edg_source, edg_target, is_transition, labels, objects, clouds, clouds_global, nei, (xyz if rows is None else xyz[rows])


def graph_collate(batch):
    """graph_processing.py:439-472 on the samples of graph_loader -> (short_name, edg_source, edg_target, is_transition, labels,
    objects, (clouds, clouds_global, nei), xyz).  Edge ends are offset by the cumulative vertex counts and objects by the cumulative
    max() of each sample (not max() + 1), as the reference does; nei gets the reference's arithmetic on its [0] rows.  No host
    synchronisation: the object offsets are computed on the device."""
    short_name, edg_source, edg_target, is_transition, labels, objects, clouds, clouds_global, nei, xyz = list(zip(*batch))
    n_batch = len(short_name)
    batch_ver_size_cumsum = np.array([c.shape[0] for c in labels]).cumsum()
    object_offsets = torch.stack([c.max() for c in objects]).cumsum(0)
    edg_source, edg_target, objects = list(edg_source), list(edg_target), list(objects)
    nei = np.vstack(nei)
    for i_batch in range(1, n_batch):
        lo, hi = int(batch_ver_size_cumsum[i_batch - 1]), int(batch_ver_size_cumsum[i_batch])
        edg_source[i_batch] = edg_source[i_batch] + lo
        edg_target[i_batch] = edg_target[i_batch] + lo
        objects[i_batch] = objects[i_batch] + object_offsets[i_batch - 1]
        non_valid = (nei[lo:hi, ] == -1).nonzero()
        nei[lo:hi, ] += lo
        nei[lo + non_valid[0], non_valid[1]] = -1
    return (short_name, torch.cat(edg_source, 0), torch.cat(edg_target, 0), torch.cat(is_transition, 0), torch.cat(labels, 0), torch.cat(objects, 0),
            (torch.cat(clouds, 0), torch.cat(clouds_global, 0), nei), torch.cat(xyz, 0))


class spatialEmbedder():
    """The hand-crafted embedding of the reference (graph_processing.py:548-560): the clouds of graph_loader with ver_value
    'geof' / 'geofrgb' ARE the embeddings."""

    def __init__(self, args):
        self.args = args

    def run_batch(self, model, clouds, *excess):
        return clouds.cuda() if self.args.cuda else clouds


# ---------------------------------------------------------------------------------------------------------------------
# the scene structure (graph_processing.py:120-221)
# ---------------------------------------------------------------------------------------------------------------------
STRUCTURE_DEFAULTS = dict(k_nn_local=20, k_nn_adj=5, voxel_width=0.03, compute_geof=1, plane_model=1, use_voronoi=0.0)   # :39-44


def _device_array(a, np_dtype, torch_dtype, dev, name):
    if a is None:
        raise ValueError(f'build_structure: {name} is needed')
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch_dtype).contiguous()
    return _up(a, np_dtype, dev)


def build_structure(xyz, rgb, labels, objects, args, dataset, n_labels, n_objects=None, elevation=None) -> DeviceScene:
    """The per-file body of the reference's main() (graph_processing.py:120-190) on the device -> the DeviceScene that the file it
    writes would give.  xyz f32 [n, 3], rgb u8 [n, 3], labels u8 [n], objects integer [n] (or None): host arrays or device
    tensors.  args: k_nn_local, k_nn_adj, voxel_width, compute_geof, plane_model, use_voronoi (STRUCTURE_DEFAULTS where absent).
    dataset 's3dis' (and 'sema3d' with objects=): voxel_width > 0 prunes with labels and objects (n_objects: the largest id + 1;
    None reads objects.max() back as the reference does), the vertex's object is the arg-max of its histogram from column 1 on;
    without pruning the objects are taken as given.  dataset 'vkitti': prunes with labels only, hard label = arg-max of the label histogram, objects =
    the components of constant hard label (without pruning, labels must already be a histogram i32 [n, C]).  Then one kNN self
    query with k_nn_local, compute_geof on that table, ops.scene_structure.  elevation: with plane_model = 1 (the reference's default)
    either 'ransac' -- the height above the RANSAC ground plane of the (pruned) cloud, ops.plane_elevation (:181-186) -- or an array
    f32 [n of the pruned cloud], used as it is; None asks the caller to choose (NotImplementedError).  With plane_model = 0 'ransac'
    and None both give z - min z (:188).  Nothing is read back but the words the ops read (voxel count, low-point count, error words,
    trial counters, component count)."""
    a = types.SimpleNamespace(**{k: getattr(args, k, v) for k, v in STRUCTURE_DEFAULTS.items()})
    k_local, k_adj = int(a.k_nn_local), int(a.k_nn_adj)
    if dataset not in ('s3dis', 'vkitti', 'sema3d'):
        raise ValueError('%s is an unknown data set' % dataset)
    if dataset == 'sema3d' and objects is None:
        raise NotImplementedError("build_structure: dataset 'sema3d' makes its objects by label inpainting with libcp.cutpursuit2 (cut "
                                  "pursuit is not part of this package); pass objects= to use the s3dis rule")
    if a.use_voronoi > 0:
        raise NotImplementedError('build_structure: use_voronoi > 0 needs the Delaunay adjacency (qhull), which is not part of this package')
    if a.plane_model and elevation is None:
        raise NotImplementedError("build_structure: plane_model = 1 fits the ground plane with RANSAC; pass elevation='ransac' (the fit of "
                                  "ops.plane_elevation on the device), an elevation array (used as it is) or plane_model = 0")
    if k_local > ops.KNN_MAX_K:
        raise NotImplementedError(f'build_structure: k_nn_local = {k_local} exceeds the device kNN limit ops.KNN_MAX_K = {ops.KNN_MAX_K}')
    if not 1 <= k_adj <= k_local:
        raise ValueError('build_structure: knn1 must be smaller than knn2 (1 <= k_nn_adj <= k_nn_local)')
    dev = _dev()
    xyz = _device_array(xyz, np.float32, torch.float32, dev, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f'build_structure: xyz must be [n, 3], got {list(xyz.shape)}')
    rgb = _device_array(rgb, np.uint8, torch.uint8, dev, 'rgb')
    pruning = a.voxel_width > 0
    voxel = float(np.float32(a.voxel_width))
    ids = hist = None
    if dataset == 'vkitti':
        id_mode = 'labels'
        if pruning:
            labels = _device_array(labels, np.uint8, torch.uint8, dev, 'labels').reshape(-1)
            xyz, rgb, labels, _ = ops.prune(xyz, voxel, rgb, labels, None, int(n_labels), 0)                   # :142
        else:
            labels = _device_array(labels, np.int32, torch.int32, dev, 'labels')
            if labels.dim() != 2:
                raise ValueError("build_structure: dataset 'vkitti' without pruning takes its hard labels from a histogram [n, C] (:168)")
        hist = labels
    else:
        if pruning:
            labels = _device_array(labels, np.uint8, torch.uint8, dev, 'labels').reshape(-1)
            objects = _device_array(objects, np.int32, torch.int32, dev, 'objects').reshape(-1)
            if n_objects is None:
                n_objects = int(objects.max()) + 1                                                             # :123
            xyz, rgb, labels, hist = ops.prune(xyz, voxel, rgb, labels, objects, int(n_labels), int(n_objects))   # :124
            id_mode = 'objects'                                                                                # :126
        else:
            labels = _device_array(labels, np.uint8, torch.uint8, dev, 'labels')
            ids = _device_array(objects, np.int64, torch.int64, dev, 'objects').reshape(-1)
            id_mode = 'given'
    n = int(xyz.shape[0])
    if n <= k_local:
        raise ValueError(f'Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {k_local + 1}')
    if isinstance(elevation, str):
        if elevation != 'ransac':
            raise ValueError(f"build_structure: elevation must be 'ransac', an array or None, got {elevation!r}")
        elevation = ops.plane_elevation(xyz)['elevation'] if a.plane_model else None                            # :181-186
    if elevation is not None:
        elevation = _device_array(elevation, np.float32, torch.float32, dev, 'elevation').reshape(-1)
        if elevation.shape[0] != n:
            raise ValueError(f'build_structure: elevation must hold one value per vertex of the {"pruned " if pruning else ""}cloud ({n}), '
                             f'got {elevation.shape[0]}')
    nei, _ = ops.knn(xyz, k_local, distances=False)                                                            # :146
    geof = ops.compute_geof(xyz, nei.reshape(-1), k_local) if a.compute_geof else None                         # :176
    s = ops.scene_structure(xyz, nei, k_adj, ids=ids, hist=hist, id_mode=id_mode, geof=geof, rgb=rgb)          # :149-190
    return DeviceScene.from_device(xyz, s['rgb'], s['edg_source'], s['edg_target'], s['is_transition'], nei, labels, s['objects'],
                                   s['elevation'] if elevation is None else elevation, s['xyn'], geof=geof, graph=s['graph'])


def structure_arrays(scene: DeviceScene):
    """The scene on the host as write_structure stores it (graph_processing.py:198-221), in the order of its datasets and with their
    dtypes, under the names of STRUCTURE_KEYS (plus 'geof' when the scene has it): xyz f32, rgb f32 in 0 ... 255 (the scene keeps
    rgb / 255: the integers are restored by rounding), elevation f32, xyn f32, edg_source / edg_target int64, is_transition u8,
    local_geometry u32 [n, K], objects u32, geof f32, labels int32 (histograms) or u8.  A MemorySceneStore takes the dict as a scene."""
    def host(t):
        return t.cpu().numpy()
    out = {'xyz': host(scene.xyz), 'rgb': np.rint(host(scene.rgb) * np.float32(255)).astype(np.float32), 'elevation': host(scene.elevation),
           'xyn': host(scene.xyn), 'edg_source': host(scene.edg_source), 'edg_target': host(scene.edg_target),
           'is_transition': host(scene.is_transition), 'local_geometry': host(scene.nei).astype(np.uint32),
           'objects': host(scene.objects).astype(np.uint32)}
    if scene.geof is not None:
        out['geof'] = host(scene.geof)
    labels = host(scene.labels)
    out['labels'] = labels.astype(np.int32 if labels.ndim > 1 and labels.shape[1] > 1 else np.uint8)
    return out
