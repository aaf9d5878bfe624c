"""`graph_loader` / `graph_collate` / `augment_cloud_whole` with the reference's signatures (supervized_partition/
graph_processing.py:347-472, :534-546), made on the device (csrc/spg_tiles.hip through ops.neighbourhood_tiles, ops.augment_whole,
ops.random_subgraph, ops.induced_subgraph): a scene (xyz, rgb, the neighbour table, the edges, the per-vertex attributes) is
uploaded once as a `DeviceScene` and every batch is built from it there -- no host gather `xyz[nei]`, no copy of the tiles, no
adjacency list rebuilt per sample.  The output of `graph_collate` feeds `LocalCloudEmbedder.run_batch` and
`losses.compute_dist` / `compute_loss` as it is: a training step of the learned partition stays on the device.

Restricted to the learned embeddings (`args.learned_embeddings` with ver_value 'ptn'); the 'geof' / 'geofrgb' vertex values
raise NotImplementedError.  What the reference draws at random stays on the host and in the reference's order (numpy's global
stream, or `rng`); only the seed vertices of the subgraph differ: the reference takes them from an unseeded C rand(), here they
come from `seeds` or from the same numpy stream.  No CPU path."""
from __future__ import annotations

import math
import os

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
    u8 [E], labels, objects i64 [n], elevation f32 [n], xyn f32 [n, 2]."""

    def __init__(self, xyz, rgb, edg_source, edg_target, is_transition, local_geometry, labels, objects, elevation, xyn, device=None):
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


class _SceneStore:
    """entry -> read_structure's ten values (host arrays) and the DeviceScene made of them, uploaded once."""

    def __init__(self):
        self._device = {}

    def scene(self, entry):
        if entry not in self._device:
            self._device[entry] = DeviceScene(*self.read_structure(entry, False))
        return self._device[entry]

    def drop(self, entry=None):
        if entry is None:
            self._device.clear()
        else:
            self._device.pop(entry, None)


class MemorySceneStore(_SceneStore):
    """features_supervision/ in memory: {entry: dict with the STRUCTURE_KEYS, or the ten arrays in read_structure's order}."""

    def __init__(self, scenes):
        super().__init__()
        self._scenes = scenes

    def read_structure(self, entry, read_geof):
        if read_geof:
            raise NotImplementedError("the 'geof' / 'geofrgb' vertex values are not part of this package")
        s = self._scenes[entry]
        return tuple(s[k] for k in STRUCTURE_KEYS) if isinstance(s, dict) else tuple(s)


class H5SceneStore(_SceneStore):
    """<ROOT_PATH>/features_supervision/<folder>/<scene>.h5 as write_structure stores it (graph_processing.py:198-247; needs h5py)."""

    def read_structure(self, entry, read_geof):
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError('H5SceneStore needs h5py; use MemorySceneStore with arrays of your own') from e
        if read_geof:
            raise NotImplementedError("the 'geof' / 'geofrgb' vertex values are not part of this package")
        f = h5py.File(entry, 'r')
        labels = np.array(f['labels']).squeeze()
        is_transition = np.array(f['is_transition'])
        if len(labels.shape) == 0:
            labels = np.array([0])
        if len(is_transition.shape) == 0:
            is_transition = np.array([0])
        return (np.array(f['xyz'], dtype='float32'), np.array(f['rgb'], dtype='float32'), np.array(f['source'], dtype='int').squeeze(),
                np.array(f['target'], dtype='int').squeeze(), is_transition, np.array(f['target_local_geometry'], dtype='uint32'), labels,
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
    ignored (the batch is made where the scene lives)."""
    if not args.learned_embeddings or 'geof' in args.ver_value:
        raise NotImplementedError(f"graph_loader: only the learned embeddings (ver_value 'ptn') are built on the device, got {args.ver_value!r}")
    scene = _store(store).scene(entry)
    short_name = entry.split(os.sep)[-2] + '/' + entry.split(os.sep)[-1]
    xyz, rgb = scene.xyz, scene.rgb
    if train:
        xyz, rgb = augment_cloud_whole(args, xyz, rgb, rng)
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
