"""'Reorganize point clouds into superpoints' on the device: the per-scene body of the reference's preprocess_pointclouds
(learning/s3dis_dataset.py:93-162, sema3d_dataset.py:85-135, vkitti_dataset.py:83-130, custom_dataset.py:67-107).  A scene goes
from device tensors (the outputs of ops.scene_structure / ops.compute_geof / ops.plane_elevation and a partition) to the
resident rows that spg.loader(..., device_cache=) reads, without leaving HBM; the kernels are csrc/spg_parsed.hip (DESIGN.md
section 4.11h).  Writing parsed/*.h5 is not done here."""
import random
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import ops

DATASETS = ('s3dis', 'sema3d', 'vkitti', 'custom')


@dataclass
class ParsedScene:
    """points f32 [Ntot, ncols] (device): the rows of superpoint ids[0], ids[1], ... back to back; offsets i64 [C + 1] (host);
    ids: the dataset names of the file (0 ... C - 1: the reference writes every component, the empty ones too); centroid f32 [3]
    (device; None for 'custom', whose files have none); class_count i64 [n_classes] (host) or None without labels; trimmed:
    {component: the positions random.sample chose}."""
    points: torch.Tensor
    offsets: np.ndarray
    ids: list
    centroid: Optional[torch.Tensor]
    class_count: Optional[np.ndarray]
    trimmed: dict

    def to_store(self):
        """{superpoint id: float32 array [n, ncols]}: a scene of MemoryPointStore."""
        host = self.points.cpu().numpy()
        return {i: host[self.offsets[k]:self.offsets[k + 1]] for k, i in enumerate(self.ids)}


def _component_csr(components, n, device):
    """-> (comp_off host int64 [C + 1], comp_idx device int32 | int64 [M])"""
    if isinstance(components, tuple) and len(components) == 2 and torch.is_tensor(components[1]) and components[1].is_cuda:
        off, idx = components                                    # a CSR pair (a tuple; a list is the reference's form)
        off = off.cpu().numpy() if torch.is_tensor(off) else np.asarray(off)
        return off.astype(np.int64).reshape(-1), idx.contiguous()
    if torch.is_tensor(components):                              # in_component [n]: ascending members per component
        if components.dim() != 1 or components.dtype.is_floating_point or components.shape[0] != n:
            raise ValueError(f'preprocess_scene: in_component must be an integer tensor [{n}]')
        comp = components.to(device=device, dtype=torch.int64)
        if comp.numel() and int(comp.min()) < 0:
            raise ValueError('preprocess_scene: in_component must not be negative')
        order = torch.sort(comp, stable=True)[1]
        counts = torch.bincount(comp).cpu().numpy()
        off = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        return off, order.to(torch.int32 if n < 2 ** 31 else torch.int64).contiguous()
    arrs = [np.asarray(c).reshape(-1) for c in components]       # the reference's form: one index array per component
    for a in arrs:
        if a.size and a.dtype.kind not in 'iu':
            raise ValueError('preprocess_scene: a component must be an integer array')
    off = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=off[1:])
    flat = np.concatenate([a.astype(np.int64) for a in arrs]) if arrs else np.zeros(0, np.int64)
    return off, torch.from_numpy(flat).to(device)


def preprocess_scene(dataset, xyz, rgb, components, *, geof=None, elevation=None, labels=None, supervized_partition=False,
                     plane_model_elevation=False, max_points=10000, rng=random):
    """One scene of preprocess_pointclouds.  dataset: 's3dis' | 'sema3d' | 'vkitti' | 'custom'; xyz f32 [n, 3], rgb u8 | f32 [n, 3],
    geof f32 [n, 4] (not for vkitti), labels u32 | i32 [n, n_classes + 1] or None, all on the device.  components: a list of index
    arrays (the reference's form), a pair (comp_off [C + 1], comp_idx [M] on the device), or in_component [n] (device).
    s3dis: with plane_model_elevation the elevation is the given tensor when supervized_partition, else ops.plane_elevation(xyz);
    without it z / 4 - 0.5.  supervized_partition also leaves geof as it is (no - 0.5).
    Components above max_points rows are trimmed with rng.sample(range(size), k=max_points), drawn on the host per oversized
    component in component order -- the reference's consumption of Python's stream: random.seed(area) before the call reproduces
    its selection.  Only the component sizes come down for this; only the trim tables go up."""
    if dataset not in DATASETS:
        raise ValueError(f'preprocess_scene: dataset must be one of {DATASETS}, got {dataset!r}')
    n, dev = int(xyz.shape[0]), xyz.device
    comp_off, comp_idx = _component_csr(components, n, dev)
    e, lpsv_raw = None, False
    if dataset == 's3dis':
        lpsv_raw = bool(supervized_partition)
        if plane_model_elevation:
            if supervized_partition:
                if elevation is None:
                    raise ValueError('preprocess_scene: supervized_partition with plane_model_elevation reads the stored elevation; pass it')
                e = elevation
            else:
                e = ops.plane_elevation(xyz)['elevation']
    sizes = np.diff(comp_off)
    trimmed = {}
    for c in np.flatnonzero(sizes > max_points):
        trimmed[int(c)] = np.asarray(rng.sample(range(int(sizes[c])), k=int(max_points)), dtype=np.int64)
    points, centroid, offsets = ops.parsed_points(dataset, xyz, rgb, comp_off, comp_idx, geof=geof, elevation=e, trim=trimmed,
                                                  lpsv_raw=lpsv_raw)
    count = None
    if labels is not None and dataset != 'custom':
        count = ops.class_count(labels, int(labels.shape[1]) - 1).cpu().numpy()
    return ParsedScene(points, offsets, list(range(len(sizes))), None if dataset == 'custom' else centroid, count, trimmed)
