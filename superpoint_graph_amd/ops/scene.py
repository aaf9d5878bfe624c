"""Per-scene preparation of the learned partition: scene structure, RANSAC ground plane, scene statistics, parsed superpoint clouds
and class counts (csrc/spg_structure.hip, spg_plane.hip, spg_parsed.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib
from ._core import _ptr, _raise_flagged, _raise_nonfinite, _req, _scene_xyz, _stream, _workspace
from .edges import EdgeGraph, connected_components


# --------------------------------------------------------------------------------------------------
# the scene structure of the learned partition (csrc/spg_structure.hip; reference supervized_partition/graph_processing.py:120-190)
# --------------------------------------------------------------------------------------------------
_ID_MODES = {'objects': 1, 'labels': 2, 'given': 3}
_NEIGHBOUR_RANGE = 2      # bit of spg_structure_edges' error word (bit 0, read after spg_structure_frame, is _core._NONFINITE)


def scene_structure(xyz, knn_idx, k_adj: int, ids=None, hist=None, id_mode='objects', geof=None, rgb=None):
    """What graph_processing.py:main() computes per file between prune, the kNN search and compute_geof (:126, :144-190), on
    device tensors: xyz f32 [n, 3]; knn_idx i32 [n, k_local] as ops.knn returns it (the point itself dropped); the first k_adj
    columns are the adjacency.  The vertex ids that decide is_transition come from
      id_mode 'objects': hist i32 [n, C] (pruned s3dis objects)  -> hist[:, 1:].argmax(1) + 1,
      id_mode 'labels':  hist i32 [n, C] (pruned vkitti labels)   -> hist.argmax(1); the objects are then the components over
                         the edges that are no transition (ops.connected_components: numbered by smallest member),
      id_mode 'given':   ids integer [n].
    geof f32 [n, 4] (ops.compute_geof) gets its column 3 doubled IN PLACE (:177); rgb u8 [n, 3] is returned as f32 / 255 (:353).
    -> dict of device tensors: edg_source, edg_target i64 [n * k_adj], nei (knn_idx itself: adopted, not copied), is_transition
    u8, hard_ids i64 [n], objects i64 [n], elevation f32 [n] (z - min z), xyn f32 [n, 2], geof, rgb (None when not given), and
    graph, the EdgeGraph of the adjacency.  Host reads: the error word after the frame pass (ValueError on NaN / infinity before
    anything else is launched) and after the edges, the EdgeGraph's, and the component count with id_mode 'labels'."""
    n, k_adj = _scene_xyz(xyz, 'scene_structure'), int(k_adj)
    _req(knn_idx, torch.int32, 'knn_idx')
    if knn_idx.dim() != 2 or knn_idx.shape[0] != n:
        raise ValueError(f'scene_structure: knn_idx must be [{n}, k_local], got {tuple(knn_idx.shape)}')
    k_local = int(knn_idx.shape[1])
    if not 1 <= k_adj <= k_local:
        raise ValueError(f'scene_structure: 1 <= k_adj <= k_local = {k_local} expected, got {k_adj}')
    if id_mode not in _ID_MODES:
        raise ValueError(f"scene_structure: id_mode must be 'objects', 'labels' or 'given', got {id_mode!r}")
    mode, ids_is_i64 = _ID_MODES[id_mode], 0
    if id_mode == 'given':
        if ids is None or hist is not None:
            raise ValueError("scene_structure: id_mode 'given' takes ids (and no hist)")
        if not torch.is_tensor(ids) or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.shape != (n,):
            raise ValueError(f'scene_structure: ids must be an integer tensor [{n}]')
        if ids.dtype not in (torch.int32, torch.int64):
            ids = ids.to(torch.int64)
        _req(ids, None, 'ids')
        ids_is_i64 = int(ids.dtype == torch.int64)
    else:
        if hist is None or ids is not None:
            raise ValueError(f'scene_structure: id_mode {id_mode!r} takes hist (and no ids)')
        _req(hist, torch.int32, 'hist')
        min_cols = 2 if id_mode == 'objects' else 1                  # 'objects' takes its arg-max from column 1 on
        if hist.dim() != 2 or hist.shape[0] != n or hist.shape[1] < min_cols:
            raise ValueError(f'scene_structure: hist must be [{n}, C] with C >= {min_cols}, got {tuple(hist.shape)}')
    if geof is not None:
        _req(geof, torch.float32, 'geof')
        if geof.shape != (n, 4):
            raise ValueError(f'scene_structure: geof must be [{n}, 4], got {tuple(geof.shape)}')
    if rgb is not None:
        _req(rgb, torch.uint8, 'rgb')
        if rgb.shape != (n, 3):
            raise ValueError(f'scene_structure: rgb must be [{n}, 3], got {tuple(rgb.shape)}')
    L, dev, st = lib(), xyz.device, _stream()
    f32, i64, u8 = torch.float32, torch.int64, torch.uint8
    frame = torch.empty(5, dtype=f32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _workspace(L.spg_structure_frame_workspace_bytes, n, dev=dev)
    check(L.spg_structure_frame(_ptr(xyz), n, _ptr(frame), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_structure_frame')
    _raise_nonfinite(int(err.item()))
    E = n * k_adj
    out = {'elevation': torch.empty(n, dtype=f32, device=dev), 'xyn': torch.empty(n, 2, dtype=f32, device=dev),
           'hard_ids': torch.empty(n, dtype=i64, device=dev), 'geof': geof, 'nei': knn_idx,
           'rgb': torch.empty(n, 3, dtype=f32, device=dev) if rgb is not None else None}
    check(L.spg_structure_vertices(_ptr(xyz), n, _ptr(frame), _ptr(rgb), _ptr(hist), int(hist.shape[1]) if hist is not None else 0, mode,
                                   _ptr(ids), ids_is_i64, _ptr(out['elevation']), _ptr(out['xyn']), _ptr(out['rgb']), _ptr(geof),
                                   _ptr(out['hard_ids']), st), 'spg_structure_vertices')
    out['edg_source'], out['edg_target'] = torch.empty(E, dtype=i64, device=dev), torch.empty(E, dtype=i64, device=dev)
    out['is_transition'], active = torch.empty(E, dtype=u8, device=dev), torch.empty(E, dtype=u8, device=dev)
    check(L.spg_structure_edges(_ptr(knn_idx), n, k_local, k_adj, _ptr(out['hard_ids']), _ptr(out['edg_source']), _ptr(out['edg_target']),
                                _ptr(out['is_transition']), _ptr(active), _ptr(err), st), 'spg_structure_edges')
    _raise_flagged(int(err.item()), {_NEIGHBOUR_RANGE: (IndexError, f'scene_structure: a neighbour index is outside [0, {n})')})
    out['graph'] = EdgeGraph(out['edg_source'], out['edg_target'], n)
    if id_mode == 'labels':
        comp, _, _ = connected_components(out['graph'], active)
        out['objects'] = comp.to(i64)
    else:
        out['objects'] = out['hard_ids']
    return out


# --------------------------------------------------------------------------------------------------
# the ground-plane elevation (csrc/spg_plane.hip; reference supervized_partition/graph_processing.py:181-186, learning/s3dis_dataset.py:130-133)
# --------------------------------------------------------------------------------------------------
PLANE_MAX_TRIALS = 1024
_NO_CONSENSUS, _SUBSET_RANGE = 2, 4      # bits of spg_plane_fit's error word


def ransac_subsets(n_low: int, trials: int = 100, seed: int = 0):
    """The first `trials` triples that sklearn's RANSACRegressor(random_state=seed) draws from n_low samples: the stream of
    sample_without_replacement(n_low, 3, random_state=np.random.RandomState(seed)) -> int64 [trials, 3] (host).  n_low >= 300
    (3 / n_low <= 0.01): tracking selection, randint(n_low) until three distinct values; 4 <= n_low <= 299: permutation(n_low)[:3];
    n_low == 3: (0, 1, 2) without a draw.  sklearn draws lazily, one triple per trial: this is a prefix of the same stream."""
    n_low, trials = int(n_low), int(trials)
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    rs = np.random.RandomState(seed)
    out = np.empty((trials, 3), np.int64)
    for t in range(trials):
        if n_low == 3:
            out[t] = (0, 1, 2)
        elif n_low < 300:
            out[t] = rs.permutation(n_low)[:3]
        else:
            sel = []
            while len(sel) < 3:
                j = int(rs.randint(n_low))
                if j not in sel:
                    sel.append(j)
            out[t] = sel
    return out


def plane_elevation(xyz, subsets=None, seed: int = 0, max_trials: int = 100, low_height: float = 0.5):
    """The elevation of graph_processing.py:181-186 with plane_model: z minus the plane that sklearn 1.7's
    RANSACRegressor(random_state=seed) fits to the points less than low_height above the lowest one, restated on the device
    (csrc/spg_plane.hip): xyz f32 [n, 3] on the device -> dict: elevation f32 [n], coef f64 [2],
    intercept f64 (0-d), threshold f32 (0-d: median |y - median y| in float32, numpy's bits), low_index i32 [n_low], inlier_mask u8
    [n_low] (device tensors) and the host ints n_low, n_trials (what sklearn's n_trials_ counts), best_trial.
    subsets: integer [T, 3], indices into the low points, one triple per trial (T <= 1024 replaces max_trials); None draws
    ransac_subsets(n_low, max_trials, seed) on the host.  Every trial is evaluated; sklearn's acceptance loop is replayed on the
    device.  Host reads: n_low with the error word (ValueError on NaN / infinity before anything else), and the error word with
    n_trials / best_trial at the end (ValueError when no trial found a consensus set, IndexError for a subset index)."""
    n = _scene_xyz(xyz, 'plane_elevation')
    L, dev, st = lib(), xyz.device, _stream()
    low_index = torch.empty(n, dtype=torch.int32, device=dev)
    head = torch.empty(2, dtype=torch.int32, device=dev)                   # n_low, error word: one read
    ws = _workspace(L.spg_plane_workspace_bytes, n, -1, 0, dev=dev)
    check(L.spg_plane_low(_ptr(xyz), n, float(low_height), _ptr(low_index), _ptr(head), _ptr(head[1:]), _ptr(ws), ws.numel(), st), 'spg_plane_low')
    n_low, err = (int(v) for v in head.tolist())
    _raise_nonfinite(err)
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    if subsets is None:
        if not 1 <= int(max_trials) <= PLANE_MAX_TRIALS:
            raise ValueError(f'plane_elevation: 1 <= max_trials <= {PLANE_MAX_TRIALS} expected, got {max_trials}')
        subsets = ransac_subsets(n_low, int(max_trials), seed)
    if not torch.is_tensor(subsets):
        subsets = torch.from_numpy(np.ascontiguousarray(np.asarray(subsets)))
    if subsets.dtype.is_floating_point or subsets.dim() != 2 or subsets.shape[1] != 3 or not 1 <= subsets.shape[0] <= PLANE_MAX_TRIALS:
        raise ValueError(f'plane_elevation: subsets must be an integer array [T, 3] with 1 <= T <= {PLANE_MAX_TRIALS}')
    subsets = subsets.to(device=dev, dtype=torch.int32).contiguous()
    T = int(subsets.shape[0])
    out = {'elevation': torch.empty(n, dtype=torch.float32, device=dev), 'coef': torch.empty(2, dtype=torch.float64, device=dev),
           'intercept': torch.empty((), dtype=torch.float64, device=dev), 'threshold': torch.empty((), dtype=torch.float32, device=dev),
           'low_index': low_index[:n_low], 'inlier_mask': torch.empty(n_low, dtype=torch.uint8, device=dev)}
    tail = torch.zeros(3, dtype=torch.int32, device=dev)                   # n_trials, best_trial, error word
    ws = _workspace(L.spg_plane_workspace_bytes, n, n_low, T, dev=dev)
    check(L.spg_plane_fit(_ptr(xyz), n, _ptr(low_index), n_low, _ptr(subsets), T, _ptr(out['elevation']), _ptr(out['coef']), _ptr(out['intercept']),
                          _ptr(out['threshold']), _ptr(out['inlier_mask']), _ptr(tail), _ptr(tail[2:]), _ptr(ws), ws.numel(), st), 'spg_plane_fit')
    n_trials, best, err = (int(v) for v in tail.tolist())
    _raise_flagged(err, {_SUBSET_RANGE: (IndexError, f'plane_elevation: a subset index is outside [0, {n_low})'),
                         _NO_CONSENSUS: (ValueError, 'RANSAC could not find a valid consensus set. All `max_trials` iterations were skipped '
                                                     'because each randomly chosen sub-sample failed the passing criteria.')})
    out.update(n_low=n_low, n_trials=n_trials, best_trial=best)
    return out


# --------------------------------------------------------------------------------------------------
# parsed superpoint clouds (csrc/spg_parsed.hip; reference learning/{s3dis,sema3d,vkitti,custom}_dataset.py: preprocess_pointclouds)
# --------------------------------------------------------------------------------------------------
PARSED_RECIPES = {'s3dis': (0, 15), 'sema3d': (1, 11), 'custom': (1, 11), 'vkitti': (2, 14)}      # name -> (SPG_PARSED_*, columns)
CLASS_COUNT_MAX = 4096
_COMPONENT_INDEX_RANGE, _TRIM_RANGE = 2, 4      # bits of spg_parsed_rows' error word


def scene_stats(xyz, with_distance: bool = False):
    """The statistics preprocess_pointclouds takes of a scene, by fixed-order reductions (the same input gives the same bits):
    xyz f32 [n, 3] on the device -> (stats_f32 [6] = min x, y, z, max x, y, z; stats_f64 [5] = mean x, y, z and, with_distance,
    the mean and population standard deviation of the distance to the room centre in float64; centroid f32 [3]), device tensors.
    One host read: the error word (ValueError on NaN / infinity)."""
    n = _scene_xyz(xyz, 'scene_stats')
    L, dev = lib(), xyz.device
    s32, s64 = torch.empty(6, dtype=torch.float32, device=dev), torch.empty(5, dtype=torch.float64, device=dev)
    centroid, err = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = _workspace(L.spg_parsed_workspace_bytes, n, dev=dev)
    check(L.spg_parsed_stats(_ptr(xyz), n, int(bool(with_distance)), _ptr(s32), _ptr(s64), _ptr(centroid), _ptr(err), _ptr(ws), ws.numel(),
                             _stream()), 'spg_parsed_stats')
    _raise_nonfinite(int(err.item()))
    return s32, s64, centroid


def parsed_points(recipe, xyz, rgb, comp_off, comp_idx, geof=None, elevation=None, trim=None, lpsv_raw: bool = False):
    """The datasets preprocess_pointclouds writes for one scene, as one device buffer (csrc/spg_parsed.hip, DESIGN.md section
    4.11h).  recipe 's3dis' (15 columns: xyz, rgb, e, lpsv[4], xyzn[3], dist), 'sema3d' / 'custom' (11: xyz, rgb, z / 100,
    geof - 0.5) or 'vkitti' (14: xyz, rgb, e, four zeros, xyzn).  xyz f32 [n, 3]; rgb u8 | f32 [n, 3]; geof f32 [n, 4] (not for
    vkitti); s3dis: elevation f32 [n] or None (z / 4 - 0.5), lpsv_raw: geof unchanged (supervized_partition).  Component c owns
    comp_idx[comp_off[c] : comp_off[c + 1]] (comp_off i64 [C + 1], host or device; comp_idx i32 | i64 [M] on the device; a vertex
    may appear in no component or in several).  trim: {component: positions inside it (integer sequence)} -- the component's rows
    are then comp_idx[comp_off[c] + positions], in that order.
    -> points f32 [Ntot, ncols] with the rows of component 0, 1, ... back to back, centroid f32 [3] (device), offsets i64 [C + 1]
    (host numpy).  Host traffic: comp_off down when it lives on the device, the offset and trim tables up, two reads of the error
    word (ValueError for NaN / infinity, IndexError for a component index or a trim position out of range)."""
    if recipe not in PARSED_RECIPES:
        raise ValueError(f'parsed_points: recipe must be one of {sorted(PARSED_RECIPES)}, got {recipe!r}')
    code, ncols = PARSED_RECIPES[recipe]
    n, dev = _scene_xyz(xyz, 'parsed_points'), xyz.device
    _req(rgb, None, 'rgb')
    if rgb.dtype not in (torch.uint8, torch.float32) or rgb.shape != (n, 3):
        raise ValueError(f'parsed_points: rgb must be uint8 or float32 [{n}, 3]')
    if code != 2:
        if geof is None:
            raise ValueError(f'parsed_points: recipe {recipe!r} needs geof')
        _req(geof, torch.float32, 'geof')
        if geof.shape != (n, 4):
            raise ValueError(f'parsed_points: geof must be [{n}, 4], got {tuple(geof.shape)}')
    else:
        geof = None
    if elevation is not None:
        if code != 0:
            raise ValueError("parsed_points: only recipe 's3dis' takes an elevation")
        _req(elevation, torch.float32, 'elevation')
        if elevation.shape != (n,):
            raise ValueError(f'parsed_points: elevation must be [{n}], got {tuple(elevation.shape)}')
    _req(comp_idx, None, 'comp_idx')
    if comp_idx.dtype not in (torch.int32, torch.int64) or comp_idx.dim() != 1:
        raise ValueError('parsed_points: comp_idx must be int32 or int64 [M]')
    M = int(comp_idx.numel())
    src_h = (comp_off.cpu().numpy() if torch.is_tensor(comp_off) else np.asarray(comp_off)).astype(np.int64).reshape(-1)
    C = len(src_h) - 1
    if C < 1 or src_h[0] != 0 or src_h[-1] > M or (np.diff(src_h) < 0).any():
        raise ValueError(f'parsed_points: comp_off must be [C + 1] with C >= 1, ascending from 0 to at most {M}')
    sizes = np.diff(src_h)
    out_sizes, trim_off_h, trim_parts, n_trim = sizes.copy(), None, [], 0
    if trim:
        trim_off_h = np.full(C, -1, np.int64)
        for c in sorted(trim):
            pos = np.asarray(trim[c])
            if not 0 <= int(c) < C or pos.ndim != 1 or pos.dtype.kind not in 'iu':
                raise ValueError(f'parsed_points: trim maps a component in [0, {C}) to a 1-d integer array')
            if pos.size and (pos.max() >= 2 ** 31 or pos.min() < -2 ** 31):
                raise IndexError(f'parsed_points: a trim position of component {c} is outside [0, {int(sizes[c])})')
            trim_off_h[c], out_sizes[c] = n_trim, pos.size
            trim_parts.append(pos.astype(np.int32))
            n_trim += pos.size
    off_h = np.zeros(C + 1, np.int64)
    np.cumsum(out_sizes, out=off_h[1:])
    n_rows = int(off_h[-1])
    if n_rows >= 2 ** 31 - 1:
        raise ValueError('parsed_points: fewer than 2^31 - 1 rows expected')
    L, st = lib(), _stream()
    s32, s64, centroid = scene_stats(xyz, code == 0)        # (sema3d reads no statistic: the centroid and the finite check)
    out_off_d, src_off_d = torch.from_numpy(off_h).to(dev), torch.from_numpy(src_h).to(dev)
    trim_off_d = trim_d = None
    if trim_off_h is not None:          # (one spare entry: the table is never empty)
        trim_off_d, trim_d = torch.from_numpy(trim_off_h).to(dev), torch.from_numpy(np.concatenate(trim_parts + [np.zeros(1, np.int32)])).to(dev)
    points = torch.empty(n_rows, ncols, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.spg_parsed_rows(code, _ptr(xyz), n, _ptr(rgb), int(rgb.dtype == torch.float32), _ptr(geof), _ptr(elevation), int(bool(lpsv_raw)),
                            _ptr(s32), _ptr(s64), _ptr(out_off_d), _ptr(src_off_d), C, _ptr(comp_idx), int(comp_idx.dtype == torch.int64),
                            _ptr(trim_d), _ptr(trim_off_d), n_rows, _ptr(points), _ptr(err), st), 'spg_parsed_rows')
    _raise_flagged(int(err.item()), {_COMPONENT_INDEX_RANGE: (IndexError, f'parsed_points: a component index is outside [0, {n})'),
                                     _TRIM_RANGE: (IndexError, 'parsed_points: a trim position is outside its component')})
    return points, centroid, off_h


def class_count(labels, n_classes: int):
    """np.bincount(np.argmax(labels[:, 1:], 1), minlength=n_classes) of the label histograms labels u32 | i32 [n, n_classes + 1] on
    the device (first maximum; an all-zero row counts for class 0) -> i64 [n_classes] on the device."""
    n_classes = int(n_classes)
    _req(labels, None, 'labels')
    if labels.dtype not in (torch.int32, torch.uint32):
        raise TypeError(f'class_count: labels must be uint32 or int32, got {labels.dtype}')
    if not 1 <= n_classes <= CLASS_COUNT_MAX:
        raise ValueError(f'class_count: 1 <= n_classes <= {CLASS_COUNT_MAX} expected, got {n_classes}')
    if labels.dim() != 2 or labels.shape[1] != n_classes + 1:
        raise ValueError(f'class_count: labels must be [n, {n_classes + 1}], got {tuple(labels.shape)}')
    count = torch.empty(n_classes, dtype=torch.int64, device=labels.device)
    check(lib().spg_class_count(_ptr(labels), int(labels.dtype == torch.int32), int(labels.shape[0]), n_classes, _ptr(count), _stream()),
          'spg_class_count')
    return count
