"""Batches of the learned partition: neighbourhood tiles, whole-cloud augmentation, random and induced subgraphs (csrc/spg_tiles.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib
from ._core import _indicator, _on_gpu, _ptr, _raise_flagged, _req, _scene_array, _stream, _workspace
from .edges import EdgeGraph


# --------------------------------------------------------------------------------------------------
# batches of the learned partition on the device (csrc/spg_tiles.hip; reference supervized_partition/graph_processing.py:347-436,
# :534-546, partition/ply_c/random_subgraph.cpp)
# --------------------------------------------------------------------------------------------------
TILES_MAX_K = 64
TILES_VERTICES_PER_BLOCK = 32      # selected vertices one workgroup of the tile kernel takes
_GLOBAL_FEAT_KEYS = ('e', 'rgb', 'XY', 'xy')
_INDEX_RANGE = 1      # bit of the error word of spg_neighbourhood_tiles (nei, rows) and spg_random_subgraph (a seed)


def neighbourhood_tiles(xyz, nei, k: int, rows=None, rgb=None, global_feat='', elevation=None, xyn=None, cloud_rgb=True,
                        stream_stores=True):
    """The tiles of graph_loader (graph_processing.py:389-411) -> (clouds f32 [m, 3 or 6, k], clouds_global f32 [m, G], diameters
    f32 [m]), bit for bit what numpy computes in float32: xyz f32 [N, 3]; nei int32 / int64 [N, K >= k], indices into the full
    cloud, 1 <= k <= 64; rows: ascending ids of the selected vertices (int64 [m]; None = all); rgb f32 [N, 3] (already / 255) adds the
    neighbours' colours as channels 3..5 unless cloud_rgb is False (the reference's use_rgb = 0, which still needs rgb for the
    'rgb' global feature).  clouds_global = diameters, then per key that is a substring of global_feat, in this order: 'e'
    elevation f32 [N], 'rgb' the vertex's own rgb, 'XY' xyn f32 [N, 2], 'xy' xyz[rows, :2].  stream_stores: non-temporal stores
    of clouds (the faster form wherever the two differed: profiles/tiles_bench.txt).  An index outside [0, N) in nei or rows raises IndexError (one host synchronisation)."""
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError('xyz must be a [N, 3] tensor')
    N, k = int(xyz.shape[0]), int(k)
    xyz = _scene_array(xyz, (N, 3), 'xyz')
    _on_gpu(nei, 'nei')
    if nei.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'nei must be int32 or int64, got {nei.dtype}')
    if nei.dim() != 2 or nei.shape[0] != N:
        raise ValueError(f'nei must be [{N}, K], got {list(nei.shape)}')
    K = int(nei.shape[1])
    if not (1 <= k <= TILES_MAX_K and k <= K):
        raise ValueError(f'1 <= k <= {TILES_MAX_K} and k <= K = {K} expected, got k = {k}')
    if not 1 <= N < 2 ** 31 - 1:
        raise ValueError(f'1 <= N < 2^31 - 1 expected, got N = {N}')
    nei = _req(nei.contiguous(), None, 'nei')
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dim() != 1:
            raise ValueError('rows must be a [m] tensor')
        rows = _req(rows.to(torch.int64).contiguous(), torch.int64, 'rows')
        m = int(rows.numel())
    else:
        m = N
    want = {key: key in global_feat for key in _GLOBAL_FEAT_KEYS}
    if rgb is not None:
        rgb = _scene_array(rgb, (N, 3), 'rgb')
    elif want['rgb']:
        raise ValueError("global_feat has 'rgb' but rgb is None")
    if want['e']:
        if elevation is None:
            raise ValueError("global_feat has 'e' but elevation is None")
        elevation = _scene_array(elevation.reshape(-1) if torch.is_tensor(elevation) else elevation, (N,), 'elevation')
    if want['XY']:
        if xyn is None:
            raise ValueError("global_feat has 'XY' but xyn is None")
        xyn = _scene_array(xyn, (N, 2), 'xyn')
    cloud_rgb = bool(cloud_rgb) and rgb is not None
    F = 6 if cloud_rgb else 3
    G = 1 + (1 if want['e'] else 0) + (3 if want['rgb'] else 0) + (2 if want['XY'] else 0) + (2 if want['xy'] else 0)
    dev = xyz.device
    clouds = torch.empty(m, F, k, dtype=torch.float32, device=dev)
    clouds_global = torch.empty(m, G, dtype=torch.float32, device=dev)
    diameters = torch.empty(m, dtype=torch.float32, device=dev)
    if m == 0:
        return clouds, clouds_global, diameters
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().spg_neighbourhood_tiles(_ptr(xyz), _ptr(rgb), N, _ptr(nei), 1 if nei.dtype == torch.int64 else 0, K, k, _ptr(rows), m,
                                        1 if cloud_rgb else 0, _ptr(elevation) if want['e'] else None, _ptr(xyn) if want['XY'] else None,
                                        1 if want['rgb'] else 0, 1 if want['xy'] else 0, 1 if stream_stores else 0, _ptr(clouds),
                                        _ptr(clouds_global), _ptr(diameters), _ptr(err), _stream()), 'spg_neighbourhood_tiles')
    _raise_flagged(int(err.item()), {_INDEX_RANGE: (IndexError, f'neighbourhood_tiles: an index in nei or rows is outside [0, {N})')})
    return clouds, clouds_global, diameters


def _host_f32(a, shape, name):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
    if a.shape != shape:
        raise ValueError(f'{name} must be {list(shape)}, got {list(a.shape)}')
    return a


def augment_whole(xyz, rgb, ref_point=None, M=None, noise_xyz=None, noise_rgb=None):
    """augment_cloud_whole (graph_processing.py:534-546) with the random quantities as inputs (drawn and clipped by the caller, so
    the reference's random stream stays usable) -> (xyz, rgb): xyz = ((xyz - ref_point) @ M + ref_point) + noise_xyz, every
    product and sum rounded on its own in float32; rgb = clip(rgb + noise_rgb, -1, 1).  ref_point [3] and M [3, 3] are host values
    (both or neither; the caller sets ref_point[2] = 0 as the reference does); noise_* f32 [N, 3] device tensors.  Every argument
    that is None leaves its part out: with all of them None the inputs are returned as they are.  rgb may be None."""
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError('xyz must be a [N, 3] tensor')
    N = int(xyz.shape[0])
    xyz = _scene_array(xyz, (N, 3), 'xyz')
    if (M is None) != (ref_point is None):
        raise ValueError('augment_whole: ref_point and M come together')
    if rgb is not None:
        rgb = _scene_array(rgb, (N, 3), 'rgb')
    elif noise_rgb is not None:
        raise ValueError('augment_whole: noise_rgb needs rgb')
    if M is None and noise_xyz is None and noise_rgb is None:
        return xyz, rgb
    Mh = rh = None
    if M is not None:
        Mh, rh = _host_f32(M, (3, 3), 'M'), _host_f32(ref_point, (3,), 'ref_point')
    if noise_xyz is not None:
        noise_xyz = _scene_array(noise_xyz, (N, 3), 'noise_xyz')
    if noise_rgb is not None:
        noise_rgb = _scene_array(noise_rgb, (N, 3), 'noise_rgb')
    xyz_out = torch.empty_like(xyz)
    rgb_out = torch.empty_like(rgb) if noise_rgb is not None else None
    check(lib().spg_augment_whole(_ptr(xyz), _ptr(rgb), N, Mh.ctypes.data if Mh is not None else None,
                                  rh.ctypes.data if rh is not None else None, _ptr(noise_xyz), _ptr(noise_rgb), _ptr(xyz_out),
                                  _ptr(rgb_out), _stream()), 'spg_augment_whole')
    return xyz_out, (rgb_out if rgb_out is not None else rgb)


def random_subgraph(graph: EdgeGraph, subgraph_size: int, seeds, state=None):
    """libply_c.random_subgraph (partition/ply_c/random_subgraph.cpp) with the seed vertices as an explicit int64 sequence, consumed
    in order, in place of the reference's unseeded rand() -> (selected_edg u8 [E], selected_ver u8 [n], n_seen, n_seeds_used,
    state).  Its queue discipline is reproduced: an already selected seed is skipped but consumed; neighbours are visited in
    adjacency order (ascending edge id, as Boost inserts them); once n_seen reaches subgraph_size every vertex still in the queue
    examines its first adjacency slot only and the first unselected one of those is accepted, so n_seen is usually
    subgraph_size + 1.  subgraph_size > n raises ValueError (the reference writes out of bounds there).  When the seeds run out
    first, n_seen < subgraph_size; a further call with more seeds and the returned state continues.  A seed outside [0, n) raises
    IndexError.  One host synchronisation."""
    graph._use()
    n, E, dev = graph.n, graph.E, graph.device
    subgraph_size = int(subgraph_size)
    if subgraph_size > n:
        raise ValueError(f'random_subgraph: subgraph_size = {subgraph_size} exceeds the {n} vertices of the graph')
    if subgraph_size < 0:
        raise ValueError(f'random_subgraph: subgraph_size >= 0 expected, got {subgraph_size}')
    if not torch.is_tensor(seeds):
        seeds = torch.as_tensor(seeds, dtype=torch.int64)
    if seeds.dim() != 1 or seeds.dtype.is_floating_point:
        raise ValueError('random_subgraph: seeds must be an integer [n_seeds] sequence')
    seeds = _req(seeds.to(device=dev, dtype=torch.int64).contiguous(), torch.int64, 'seeds')
    if state is None:
        selected_ver = torch.zeros(n, dtype=torch.uint8, device=dev)
        n_seen = 0
    else:
        selected_ver, n_seen = state
        selected_ver = _req(selected_ver, torch.uint8, 'state')
        if selected_ver.shape != (n,):
            raise ValueError(f'random_subgraph: state belongs to a graph of {selected_ver.numel()} vertices, this one has {n}')
        selected_ver = selected_ver.clone()
    L = lib()
    st = torch.tensor([int(n_seen), 0, 0], dtype=torch.int64).to(dev)
    selected_edg = torch.empty(E, dtype=torch.uint8, device=dev)
    ws = _workspace(L.spg_random_subgraph_workspace_bytes, n, dev=dev)
    check(L.spg_random_subgraph(_ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends), E, n, subgraph_size, _ptr(seeds), int(seeds.numel()),
                                _ptr(selected_ver), _ptr(selected_edg), _ptr(st), _ptr(ws), ws.numel(), _stream()), 'spg_random_subgraph')
    n_seen, used, err = (int(v) for v in st.tolist())
    _raise_flagged(err, {_INDEX_RANGE: (IndexError, f'random_subgraph: seed {used} is outside [0, {n})')})
    return selected_edg, selected_ver, n_seen, used, (selected_ver, n_seen)


def induced_subgraph(graph: EdgeGraph, selected_ver, selected_edg):
    """graph_processing.py:375-379 on the device -> (rows i64 [m] the selected vertices ascending, new_ver_index i64 [n] with -1
    where unselected, kept i64 [E'] the selected edge ids in order, edg_source i64 [E'], edg_target i64 [E'] =
    new_ver_index[end points of the kept edges]).  Scans on the device; one host read (the two counts)."""
    graph._use()
    n, E, dev = graph.n, graph.E, graph.device
    sv = _indicator(selected_ver, n, 'selected_ver')
    se = _indicator(selected_edg, E, 'selected_edg')
    L, i64 = lib(), torch.int64
    rows = torch.empty(n, dtype=i64, device=dev)
    new_ver_index = torch.empty(n, dtype=i64, device=dev)
    kept, src, tgt = (torch.empty(E, dtype=i64, device=dev) for _ in range(3))
    counts = torch.empty(2, dtype=i64, device=dev)
    ws = _workspace(L.spg_induced_subgraph_workspace_bytes, n, E, dev=dev)
    check(L.spg_induced_subgraph(_ptr(graph.ends), E, n, _ptr(sv), _ptr(se), _ptr(rows), _ptr(new_ver_index), _ptr(kept), _ptr(src), _ptr(tgt),
                                 _ptr(counts), _ptr(ws), ws.numel(), _stream()), 'spg_induced_subgraph')
    m, Ek = (int(v) for v in counts.tolist())
    return rows[:m], new_ver_index, kept[:Ek], src[:Ek], tgt[:Ek]
