"""Superpoint-graph construction, geometric features, voxel pruning and the exact kNN index (csrc/spg_spgraph.hip, spg_knn.hip)."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._core import _ptr, _raise_flagged, _req, _stream, _workspace


# --------------------------------------------------------------------------------------------------
# superpoint-graph construction (partition/graphs.py compute_sp_graph after the triangulation, ply_c compute_geof)
# --------------------------------------------------------------------------------------------------
def sp_graph(xyz, comp, n_com: int, tets, d_max: float, labels=None, label_rows=None, n_labels: int = 0):
    """xyz f32 [n,3], comp i32 [n], tets i32 [T,4] (Delaunay simplices), all on the device -> dict of device tensors with the
    keys of the reference's compute_sp_graph (partition/graphs.py:75-210).  Three host synchronisations (the numbers of raw
    interface pairs, unique edges and superedges size the next stage's buffers)."""
    _req(xyz, torch.float32, 'xyz'); _req(comp, torch.int32, 'comp'); _req(tets, torch.int32, 'tets')
    L, dev, st = lib(), xyz.device, _stream()
    n, T = int(xyz.shape[0]), int(tets.shape[0])
    if xyz.dim() != 2 or xyz.shape[1] != 3 or comp.numel() != n or (T and tets.shape[1] != 4):
        raise ValueError('sp_graph: xyz [n,3], comp [n], tets [T,4] expected')
    u64, f32 = torch.int64, torch.float32                 # (torch has no uint64 arithmetic: int64 storage, the library reads it unsigned)
    cnt = torch.zeros(1, dtype=u64, device=dev)
    # ---- superpoints (graphs.py:141-172) ----
    out = {'sp_centroids': torch.empty(n_com, 3, dtype=f32, device=dev), 'sp_length': torch.empty(n_com, 1, dtype=f32, device=dev),
           'sp_surface': torch.empty(n_com, 1, dtype=f32, device=dev), 'sp_volume': torch.empty(n_com, 1, dtype=f32, device=dev),
           'sp_point_count': torch.empty(n_com, 1, dtype=u64, device=dev)}
    sp_labels = None
    if labels is not None or label_rows is not None:
        sp_labels = torch.empty(n_com, n_labels + 1, dtype=torch.int32, device=dev)
        if labels is not None:
            _req(labels, torch.int32, 'labels')
        else:
            _req(label_rows, torch.int32, 'label_rows')
    ws = _workspace(L.spg_spg_workspace_bytes, 2, n, dev=dev)
    check(L.spg_spg_superpoints(_ptr(xyz), n, _ptr(comp), n_com, _ptr(labels), _ptr(label_rows), n_labels, _ptr(out['sp_centroids']),
                                _ptr(out['sp_length']), _ptr(out['sp_surface']), _ptr(out['sp_volume']), _ptr(out['sp_point_count']),
                                _ptr(sp_labels), _ptr(ws), ws.numel(), st), 'spg_spg_superpoints')
    out['sp_labels'] = sp_labels
    # ---- interface edges of the tetrahedra, unique, shorter than d_max (:85-113) ----
    keys = torch.empty(max(12 * T, 1), dtype=u64, device=dev)
    check(L.spg_spg_tet_edges(_ptr(tets) if T else None, T, _ptr(comp), _ptr(keys), 12 * T, _ptr(cnt), st), 'spg_spg_tet_edges')
    n_raw = int(cnt.item())
    edge_keys = torch.empty(max(n_raw, 1), dtype=u64, device=dev)
    cc_keys = torch.empty(max(n_raw, 1), dtype=u64, device=dev)
    ws = _workspace(L.spg_spg_workspace_bytes, 0, n_raw, dev=dev)
    check(L.spg_spg_unique_edges(_ptr(keys), n_raw, _ptr(xyz), _ptr(comp), n_com, float(d_max), _ptr(edge_keys), _ptr(cc_keys), _ptr(cnt),
                                 _ptr(ws), ws.numel(), st), 'spg_spg_unique_edges')
    n_edg = int(cnt.item())
    # ---- ordered by component pair, superedge segments (:117-128) ----
    cc_sorted = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    edges_sorted = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    seg_cc = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    seg_off = torch.empty(n_edg + 1, dtype=u64, device=dev)
    ws = _workspace(L.spg_spg_workspace_bytes, 1, n_edg, dev=dev)
    check(L.spg_spg_group_edges(_ptr(cc_keys), _ptr(edge_keys), n_edg, _ptr(cc_sorted), _ptr(edges_sorted), _ptr(seg_cc), _ptr(seg_off),
                                _ptr(cnt), _ptr(ws), ws.numel(), st), 'spg_spg_group_edges')
    n_sedg = int(cnt.item())
    # ---- superedge features (:174-208) ----
    se = {'source': torch.empty(n_sedg, 1, dtype=torch.int32, device=dev), 'target': torch.empty(n_sedg, 1, dtype=torch.int32, device=dev)}
    for k, w in (('se_delta_mean', 3), ('se_delta_std', 3), ('se_delta_norm', 1), ('se_delta_centroid', 3), ('se_length_ratio', 1),
                 ('se_surface_ratio', 1), ('se_volume_ratio', 1), ('se_point_count_ratio', 1)):
        se[k] = torch.empty(n_sedg, w, dtype=f32, device=dev)
    check(L.spg_spg_superedges(_ptr(edges_sorted), _ptr(seg_cc), _ptr(seg_off), n_sedg, n_com, _ptr(xyz), _ptr(out['sp_centroids']),
                               _ptr(out['sp_length']), _ptr(out['sp_surface']), _ptr(out['sp_volume']), _ptr(out['sp_point_count']),
                               _ptr(se['source']), _ptr(se['target']), _ptr(se['se_delta_mean']), _ptr(se['se_delta_std']),
                               _ptr(se['se_delta_norm']), _ptr(se['se_delta_centroid']), _ptr(se['se_length_ratio']),
                               _ptr(se['se_surface_ratio']), _ptr(se['se_volume_ratio']), _ptr(se['se_point_count_ratio']), st),
          'spg_spg_superedges')
    out.update(se)
    out['edges'] = edges_sorted[:n_edg]                    # (source << 32 | target) of every Delaunay edge behind the superedges
    out['seg_off'] = seg_off[:n_sedg + 1]
    return out


def compute_geof(xyz, target, k_nn: int):
    """xyz f32 [n,3], target (u)int32 [n * k_nn] neighbour indices on the device -> geof f32 [n,4] (ply_c.cpp:384-462)."""
    _req(xyz, torch.float32, 'xyz'); _req(target, torch.int32, 'target')
    n = int(xyz.shape[0])
    if target.numel() != n * k_nn:
        raise ValueError(f'compute_geof: {n} points x {k_nn} neighbours need {n * k_nn} targets, got {target.numel()}')
    geof = torch.empty(n, 4, dtype=torch.float32, device=xyz.device)
    check(lib().spg_compute_geof(_ptr(xyz), _ptr(target), n, int(k_nn), _ptr(geof), _stream()), 'spg_compute_geof')
    return geof


_VOXEL_RANGE, _ID_RANGE = 1, 2      # bits of the error word of spg_prune_voxels and spg_prune_reduce


def prune(xyz, voxel_size: float, rgb=None, labels=None, objects=None, n_labels: int = 0, n_objects: int = 0):
    """Voxel-grid subsampling (ply_c.cpp:288-382) of device tensors: xyz f32 [n,3], rgb u8 [n,3] or None, labels u8 [n] or None,
    objects i32 [n] (read as uint32) or None -> (xyz f32 [V,3], rgb u8 [V,3], labels i32 [V, n_labels+1], objects i32 [V, n_objects+1]);
    voxels in the order of their first point.  One host synchronisation (the number of voxels)."""
    _req(xyz, torch.float32, 'xyz')
    L, dev, st = lib(), xyz.device, _stream()
    n = int(xyz.shape[0])
    if rgb is not None:
        _req(rgb, torch.uint8, 'rgb')
    if labels is not None:
        _req(labels, torch.uint8, 'labels')
    if objects is not None:
        _req(objects, torch.int32, 'objects')
    ws = _workspace(L.spg_prune_workspace_bytes, n, dev=dev)
    nv = torch.zeros(1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.spg_prune_voxels(_ptr(xyz), n, float(voxel_size), _ptr(nv), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_prune_voxels')
    V = int(nv.item())
    _raise_flagged(int(err.item()), {_VOXEL_RANGE: (ValueError, 'prune: more than 2^21 voxels along an axis (voxel_size too small for the '
                                                                'extent of the cloud)')})
    out_xyz = torch.empty(V, 3, dtype=torch.float32, device=dev)
    out_rgb = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    out_lab = torch.empty(V, n_labels + 1, dtype=torch.int32, device=dev)
    out_obj = torch.empty(V, n_objects + 1, dtype=torch.int32, device=dev)
    check(L.spg_prune_reduce(_ptr(xyz), _ptr(rgb), _ptr(labels), _ptr(objects), n, V, int(n_labels), int(n_objects), _ptr(out_xyz),
                             _ptr(out_rgb), _ptr(out_lab), _ptr(out_obj), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_prune_reduce')
    _raise_flagged(int(err.item()), {_ID_RANGE: (IndexError, 'prune: a label / object id exceeds n_labels / n_objects')})
    return out_xyz, out_rgb, out_lab, out_obj


_KNN_NONFINITE = 1      # bit of the error word of spg_knn_build and spg_knn_query
KNN_MAX_K = 47          # k + 1 <= 48: the largest top-k list the query kernels keep in registers without scratch


class KnnIndex:
    """Exact k-nearest-neighbour index of a device point set (csrc/spg_knn.hip): ref_xyz f32 [n,3] on the GPU, indexed once
    into a uniform grid; query() / self_query() answer on the device.  Order: float64 squared distance (dx*dx + dy*dy) + dz*dz
    (no fused multiply-add), ties by point index; self queries drop the query point itself.  The results do not depend on
    cell_size (None = automatic, ~32 points per occupied cell; a value is for tuning and tests).  query_capacity: the largest
    query set the workspace is sized for in one internal chunk (larger sets are streamed in chunks)."""

    def __init__(self, ref_xyz, cell_size=None, query_capacity: int = 0):
        _req(ref_xyz, torch.float32, 'ref_xyz')
        if ref_xyz.dim() != 2 or ref_xyz.shape[1] != 3:
            raise ValueError(f'knn: ref_xyz must be [n, 3], got {tuple(ref_xyz.shape)}')
        n = int(ref_xyz.shape[0])
        if n == 0:
            raise ValueError('knn: empty reference set')
        if n >= 2 ** 32 - 1:
            raise ValueError('knn: point indices are uint32: at most 2^32 - 2 reference points')
        if cell_size is not None and not (float(cell_size) > 0.0):
            raise ValueError(f'knn: cell_size must be > 0, got {cell_size}')
        L, dev = lib(), ref_xyz.device
        self.ref, self.n = ref_xyz, n
        self.ws = _workspace(L.spg_knn_workspace_bytes, n, int(query_capacity), 1, dev=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        check(L.spg_knn_build(_ptr(ref_xyz), n, float(cell_size or 0.0), _ptr(self.err), _ptr(self.ws), self.ws.numel(), _stream()),
              'spg_knn_build')

    def _k(self, k, n_avail):
        k = int(k)
        if k < 1:
            raise ValueError(f'knn: k must be >= 1, got {k}')
        if k + 1 > KNN_MAX_K + 1:
            raise ValueError(f'knn: k + 1 = {k + 1} exceeds the limit of {KNN_MAX_K + 1} (k <= {KNN_MAX_K})')
        if k > n_avail:
            raise ValueError(f'knn: Expected n_neighbors <= n_samples, but n_samples = {self.n}, n_neighbors = '
                             f'{k + 1 if n_avail < self.n else k}')
        return k

    def _run(self, q, nq, k, self_query, distances):
        dev = self.ref.device
        idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
        dist = torch.empty(nq, k, dtype=torch.float32, device=dev) if distances else None
        check(lib().spg_knn_query(_ptr(q), nq, self.n, k, int(self_query), _ptr(idx), _ptr(dist), _ptr(self.err), _ptr(self.ws),
                                  self.ws.numel(), _stream()), 'spg_knn_query')
        _raise_flagged(int(self.err.item()), {_KNN_NONFINITE: (ValueError, 'knn: the input contains NaN or infinity')})
        return idx, dist

    def query_chunk(self, n_query: int) -> int:
        """queries per internal chunk that query() uses for n_query queries on this index's workspace."""
        return int(lib().spg_knn_query_chunk(self.n, int(n_query), self.ws.numel()))

    def self_query(self, k, distances=True):
        """k nearest other points of every reference point -> (idx i32 [n, k], dist f32 [n, k] or None)."""
        return self._run(None, self.n, self._k(k, self.n - 1), True, distances)

    def query(self, query_xyz, k, distances=True):
        """k nearest reference points of every query point -> (idx i32 [m, k], dist f32 [m, k] or None)."""
        _req(query_xyz, torch.float32, 'query_xyz')
        if query_xyz.dim() != 2 or query_xyz.shape[1] != 3:
            raise ValueError(f'knn: query_xyz must be [m, 3], got {tuple(query_xyz.shape)}')
        nq = int(query_xyz.shape[0])
        if nq >= 2 ** 32 - 1:
            raise ValueError('knn: at most 2^32 - 2 query points per call')
        return self._run(query_xyz, nq, self._k(k, self.n), False, distances)


def knn(ref_xyz, k: int, query_xyz=None, cell_size=None, distances: bool = True):
    """Exact k nearest neighbours on the device (sklearn NearestNeighbors(algorithm='kd_tree') in the reference's
    partition/graphs.py:11-73 and provider.py:681-687).  ref_xyz f32 [n,3]; query_xyz f32 [m,3] or None = self query (the point
    itself is dropped) -> (idx int32 [m, k], distances float32 [m, k] or None), in query order.  1 <= k <= KNN_MAX_K."""
    index = KnnIndex(ref_xyz, cell_size, 0 if query_xyz is None else int(query_xyz.shape[0]))
    if query_xyz is None:
        return index.self_query(k, distances)
    return index.query(query_xyz, k, distances)
