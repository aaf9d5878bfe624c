"""numpy restatement of the scene structure of the learned partition (what csrc/spg_structure.hip and
supervized_partition.graph_processing.build_structure compute), written from the formulas:

    hard id of a histogram row   objects: first arg-max over columns 1 ... C - 1, as a column number (an all-zero row: 1)
                                 labels:  first arg-max over all columns (an all-zero row: 0)
    adjacency                    source = every vertex k_adj times, target = the first k_adj columns of the kNN table
    is_transition                id[source] != id[target]
    objects (labels rule)        components over the edges that are no transition, numbered by smallest member
    elevation                    z - min z                              } float32 at every step
    xyn                          (xy - min xy) / ((max xy - min xy) + float32(1e-8))
    geof                         column 3 doubled
    clouds (geof / geofrgb)      geof, or geof with rgb / 255 appended

The steps that have restatements already are taken from there: prune and geof (oracle.spg_partition_oracle), the kNN order
(tests/knn_restatement.py), the components (tests/edge_loss_restatement.py)."""
import numpy as np

import edge_loss_restatement as ELR
import knn_restatement as KR
from oracle import spg_partition_oracle as P

F32 = np.float32


def hard_ids(hist, rule):
    """rule 'objects' | 'labels' -> int64 [n]."""
    hist = np.asarray(hist)
    first = 1 if rule == 'objects' else 0
    best = hist[:, first:].max(1, keepdims=True)
    return (first + (hist[:, first:] == best).argmax(1)).astype(np.int64)      # argmax of a bool row: its first True


def adjacency(nei, k_adj):
    nei = np.asarray(nei, dtype=np.int64)
    n = len(nei)
    return np.arange(n, dtype=np.int64).repeat(k_adj), nei[:, :k_adj].reshape(-1).copy()


def frame_values(xyz):
    """elevation f32 [n], xyn f32 [n, 2]: one rounding per operation."""
    xyz = np.asarray(xyz, dtype=F32)
    elevation = xyz[:, 2] - xyz[:, 2].min()
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    extent = (hi - lo).astype(F32)
    denom = (extent + F32(1e-8)).astype(F32)
    xyn = ((xyz[:, :2] - lo).astype(F32) / denom).astype(F32)
    return elevation.astype(F32), xyn


def structure(xyz, nei, k_adj, ids, rule, geof=None):
    """ids: int [n] with rule 'given', a histogram [n, C] otherwise -> dict like ops.scene_structure's (numpy)."""
    hid = np.asarray(ids, dtype=np.int64).reshape(-1) if rule == 'given' else hard_ids(ids, rule)
    src, tgt = adjacency(nei, k_adj)
    trans = (hid[src] != hid[tgt]).astype(np.uint8)
    if rule == 'labels':
        objects = ELR.components(len(hid), src, tgt, 1 - trans)[0].astype(np.int64)
    else:
        objects = hid
    elevation, xyn = frame_values(xyz)
    out = dict(edg_source=src, edg_target=tgt, is_transition=trans, hard_ids=hid, objects=objects, elevation=elevation, xyn=xyn,
               nei=np.asarray(nei, dtype=np.uint32))
    if geof is not None:
        g = np.array(geof, dtype=F32)
        g[:, 3] = F32(2) * g[:, 3]
        out['geof'] = g
    return out


def build(xyz, rgb, labels, objects, dataset, n_labels, voxel_width, k_local, k_adj):
    """The whole chain on raw arrays -> dict with the fields of write_structure (xyz, rgb, labels included)."""
    xyz, rgb = np.asarray(xyz, dtype=F32), np.asarray(rgb, dtype=np.uint8)
    rule = 'labels' if dataset == 'vkitti' else ('objects' if voxel_width > 0 else 'given')
    if voxel_width > 0:
        if dataset == 'vkitti':
            xyz, rgb, labels, _ = P.prune(xyz, voxel_width, rgb, labels, np.zeros(1, np.uint8), n_labels, 0)
            ids = labels
        else:
            xyz, rgb, labels, ids = P.prune(xyz, voxel_width, rgb, labels, objects, n_labels, int(np.max(objects)) + 1)
    else:
        ids = labels if dataset == 'vkitti' else objects
    nei = KR.knn(xyz, k_local)[0]
    out = structure(xyz, nei, k_adj, ids, rule, P.geof(xyz, nei.reshape(-1), k_local))
    out.update(xyz=xyz, rgb=rgb, labels=np.asarray(labels))
    return out


def clouds(geof, rgb, ver_value):
    """graph_loader's clouds for ver_value 'geof' / 'geofrgb': rgb as stored (0 ... 255), divided in float32."""
    geof = np.asarray(geof, dtype=F32)
    if ver_value == 'geof':
        return geof
    return np.concatenate([geof, np.asarray(rgb, dtype=F32) / F32(255)], axis=1)
