"""float64 brute-force restatement of the device kNN order (csrc/spg_knn.hip): key d2 = (dx*dx + dy*dy) + dz*dz in float64 with
dx = float64(q.x) - float64(p.x) (numpy rounds every operation: nothing is fused), ties by point index; in self mode the query
point itself sorts first and is the dropped column.  Distances are float32(sqrt(d2)), as sklearn returns them."""
import numpy as np


def d2_rows(q, p):
    """float64 squared distances [len(q), len(p)] in the contract's operation order."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn(ref, k, query=None, rows=None, chunk=64):
    """(idx int64 [m, k], d2 float64 [m, k]) for the query rows `rows` (default: all); query None = self mode over ref."""
    ref = np.asarray(ref, dtype=np.float32)
    self_mode = query is None
    qset = ref if self_mode else np.asarray(query, dtype=np.float32)
    rows = np.arange(len(qset)) if rows is None else np.asarray(rows)
    idx = np.empty((len(rows), k), dtype=np.int64)
    d2o = np.empty((len(rows), k), dtype=np.float64)
    ar = np.arange(len(ref))
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        d2 = d2_rows(qset[r], ref)
        if self_mode:
            d2[np.arange(len(r)), r] = -1.0                 # the query point sorts first
        kk = k + 1 if self_mode else k
        for j in range(len(r)):
            # everything at or below the kk-th smallest key, then the exact (d2, index) order
            kth = np.partition(d2[j], kk - 1)[kk - 1]
            cand = ar[d2[j] <= kth]
            order = np.lexsort((cand, d2[j][cand]))[:kk]
            sel = cand[order]
            if self_mode:
                sel = sel[1:]
            idx[a + j] = sel
            d2o[a + j] = d2[j][sel]
    return idx, d2o


def dist32(d2):
    return np.sqrt(d2).astype(np.float32)
