"""The supervised loader's neighbourhood sub-sampling (reference learning/spg.py:115-144: permute_vertices ->
random_neighborhoods -> k_big_enough) restated in ORIGINAL vertex ids, in numpy, in the project's own words: the form the device
kernels implement (csrc/spg_sample.hip).  It is NOT the judge of the kernels -- that is the host path
itself (spg_sample_cases.host_sample) -- but the bridge between the two: tests/test_spg_sample_cases.py shows, without a GPU,
that this formulation and the host path select the same vertices and edges in the same order."""
import numpy as np


def sample(n, edges, sizes=None, perm=None, centres=None, order=0, minpts=0, hardcutoff=0):
    """edges i64 [E, 2] in file order; perm[k] = position of vertex k, or None; centres = ids in the PERMUTED numbering, or None =
    every vertex is a member -> dict(vids, edges, kept, degs, member): the kept vertices (original ids) in position order, the kept
    edges relabelled, their ids, the in-degrees of the sample, and the member mask per original vertex."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    perm = np.arange(n) if perm is None else np.asarray(perm, dtype=np.int64)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    if centres is None:
        member = np.ones(n, dtype=bool)
    else:
        level = np.full(n, -1, dtype=np.int64)
        level[inv[np.asarray(centres, dtype=np.int64)]] = 0
        for L in range(1, int(order) + 1):
            a, b = edges[:, 0], edges[:, 1]
            new = np.concatenate([b[(level[a] == L - 1) & (level[b] < 0)], a[(level[b] == L - 1) & (level[a] < 0)]])
            if new.size == 0:
                break
            level[new] = L
        member = level >= 0
    mp = member[inv]                                                   # along the permuted positions
    if hardcutoff > 0:
        big = mp & (np.asarray(sizes)[inv] >= minpts)
        kept_pos = mp & (np.cumsum(big) <= hardcutoff)
    else:
        kept_pos = mp
    vids = inv[kept_pos]
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[vids] = np.arange(len(vids))
    ok = (new_id[edges[:, 0]] >= 0) & (new_id[edges[:, 1]] >= 0)
    kept = np.nonzero(ok)[0]
    out_edges = new_id[edges[kept]].reshape(-1, 2)
    degs = np.bincount(out_edges[:, 1], minlength=len(vids)).astype(np.int64)
    return dict(vids=vids, edges=out_edges, kept=kept, degs=degs, member=member)
