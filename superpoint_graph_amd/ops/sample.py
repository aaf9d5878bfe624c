"""Neighbourhood sub-sampling of a resident superpoint graph for the supervised loader (csrc/spg_sample.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib
from ._core import _ptr, _raise_flagged, _workspace, upload, upload_packed
from .edges import EdgeGraph


# --------------------------------------------------------------------------------------------------
# neighbourhood sub-sampling of the supervised loader (csrc/spg_sample.hip; reference learning/spg.py:115-144)
# --------------------------------------------------------------------------------------------------
def _resident(a, dtype, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    t = t.to(dtype).contiguous()
    return t if t.is_cuda else upload(t, dev)


class ResidentSPG:
    """A scene's superpoint graph in device memory: edges i64 [E, 2] in file order with their EdgeGraph, the edge features f32
    [E, F] (or None) and the vertices' point counts i64 [n] (or None; needed for a cut).  Host arrays are uploaded here.  The
    EdgeGraph's range check synchronises once, after every upload: the object is complete on every stream when this returns."""

    def __init__(self, edges, feats, sizes, n: int):
        dev = torch.device('cuda', torch.cuda.current_device())
        self.n = int(n)
        self.edges = _resident(edges, torch.int64, dev).reshape(-1, 2)
        self.E = int(self.edges.shape[0])
        self.feats = None if feats is None else _resident(feats, torch.float32, dev).reshape(self.E, -1)
        self.sizes = None if sizes is None else _resident(sizes, torch.int64, dev).reshape(-1)
        if self.sizes is not None and self.sizes.numel() != self.n:
            raise ValueError(f'ResidentSPG: {self.sizes.numel()} sizes for {self.n} vertices')
        self.graph = EdgeGraph(self.edges[:, 0].contiguous(), self.edges[:, 1].contiguous(), self.n)
        self.device = self.graph.device


class SPGSample:
    """What sample_spg returns: host `vids` i64 [n] (original ids of the kept vertices; their position is their new id) and `degs`
    i64 [n] (in-degrees), the counts `n`, `E`, and on the device `edges` i64 [E, 2] (relabelled), `feats` f32 [E, F] or None, `kept`
    i64 [E] (ids of the kept edges)."""
    __slots__ = ('vids', 'degs', 'n', 'E', 'edges', 'feats', 'kept')


_CENTRE_RANGE, _NO_PERMUTATION = 1, 2      # bits of spg_sample_spg's error word (head[2])
_sample_side = {}      # device index -> (the sampler's stream, its page-locked read-back buffer)


def _sampler(dev, n_words):
    ent = _sample_side.get(dev.index)
    if ent is None or ent[1].numel() < n_words:
        stream = ent[0] if ent is not None else torch.cuda.Stream(device=dev)
        ent = _sample_side[dev.index] = (stream, torch.empty(max(n_words, 4096), dtype=torch.int64).pin_memory())
    return ent


def _index_vector(a, name):
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.int64))
    if t.dim() != 1 or t.dtype.is_floating_point:
        raise ValueError(f'sample_spg: {name} must be an integer vector')
    return t.to(torch.int64).contiguous()


def sample_spg(g: ResidentSPG, perm=None, centres=None, order: int = 0, minpts: int = 0, hardcutoff: int = 0) -> SPGSample:
    """The loader's sub-sampling (permute_vertices -> random_neighborhoods -> k_big_enough) cut out of a resident graph: perm
    (vertex k becomes position perm[k]) or None, centres (ids in the permuted numbering) or None = every vertex is a member,
    else the members are the vertices within `order` steps of a centre, direction ignored; along the permuted positions a member is
    kept while the count of members of >= minpts points is <= hardcutoff (hardcutoff <= 0: all members).  Index-exact with the host
    path; include/spg_hip.h: spg_sample_spg.  perm / centres: host sequences (staged here) or device tensors.
    The launches and the read-back run on the sampler's own stream and ONLY that stream is synchronised (once): the call does not
    wait for work in flight on the current stream.  After it returns the outputs may be used on any stream.
    A centre outside [0, n) raises IndexError, a perm that is no permutation of 0 ... n - 1 ValueError."""
    g.graph._use()
    n, E, dev = g.n, g.E, g.device
    hardcutoff, minpts, order = int(hardcutoff), int(minpts), int(order)
    if order < 0:
        raise ValueError(f'sample_spg: order >= 0 expected, got {order}')
    if hardcutoff > 0 and g.sizes is None:
        raise ValueError('sample_spg: a cut (hardcutoff > 0) needs the sizes of the resident graph')
    perm, centres = _index_vector(perm, 'perm'), _index_vector(centres, 'centres')
    if perm is not None and perm.numel() != n:
        raise ValueError(f'sample_spg: perm has {perm.numel()} entries, the graph {n} vertices')
    L, i64 = lib(), torch.int64
    F = 0 if g.feats is None else int(g.feats.shape[1])
    stream, pinned = _sampler(dev, 3 + 2 * n)
    with torch.cuda.stream(stream):
        staged = upload_packed([t if (t is not None and not t.is_cuda) else None for t in (perm, centres)], dev)
        perm_d, centres_d = (s if s is not None else t for s, t in zip(staged, (perm, centres)))
        back = torch.empty(3 + 2 * n, dtype=i64, device=dev)          # head, vids, degs: one read-back
        head, vids, degs = back[:3], back[3:3 + n], back[3 + n:]
        edges = torch.empty(E, 2, dtype=i64, device=dev)
        kept = torch.empty(E, dtype=i64, device=dev)
        feats = torch.empty(E, F, dtype=torch.float32, device=dev) if g.feats is not None else None
        ws = _workspace(L.spg_sample_spg_workspace_bytes, n, E, dev=dev)
        check(L.spg_sample_spg(_ptr(g.graph.ends), E, n, _ptr(perm_d), _ptr(centres_d), 0 if centres_d is None else int(centres_d.numel()),
                               _ptr(g.sizes), _ptr(g.feats), F, order, minpts, hardcutoff, _ptr(vids), _ptr(edges), _ptr(kept), _ptr(feats),
                               _ptr(degs), _ptr(head), _ptr(ws), ws.numel(), stream.cuda_stream), 'spg_sample_spg')
        host = pinned[:3 + 2 * n]
        host.copy_(back, non_blocking=True)
    stream.synchronize()
    m, Ek, err = (int(v) for v in host[:3].tolist())
    _raise_flagged(err, {_CENTRE_RANGE: (IndexError, f'sample_spg: a centre is outside [0, {n})'),
                         _NO_PERMUTATION: (ValueError, f'sample_spg: perm is not a permutation of 0 ... {n - 1}')})
    out = SPGSample()
    out.n, out.E = m, Ek
    out.vids, out.degs = host[3:3 + m].clone(), host[3 + n:3 + n + m].clone()
    out.edges, out.kept, out.feats = edges[:Ek], kept[:Ek], (feats[:Ek] if feats is not None else None)
    # allocated on the sampler's stream, consumed on the caller's: the allocator must not hand the blocks out again before that use
    cur = torch.cuda.current_stream(dev)
    for t in (edges, kept, feats):
        if t is not None:
            t.record_stream(cur)
    return out
