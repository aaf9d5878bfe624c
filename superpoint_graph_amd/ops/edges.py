"""EdgeGraph, the graph contrastive loss, connected components and the cross-partition weights (csrc/spg_edgeloss.hip)."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._core import _as_vec, _on_gpu, _ptr, _raise_flagged, _req, _stream, _workspace


# --------------------------------------------------------------------------------------------------
# graph contrastive loss of the learned partition (csrc/spg_edgeloss.hip; reference supervized_partition/losses.py)
# --------------------------------------------------------------------------------------------------
EDGE_MAX_D = 64
_DIST_TYPES = {'euclidian': 0, 'intrinsic': 1, 'scalar': 2}
_EDGE_RANGE = 1      # bit of spg_edgegraph_build's error word


def _dist_code(dist_type):
    if dist_type not in _DIST_TYPES:
        raise ValueError(" %s is an unknown argument of parameter --dist_type" % (dist_type))
    return _DIST_TYPES[dist_type]


def _loss_codes(loss):
    """(intra, inter) of a --loss string, by the reference's substring tests in their order (losses.py:46-61)."""
    if 'tv' in loss:
        intra = 0
    elif 'laplacian' in loss:
        intra = 1
    elif 'TVH' in loss:
        intra = 2
    else:
        raise ValueError(" %s is an unknown argument of parameter --loss" % (loss))
    if 'zhang' in loss:
        inter = 0
    elif 'TVminus' in loss:
        inter = 1
    else:
        raise ValueError(" %s is an unknown argument of parameter --loss" % (loss))
    return intra, inter


class EdgeGraph:
    """Edges of one batch on the device with their per-vertex incidence CSR (built once, used by the loss forward, its
    atomic-free backward, connected_components and crosspartition_weights): src / tgt int64 [E] device tensors, n vertices.
    rowptr i32 [n + 1]; inc i32 [2E] = edge << 1 | side (side 0: the vertex is the edge's source), ascending edge id inside a
    vertex; ends i32 [E, 2].  One host synchronisation (the range check of the indices).  build() may be called again with
    other edges; after an IndexError the object holds no graph until a build() succeeds."""

    def __init__(self, src, tgt, n: int):
        self.n, self.E, self.valid = int(n), 0, False
        self.build(src, tgt)

    def build(self, src, tgt):
        src = _req(src, torch.int64, 'src'); tgt = _req(tgt, torch.int64, 'tgt')
        if src.dim() != 1 or src.shape != tgt.shape:
            raise ValueError(f'EdgeGraph: src and tgt must be [E], got {tuple(src.shape)} and {tuple(tgt.shape)}')
        n, E = self.n, int(src.numel())
        if not (1 <= n < 2 ** 31 - 1 and E < 2 ** 30):
            raise ValueError(f'EdgeGraph: 1 <= n < 2^31 - 1 and E < 2^30 expected, got n = {n}, E = {E}')
        L, dev = lib(), src.device
        self.valid = False
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        inc = torch.empty(2 * E, dtype=torch.int32, device=dev)
        ends = torch.empty(E, 2, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _workspace(L.spg_edgegraph_workspace_bytes, n, E, dev=dev)
        check(L.spg_edgegraph_build(_ptr(src), _ptr(tgt), E, n, _ptr(rowptr), _ptr(inc), _ptr(ends), _ptr(err), _ptr(ws), ws.numel(),
                                    _stream()), 'spg_edgegraph_build')
        _raise_flagged(int(err.item()), {_EDGE_RANGE: (IndexError, f'EdgeGraph: an edge index is outside [0, {n})')})
        self.E, self.rowptr, self.inc, self.ends, self.device = E, rowptr, inc, ends, dev
        self.valid = True
        return self

    def _use(self):
        if not self.valid:
            raise RuntimeError('EdgeGraph: the last build() failed; build() it again before use')
        return self


def _edge_forward(mode, emb, graph, dist_code, intra, inter, is_transition, weights, diff):
    """-> (diff, dx, dl, loss f64 [2]) of spg_edge_forward (mode 1: diff; 2: loss from diff, graph = None; 3: both)."""
    L = lib()
    E, dev = (graph.E, graph.device) if graph is not None else (int(diff.numel()), diff.device)
    f32 = torch.float32
    dx = dl = loss = ws = None
    if mode & 1:
        diff = torch.empty(E, dtype=f32, device=dev)
        dx = torch.empty(E, dtype=f32, device=dev) if dist_code == 1 else None
    if mode & 2:
        dl = torch.empty(E, dtype=f32, device=dev)
        loss = torch.empty(2, dtype=torch.float64, device=dev)
        ws = _workspace(L.spg_edge_forward_workspace_bytes, E, dev=dev)
    n, d = (int(emb.shape[0]), int(emb.shape[1])) if emb is not None else (1, 1)
    check(L.spg_edge_forward(mode, _ptr(emb), n, d, _ptr(graph.ends) if graph is not None else None, E, dist_code, intra, inter, _ptr(is_transition), _ptr(weights),
                             _ptr(diff), _ptr(dx), _ptr(dl), _ptr(loss), _ptr(ws), ws.numel() if ws is not None else 0, _stream()),
          'spg_edge_forward')
    return diff, dx, dl, loss


def _edge_backward(emb, graph, dist_code, dl, is_transition, up, gdiff, dx):
    grad = torch.empty_like(emb)
    check(lib().spg_edge_backward(_ptr(emb), int(emb.shape[0]), int(emb.shape[1]), _ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends),
                                  graph.E, dist_code, _ptr(dl), _ptr(is_transition), _ptr(up), _ptr(gdiff), _ptr(dx), _ptr(grad),
                                  _stream()), 'spg_edge_backward')
    return grad


def _emb_arg(emb, graph):
    emb = _req(emb.contiguous(), torch.float32, 'embeddings')
    if emb.dim() != 2 or emb.shape[0] != graph.n:
        raise ValueError(f'embeddings must be [{graph.n}, d], got {tuple(emb.shape)}')
    if not 1 <= emb.shape[1] <= EDGE_MAX_D:
        raise ValueError(f'embeddings: 1 <= d <= {EDGE_MAX_D} expected, got d = {emb.shape[1]}')
    return emb


def _up_pair(g1, g2, dev):
    z = torch.zeros((), dtype=torch.float32, device=dev)
    return torch.stack([z if g1 is None else g1.float().reshape(()), z if g2 is None else g2.float().reshape(())])


class _EdgeDistFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, dist_code):
        emb = _emb_arg(emb, graph)
        diff, dx, _, _ = _edge_forward(1, emb, graph, dist_code, 0, 0, None, None, None)
        ctx.save_for_backward(emb, dx)
        ctx.graph, ctx.dist_code = graph, dist_code
        return diff

    @staticmethod
    def backward(ctx, grad_diff):
        emb, dx = ctx.saved_tensors
        gdiff = _req(grad_diff.contiguous(), torch.float32, 'grad_diff')
        return _edge_backward(emb, ctx.graph._use(), ctx.dist_code, None, None, None, gdiff, dx), None, None


class _EdgeLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, diff, is_transition, weights, intra, inter, dist_code):
        diff = _req(diff.contiguous(), torch.float32, 'diff')
        _, _, dl, loss = _edge_forward(2, None, None, dist_code, intra, inter, is_transition, weights, diff)
        ctx.save_for_backward(dl, is_transition)
        loss = loss.float()
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g1, g2):
        dl, is_transition = ctx.saved_tensors
        gdiff = torch.empty_like(dl)
        up = _up_pair(g1, g2, dl.device)
        check(lib().spg_edge_loss_backward(_ptr(dl), _ptr(is_transition), _ptr(up), dl.numel(), _ptr(gdiff), _stream()),
              'spg_edge_loss_backward')
        return gdiff, None, None, None, None, None


class _ContrastiveEdgeLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, is_transition, weights, intra, inter, dist_code):
        emb = _emb_arg(emb, graph)
        diff, dx, dl, loss = _edge_forward(3, emb, graph, dist_code, intra, inter, is_transition, weights, None)
        ctx.save_for_backward(emb, dx, dl, is_transition)
        ctx.graph, ctx.dist_code = graph, dist_code
        loss = loss.float()
        return loss[0], loss[1], diff

    @staticmethod
    def backward(ctx, g1, g2, grad_diff):
        emb, dx, dl, is_transition = ctx.saved_tensors
        up = _up_pair(g1, g2, emb.device)
        gdiff = None if grad_diff is None else _req(grad_diff.contiguous(), torch.float32, 'grad_diff')
        return (_edge_backward(emb, ctx.graph._use(), ctx.dist_code, dl, is_transition, up, gdiff, dx),
                None, None, None, None, None, None)


def edge_dist(embeddings, graph: EdgeGraph, dist_type='euclidian'):
    """compute_dist (losses.py:31-42): embeddings f32 [n, d <= 64] -> diff f32 [E]; differentiable (atomic-free backward)."""
    code = _dist_code(dist_type)
    return _EdgeDistFunction.apply(embeddings, graph._use(), code)


def edge_loss(diff, is_transition, weights, loss='TVH_zhang', dist_type='euclidian'):
    """compute_loss (losses.py:44-64) from a given diff f32 [E] -> (loss1, loss2), float64 sums in a fixed order returned as
    float32 scalars; differentiable wrt diff."""
    intra, inter = _loss_codes(loss)
    code = _dist_code(dist_type)
    _on_gpu(diff, 'diff')
    if diff.dim() != 1:
        raise ValueError(f'diff must be [E], got {tuple(diff.shape)}')
    E = int(diff.numel())
    return _EdgeLossFunction.apply(diff, _as_vec(is_transition, torch.uint8, E, 'is_transition'),
                                   _as_vec(weights, torch.float32, E, 'weights'), intra, inter, code)


def contrastive_edge_loss(embeddings, graph: EdgeGraph, is_transition, weights, loss='TVH_zhang', dist_type='euclidian'):
    """compute_dist + compute_loss in one launch over the edges -> (loss1, loss2, diff), bit-identical to edge_dist followed by
    edge_loss; the backward is one launch over the vertices through the incidence CSR (no atomics, deterministic)."""
    intra, inter = _loss_codes(loss)
    code = _dist_code(dist_type)
    graph._use()
    _on_gpu(embeddings, 'embeddings')
    return _ContrastiveEdgeLossFunction.apply(embeddings, graph, _as_vec(is_transition, torch.uint8, graph.E, 'is_transition'),
                                              _as_vec(weights, torch.float32, graph.E, 'weights'), intra, inter, code)


def connected_components(graph: EdgeGraph, active):
    """Components of the vertices over the edges with active != 0 (libply_c.connected_comp with cutoff 0) ->
    (in_component i32 [n], n_components int, component_size i32 [n_components]), numbered by ascending smallest member."""
    graph._use()
    active = _as_vec(active, torch.uint8, graph.E, 'active')
    L, dev, n = lib(), graph.device, graph.n
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    ncomp = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _workspace(L.spg_cc_workspace_bytes, n, dev=dev)
    check(L.spg_connected_components(_ptr(graph.ends), _ptr(active), graph.E, n, _ptr(comp), _ptr(size), _ptr(ncomp), _ptr(ws),
                                     ws.numel(), _stream()), 'spg_connected_components')
    k = int(ncomp.item())
    return comp, k, size[:k]


def crosspartition_weights(graph: EdgeGraph, pred_in_component, is_transition, factor, return_components=False):
    """compute_weights_XPART (losses.py:130-166): pred_in_component integer [n] (the predicted partition), is_transition [E]
    -> weights f32 [E]: 1 + min(size_a, size_b) / count(pair) * factor on transition edges (float64, rounded once), 1 elsewhere;
    a, b are the components over the edges that neither the truth nor the prediction cuts.
    return_components: also (in_component_x i32 [n], n_components int, component_size i32)."""
    graph._use()
    is_transition = _as_vec(is_transition, torch.uint8, graph.E, 'is_transition')
    _on_gpu(pred_in_component, 'pred_in_component')
    pred = _req(pred_in_component.to(torch.int32).contiguous(), torch.int32, 'pred_in_component')
    L, dev, n = lib(), graph.device, graph.n
    if pred.shape != (n,):
        raise ValueError(f'pred_in_component must be [{n}], got {tuple(pred.shape)}')
    w = torch.empty(graph.E, dtype=torch.float32, device=dev)
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    ncomp = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _workspace(L.spg_xpart_workspace_bytes, n, graph.E, dev=dev)
    check(L.spg_xpart_weights(_ptr(graph.ends), graph.E, n, _ptr(pred), _ptr(is_transition), float(factor), _ptr(w), _ptr(comp),
                              _ptr(size), _ptr(ncomp), _ptr(ws), ws.numel(), _stream()), 'spg_xpart_weights')
    if return_components:
        k = int(ncomp.item())
        return w, comp, k, size[:k]
    return w
