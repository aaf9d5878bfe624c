"""`zhang` / `compute_dist` / `compute_loss` / `compute_weights_XPART` / `compute_weight_loss` with the reference's signatures
(supervized_partition/losses.py:24-166), computed by the HIP library (csrc/spg_edgeloss.hip through ops.EdgeGraph,
ops.edge_dist, ops.edge_loss, ops.crosspartition_weights).  Everything between the embeddings and `loss.backward()` runs on the
device: the distance and loss are one launch over the edges each, their backward is one launch over the vertices without
atomics (deterministic), the cross-partition weights are a device connected-components pass and a sort.

What is not here: cut pursuit (`libcp`, losses.py:67-89 compute_partition).  The predicted partition is an INPUT:
`compute_weight_loss(..., partition=(pred_components, pred_in_component))` takes what the caller's own cut pursuit returned.
SEAL weights are not implemented.  No CPU path."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..ops import EdgeGraph

_NO_LIBCP = ("%s needs the predicted partition, which the reference gets from cut pursuit (libcp.cutpursuit, losses.py:82); "
             "libcp is not part of this package: run your own cut pursuit and pass partition=(pred_components, pred_in_component)")


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError('superpoint_graph_amd.supervized_partition has no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


_last = None          # (source array, target array, n, EdgeGraph): the pair a training step passes to every call of the step


def _graph(edg_source, edg_target, n):
    """The EdgeGraph of a numpy / tensor index pair; the pair seen last is not rebuilt (the reference's train() hands the same
    two arrays to compute_dist, compute_weight_loss and compute_loss of one step)."""
    global _last
    if isinstance(edg_source, EdgeGraph):
        return edg_source
    if isinstance(edg_target, EdgeGraph):
        return edg_target
    if _last is not None and _last[0] is edg_source and _last[1] is edg_target and _last[2] == n and _last[3].valid \
            and _last[4] == (_fingerprint(edg_source), _fingerprint(edg_target)):
        return _last[3]
    dev = _dev()

    def up(a):
        if torch.is_tensor(a):
            return a.to(device=dev, dtype=torch.int64).contiguous()
        return ops.upload(torch.from_numpy(np.ascontiguousarray(a).astype(np.int64, copy=False)), dev)
    g = EdgeGraph(up(edg_source), up(edg_target), n)         # an IndexError leaves the cache as it was
    _last = (edg_source, edg_target, n, g, (_fingerprint(edg_source), _fingerprint(edg_target)))
    return g


def _fingerprint(a):
    """Guards the identity cache against an array modified in place: its length, first and last entries."""
    m = len(a)
    return (m, int(a[0]), int(a[m // 2]), int(a[-1])) if m else (0,)


def _require_gpu(t, name):
    if torch.is_tensor(t) and not t.is_cuda:
        raise RuntimeError(f'{name} must live on the GPU: superpoint_graph_amd.supervized_partition has no CPU path')


def zhang(x, lam, dist_type):
    """losses.py:24-29 (the expression itself; compute_loss evaluates it inside its kernel)."""
    if dist_type == 'euclidian' or dist_type == 'scalar':
        beta = 1
    elif dist_type == 'intrinsic':
        beta = 1.0471975512
    else:
        raise ValueError(" %s is an unknown argument of parameter --dist_type" % (dist_type))
    _require_gpu(x, 'x')
    return torch.clamp(-lam * x + lam * beta, min=0)


def compute_dist(embeddings, edg_source, edg_target, dist_type):
    """losses.py:31-42 -> diff float32 [E] on the device, differentiable."""
    if dist_type not in ('euclidian', 'intrinsic', 'scalar'):
        raise ValueError(" %s is an unknown argument of parameter --dist_type" % (dist_type))
    _require_gpu(embeddings, 'embeddings')
    return ops.edge_dist(embeddings, _graph(edg_source, edg_target, int(embeddings.shape[0])), dist_type)


def compute_loss(args, diff, is_transition, weights_loss):
    """losses.py:44-64 -> (loss1, loss2), float32 scalars on the device, differentiable wrt diff."""
    ops._loss_codes(args.loss)
    _require_gpu(diff, 'diff')
    return ops.edge_loss(diff, _edge_tensor(is_transition, diff.device), _edge_tensor(weights_loss, diff.device), args.loss,
                         args.dist_type)


def _edge_tensor(a, dev):
    if torch.is_tensor(a):
        _require_gpu(a, 'an edge tensor')
        return a
    return ops.upload(torch.from_numpy(np.ascontiguousarray(a)), dev)


def compute_weights_XPART(pred_components, pred_in_component, objects, edg_source, edg_target, is_transition, transition_factor, xyz):
    """losses.py:130-166 -> float32 numpy [E], as the reference returns it.  pred_components, objects and xyz are unused there
    too (only the membership enters)."""
    n = len(pred_in_component)
    g = _graph(edg_source, edg_target, n)
    dev = g.device
    pred = pred_in_component if torch.is_tensor(pred_in_component) else torch.from_numpy(np.ascontiguousarray(pred_in_component).astype(np.int32))
    tr = is_transition if torch.is_tensor(is_transition) else torch.from_numpy(np.ascontiguousarray(is_transition))
    w = ops.crosspartition_weights(g, pred.to(dev), (tr != 0).to(device=dev, dtype=torch.uint8), transition_factor)
    return w.cpu().numpy()


def compute_weight_loss(args, embeddings, objects, edg_source, edg_target, is_transition, diff, return_partition, xyz=0, partition=None):
    """losses.py:91-117.  partition = (pred_components, pred_in_component) of the caller's cut pursuit (needed by
    loss_weight 'crosspartition' and by return_partition).  -> weights float32 [E] on the device [, pred_components,
    pred_in_component]."""
    if args.loss_weight == 'seal':
        raise NotImplementedError('loss_weight seal (compute_weights_SEAL) is not implemented')
    if args.loss_weight not in ('none', 'proportional', 'crosspartition'):
        raise ValueError(" %s is an unknown argument of parameter --loss" % (args.loss_weight))
    if (args.loss_weight == 'crosspartition' or return_partition) and partition is None:
        raise ValueError(_NO_LIBCP % ("loss_weight 'crosspartition'" if args.loss_weight == 'crosspartition' else 'return_partition'))
    _require_gpu(embeddings, 'embeddings'); _require_gpu(is_transition, 'is_transition')
    dev = embeddings.device
    E = int(is_transition.shape[0])
    if args.loss_weight == 'none':
        weights_loss = torch.ones(E, dtype=torch.float32, device=dev)
    elif args.loss_weight == 'proportional':
        # :99-100: float32(E) / float32(#intra) on the edges inside an object; float64 E / #inter * factor, rounded once, on the others
        trans = is_transition != 0
        n_trans = int(trans.sum().item())
        intra = (torch.tensor(float(E), dtype=torch.float32) / torch.tensor(float(E - n_trans), dtype=torch.float32)).item() if n_trans < E else 1.0
        weights_loss = torch.full((E,), intra, dtype=torch.float32, device=dev)
        if n_trans:
            weights_loss[trans] = float(E) / float(n_trans) * args.transition_factor
    else:
        pred_in_component = partition[1]
        g = _graph(edg_source, edg_target, int(embeddings.shape[0]))
        pred = pred_in_component if torch.is_tensor(pred_in_component) else torch.from_numpy(np.ascontiguousarray(pred_in_component).astype(np.int32))
        weights_loss = ops.crosspartition_weights(g, pred.to(dev), (is_transition != 0).to(torch.uint8),
                                                  args.transition_factor * 2 * args.k_nn_adj)
    if return_partition:
        return weights_loss, partition[0], partition[1]
    return weights_loss
