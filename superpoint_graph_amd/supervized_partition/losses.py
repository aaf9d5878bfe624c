"""`zhang` / `compute_dist` / `compute_loss` / `compute_weights_XPART` / `compute_weights_SEAL` / `mode` / `relax_edge_binary` /
`compute_weight_loss` with the reference's signatures (supervized_partition/losses.py:24-186), computed by the HIP library
(csrc/spg_edgeloss.hip and csrc/spg_parteval.hip through ops.EdgeGraph, ops.edge_dist, ops.edge_loss,
ops.crosspartition_weights, ops.seal_weights, ops.component_mode, ops.relax_edges).  Everything between the embeddings and
`loss.backward()` runs on the device: the distance and loss are one launch over the edges each, their backward is one launch
over the vertices without atomics (deterministic), the cross-partition weights are a device connected-components pass and a
sort, the SEAL weights a sort of (component, object) pairs and one launch over the edges.

The predicted partition (losses.py:67-89 compute_partition) comes from the device cut pursuit of partition/libcp.py
(ops.cut_pursuit, UNPINNED against libcp: DESIGN.md section 4.11j): `compute_weight_loss(..., partition='device')` computes it,
`partition=(pred_components, pred_in_component)` takes what the caller's own cut pursuit returned, and without either the
functions that need a partition refuse as before.
`relax_edge_binary` reproduces what the reference's function computes, including what its integer indexing does (see
ops.relax_edges).  No CPU path."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..ops import EdgeGraph
from ..ops.edges import _loss_codes

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
    _loss_codes(args.loss)
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


def _vertex_tensor(a, dev):
    """A per-vertex integer array (numpy or tensor) as an int32 device tensor."""
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch.int32)
    return ops.upload(torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)), dev)


def compute_weights_SEAL(pred_components, pred_in_component, objects, edg_source, edg_target, is_transition, transition_factor):
    """losses.py:119-128 -> float32 numpy [E], as the reference returns it: 1 + max over both ends of (size of the predicted
    component - frequency of its most frequent object) * transition_factor on transition edges (float64, rounded once), 1
    elsewhere.  Of pred_components only its length enters (the membership is pred_in_component)."""
    n = len(pred_in_component)
    g = _graph(edg_source, edg_target, n)
    dev = g.device
    index = ops.PartitionIndex(_vertex_tensor(pred_in_component, dev), len(pred_components))
    tr = is_transition if torch.is_tensor(is_transition) else torch.from_numpy(np.ascontiguousarray(is_transition))
    w = ops.seal_weights(g, index, _vertex_tensor(objects, dev), (tr != 0).to(device=dev, dtype=torch.uint8), transition_factor)
    return w.cpu().numpy()


def mode(array, only_frequency=False):
    """losses.py:168-173: the most frequent value of a non-negative integer array (the smallest among equals) and its
    frequency; only_frequency: the frequency alone."""
    a = array.detach().cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    a = a.reshape(-1)
    if a.size == 0:
        raise ValueError('mode: empty array')
    if not np.issubdtype(a.dtype, np.integer) and a.dtype != np.bool_:
        raise TypeError('mode: an integer array is expected')
    if int(a.max()) > 2 ** 31 - 1:
        raise ValueError('mode: values up to 2^31 - 1')
    dev = _dev()
    index = ops.PartitionIndex(torch.zeros(a.size, dtype=torch.int32, device=dev), 1)
    freq, value = ops.component_mode(index, _vertex_tensor(a, dev))
    freq = np.int64(freq.item())
    if only_frequency:
        return freq
    return a.dtype.type(value.item()), freq


def relax_edge_binary(edg_binary, edg_source, edg_target, n_ver, tolerance):
    """losses.py:175-186 -> numpy [E] of the input's dtype (bool or uint8): what the reference's function computes, which is
    not the symmetric relaxation its text describes (ops.relax_edges, mode 'reference': edges 0 and 1 are set through integer
    indexing, the relaxation spreads through target vertices only).  E < 2 with tolerance > 0 raises ValueError."""
    b = edg_binary.detach().cpu().numpy() if torch.is_tensor(edg_binary) else np.asarray(edg_binary)
    if b.dtype not in (np.bool_, np.uint8):
        raise TypeError(f'relax_edge_binary: a bool or uint8 indicator is expected, got {b.dtype}')
    g = _graph(edg_source, edg_target, int(n_ver))
    out = ops.relax_edges(g, ops.upload(torch.from_numpy(np.ascontiguousarray(b)), g.device), int(tolerance), 'reference')
    return out.cpu().numpy()


def compute_partition(args, embeddings, edg_source, edg_target, diff, xyz=0, device=False):
    """losses.py:67-89 -> (pred_components, pred_in_component) of libcp.cutpursuit on the embeddings (and spatial_emb * xyz when
    args.spatial_emb > 0) with the reference's edge weights, regularisation reg_strength / (4 k_nn_adj), cutoff CP_cutoff and
    decay 0.7.  numpy as the reference returns it; device=True: device tensors.  edg_source may be an EdgeGraph."""
    from ..partition import libcp
    _require_gpu(embeddings, 'embeddings'); _require_gpu(diff, 'diff')
    dev = embeddings.device
    E = int(diff.shape[0])
    edge_weight = torch.ones(E, dtype=torch.float32, device=dev)
    if args.edge_weight_threshold > 0:
        edge_weight[diff.detach() > 1] = args.edge_weight_threshold
    if args.edge_weight_threshold < 0:
        # (a float32 division by a tensor: dividing by a host scalar multiplies by its reciprocal)
        edge_weight = torch.exp(diff.detach().float() * args.edge_weight_threshold) / \
            torch.tensor(np.exp(args.edge_weight_threshold), dtype=torch.float32, device=dev)
    ver_value = embeddings.detach().float()
    if args.spatial_emb > 0:
        pos = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(xyz))
        ver_value = torch.cat([ver_value, args.spatial_emb * pos.to(device=dev, dtype=torch.float32)], 1)
    g = _graph(edg_source, edg_target, int(embeddings.shape[0]))
    return libcp.cutpursuit(ver_value.contiguous(), g, None, edge_weight, args.reg_strength / (4 * args.k_nn_adj), cutoff=args.CP_cutoff,
                            spatial=int(args.spatial_emb > 0), weight_decay=0.7, device=device)


def compute_weight_loss(args, embeddings, objects, edg_source, edg_target, is_transition, diff, return_partition, xyz=0, partition=None):
    """losses.py:91-117.  partition = (pred_components, pred_in_component) of the caller's cut pursuit, or 'device': compute_partition
    on the device (a partition is needed by loss_weight 'crosspartition' and 'seal' and by return_partition; 'seal' without it raises
    NotImplementedError).  -> weights float32 [E] on the device [, pred_components, pred_in_component]."""
    if args.loss_weight == 'seal' and partition is None:
        raise NotImplementedError(_NO_LIBCP % "loss_weight 'seal'")
    if args.loss_weight not in ('none', 'proportional', 'crosspartition', 'seal'):
        raise ValueError(" %s is an unknown argument of parameter --loss" % (args.loss_weight))
    if (args.loss_weight == 'crosspartition' or return_partition) and partition is None:
        raise ValueError(_NO_LIBCP % ("loss_weight 'crosspartition'" if args.loss_weight == 'crosspartition' else 'return_partition'))
    _require_gpu(embeddings, 'embeddings'); _require_gpu(is_transition, 'is_transition')
    dev = embeddings.device
    E = int(is_transition.shape[0])
    if isinstance(partition, str):
        if partition != 'device':
            raise ValueError(f"partition must be (pred_components, pred_in_component) or 'device', got {partition!r}")
        needed = args.loss_weight in ('seal', 'crosspartition') or return_partition
        partition = compute_partition(args, embeddings, edg_source, edg_target, diff, xyz, device=True) if needed else None
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
    elif args.loss_weight == 'seal':
        # :103: the SEAL weights of the given partition, with the plain transition factor
        g = _graph(edg_source, edg_target, int(embeddings.shape[0]))
        index = ops.PartitionIndex(_vertex_tensor(partition[1], dev), len(partition[0]))
        weights_loss = ops.seal_weights(g, index, _vertex_tensor(objects, dev), (is_transition != 0).to(torch.uint8), args.transition_factor)
    else:
        pred_in_component = partition[1]
        g = _graph(edg_source, edg_target, int(embeddings.shape[0]))
        pred = pred_in_component if torch.is_tensor(pred_in_component) else torch.from_numpy(np.ascontiguousarray(pred_in_component).astype(np.int32))
        weights_loss = ops.crosspartition_weights(g, pred.to(dev), (is_transition != 0).to(torch.uint8),
                                                  args.transition_factor * 2 * args.k_nn_adj)
    if return_partition:
        return weights_loss, partition[0], partition[1]
    return weights_loss
