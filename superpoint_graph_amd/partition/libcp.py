"""`libcp.cutpursuit` / `libcp.cutpursuit2` with the reference's call signatures (partition/partition.py, supervized_partition/
losses.py:82, learning/../graph_processing), computed on the device by ops.cut_pursuit (csrc/spg_cutpursuit.hip; DESIGN.md section
4.14 states the algorithm).  numpy in, numpy out; device=True takes and returns device tensors where it can.

UNPINNED against libcp: the reference ships it as an empty submodule and its k-means start is unseeded, so there is nothing to
compare bits with.  What is pinned is the numpy restatement of the algorithm (tests/cutpursuit_restatement.py), exactly.

`spatial` is accepted and has no effect: every column of `obs` enters the fidelity, at most 32 of them.  No CPU path."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError('superpoint_graph_amd.partition.libcp has no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


_NP_DTYPE = {torch.float32: np.float32, torch.int64: np.int64}


def _up(a, dtype, dev):
    if torch.is_tensor(a):
        return a.detach().to(device=dev, dtype=dtype).contiguous()
    return ops.upload(torch.from_numpy(np.ascontiguousarray(np.asarray(a)).astype(_NP_DTYPE[dtype], copy=False)), dev)


def _solve(obs, source, target, edge_weight, node_weight, reg_strength, cutoff, weight_decay):
    dev = _dev()
    obs = _up(obs, torch.float32, dev)
    if obs.dim() == 1:
        obs = obs[:, None].contiguous()
    graph = source if isinstance(source, ops.EdgeGraph) else ops.EdgeGraph(_up(source, torch.int64, dev), _up(target, torch.int64, dev),
                                                                          int(obs.shape[0]))
    w = _up(edge_weight, torch.float32, dev).reshape(-1)
    m = None if node_weight is None else _up(node_weight, torch.float32, dev).reshape(-1)
    return ops.cut_pursuit(obs, graph, w, m, reg_strength=float(reg_strength), cutoff=int(cutoff), weight_decay=float(weight_decay))


def _component_lists(in_component, n_com):
    """the vertices of every component, ascending, as one sorted index tensor and the component sizes"""
    order = torch.sort(in_component, stable=True)[1]
    return order, torch.bincount(in_component.long(), minlength=n_com)


def cutpursuit(obs, source, target, edge_weight, reg_strength, cutoff=0, spatial=0, weight_decay=1.0, device=False):
    """-> (components: list of n_com index arrays, in_component uint32 [n]).  obs [n, D <= 32] float32, source / target [E] vertex ids
    (or an ops.EdgeGraph as `source`), edge_weight [E] >= 0.  device=True: components are int64 device tensors and in_component is
    the int32 device tensor."""
    comp, n_com, _, _ = _solve(obs, source, target, edge_weight, None, reg_strength, cutoff, weight_decay)
    order, size = _component_lists(comp, n_com)
    if device:
        return list(torch.split(order, size.tolist())), comp
    bounds = np.cumsum(size.cpu().numpy())[:-1]
    return np.split(order.cpu().numpy(), bounds), comp.cpu().numpy().astype(np.uint32)


def cutpursuit2(obs, source, target, edge_weight, node_weight, reg_strength, cutoff=0, spatial=0, weight_decay=1.0, device=False):
    """-> (solution f32 [n, D]: every vertex's component value, the weighted mean of its observations; in_component uint32 [n]).
    node_weight [n] >= 0: a vertex of weight 0 takes its value from its component (the inpainting of partition labels)."""
    comp, n_com, values, _ = _solve(obs, source, target, edge_weight, node_weight, reg_strength, cutoff, weight_decay)
    solution = values[comp.long()]
    if device:
        return solution, comp
    return solution.cpu().numpy(), comp.cpu().numpy().astype(np.uint32)
