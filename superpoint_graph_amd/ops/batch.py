"""A training batch on the device: graph construction, edge features, the superpoint loader, cross entropy and the evaluation
counters (csrc/spg_batch.hip, spg_loader.hip, spg_loss.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib
from .._lib import check, lib
from ._core import _ptr, _req, _stream
from .model import DeviceGraph


# --------------------------------------------------------------------------------------------------
# batch construction on the device
# --------------------------------------------------------------------------------------------------
def set_batch(edges, n_nodes: int):
    """edges i64 [E, 2] (source, target; batch node offsets applied) on the device -> (idxn i64 [E], degs i64 [N],
    perm i64 [E]): edges ordered by target (stable), see include/spg_hip.h."""
    _req(edges, torch.int64, 'edges')
    E = int(edges.shape[0])
    dev = edges.device
    idxn = torch.empty(E, dtype=torch.int64, device=dev)
    perm = torch.empty(E, dtype=torch.int64, device=dev)
    degs = torch.empty(n_nodes, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib().spg_set_batch_workspace_bytes(n_nodes, E), dtype=torch.uint8, device=dev)
    check(lib().spg_set_batch(_ptr(edges) if E else None, n_nodes, E, _ptr(idxn) if E else None, _ptr(degs), _ptr(perm) if E else None,
                              _ptr(ws), _ptr(err), _stream()), 'spg_set_batch')
    return idxn, degs, perm, err


def batch_graph_fits(n_nodes: int, n_edges: int, n_feat: int) -> bool:
    """True when the single-launch batch builder serves a batch of this size (include/spg_hip.h: spg_batch_graph_scratch_bytes)."""
    return n_edges > 0 and lib().spg_batch_graph_scratch_bytes(int(n_nodes), int(n_edges), int(n_feat)) > 0


def batch_graph_build(edges_h: torch.Tensor, feats_h: Optional[torch.Tensor], n_nodes: int, device=None):
    """The whole construction of a small batch in one launch (include/spg_hip.h: spg_batch_graph_build / _dev): edges i64 [E, 2]
    (batch node offsets applied) and edge features f32 [E, F], both on the HOST (uploaded here) or both on the DEVICE already -> (idxn, degs, feats_sorted, DeviceGraph, error flag) on the
    device, or None when the batch is too large for the single-workgroup builder (use set_batch + gather_rows + DeviceGraph)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    E = int(edges_h.shape[0])
    F = 0 if feats_h is None else int(feats_h.shape[1])
    L = lib()
    nscratch = L.spg_batch_graph_scratch_bytes(n_nodes, E, F)
    on_dev = edges_h.is_cuda
    if nscratch == 0 or (feats_h is not None and feats_h.is_cuda != on_dev):
        return None
    edges_h = edges_h.contiguous()
    if edges_h.dtype != torch.int64:
        raise TypeError('edges must be int64')
    if feats_h is not None:
        feats_h = feats_h.contiguous()
        if feats_h.dtype != torch.float32 or feats_h.shape[0] != E:
            raise TypeError(f'edge features must be float32 [{E}, F]')
    idxn = torch.empty(E, dtype=torch.int64, device=device)
    degs = torch.empty(n_nodes, dtype=torch.int64, device=device)
    feats = torch.empty(E, F, dtype=torch.float32, device=device) if feats_h is not None else None
    ws = torch.empty(L.spg_graph_workspace_bytes(n_nodes, n_nodes, E), dtype=torch.uint8, device=device)
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=device)
    err = torch.empty(1, dtype=torch.int32, device=device)
    # (inputs already on the device: uploaded with the batch's other small vectors by ONE upload_packed)
    check((L.spg_batch_graph_build_dev if on_dev else L.spg_batch_graph_build)(edges_h.data_ptr() if E else None, feats_h.data_ptr() if (feats_h is not None and E) else None, n_nodes, E, F,
                                  _ptr(idxn) if E else None, _ptr(degs), _ptr(feats) if (feats is not None and E) else None, _ptr(ws),
                                  _ptr(scratch), _ptr(err), _stream()), 'spg_batch_graph_build')
    return idxn, degs, feats, DeviceGraph.from_workspace(ws, idxn, degs), err


def gather_rows(src, perm):
    _req(src, torch.float32, 'src'); _req(perm, torch.int64, 'perm')
    rows, cols = int(perm.numel()), int(src.shape[1])
    dst = torch.empty(rows, cols, dtype=torch.float32, device=src.device)
    check(lib().spg_gather_rows(_ptr(src), cols, _ptr(perm), rows, cols, _ptr(dst), cols, _stream()), 'spg_gather_rows')
    return dst


_EF_KIND = {'': 0, 'copy': 0, 'd': 1, 'ld': 2, 'r': 3, 'const': 4}


def edge_features(columns, edges, mean=None, scale=None):
    """columns: list of (kind, tensor or None, column) per OUTPUT column with kind in copy|d|ld|r|const; the tensor is a
    float32 / float64 device matrix (per edge for copy, per node otherwise).  edges i64 [E, 2]; mean / scale f64 [ncols]."""
    _req(edges, torch.int64, 'edges')
    specs = _lib.EdgeFeatureSpecs()
    if len(columns) > _lib.SPG_EF_MAX_COLS:
        raise ValueError('too many edge feature columns')
    specs.ncols = len(columns)
    keep = []
    for i, (kind, t, col) in enumerate(columns):
        sp = specs.col[i]
        sp.kind = _EF_KIND[kind]
        if t is not None:
            _req(t, name='attribute')
            if t.dtype not in (torch.float32, torch.float64) or t.dim() != 2:
                raise TypeError('attributes must be 2-d float32 / float64 matrices')
            sp.data, sp.ld, sp.column, sp.is_f64 = t.data_ptr(), t.shape[1], int(col), int(t.dtype == torch.float64)
            keep.append(t)
    E = int(edges.shape[0])
    out = torch.empty(E, len(columns), dtype=torch.float32, device=edges.device)
    check(lib().spg_edge_features(ctypes.byref(specs), _ptr(edges) if E else None, E, _ptr(mean), _ptr(scale), _ptr(out), _stream()),
          'spg_edge_features')
    return out


# --------------------------------------------------------------------------------------------------
# superpoint loader
# --------------------------------------------------------------------------------------------------
def load_superpoints(points, offsets, slot, sample_idx, colmap, xyznormalize: bool, n_valid: int, M=None, noise=None):
    """points f32 [Ntot, ncols], offsets i64 [S+1], slot i32 [S], sample_idx i32 [S, npts] (on the device), colmap:
    sequence of raw column indices (host) -> clouds f32 [n_valid, F, npts], diam f32 [n_valid].
    M: f64 [S, 3, 3] or None, noise: f32 [n_valid, npts, F] or None (device)."""
    _req(points, torch.float32, 'points'); _req(offsets, torch.int64, 'offsets'); _req(slot, torch.int32, 'slot')
    _req(sample_idx, torch.int32, 'sample_idx')
    colmap_h = (ctypes.c_int32 * len(colmap))(*[int(c) for c in colmap])
    S, npts, F = slot.numel(), sample_idx.shape[1], len(colmap)
    if offsets.numel() != S + 1 or sample_idx.shape[0] != S:
        raise ValueError('offsets / slot / sample_idx disagree on the number of superpoints')
    if M is not None:
        _req(M, torch.float64, 'M')
    if noise is not None:
        _req(noise, torch.float32, 'noise')
    clouds = torch.empty(n_valid, F, npts, dtype=torch.float32, device=points.device)
    diam = torch.empty(n_valid, dtype=torch.float32, device=points.device)
    if n_valid == 0:      # no superpoint of ptn_minpts points (every slot -1): empty clouds, nothing to launch
        return clouds, diam
    check(lib().spg_load_superpoints(_ptr(points), points.shape[1], _ptr(offsets), S, _ptr(slot), _ptr(sample_idx), npts,
                                     int(bool(xyznormalize)), ctypes.cast(colmap_h, ctypes.c_void_p), F, _ptr(M), _ptr(noise), _ptr(clouds),
                                     _ptr(diam), _stream()), 'spg_load_superpoints')
    return clouds, diam


def loader_random(counts, ids, slot, npts: int, nfeat: int, n_valid: int, seed: int, step: int, augment: bool,
                  scale: float = 0.0, rot: bool = False, mirror_prob: float = 0.0, jitter: bool = False):
    """The loader's random streams generated on the device (Philox4x32-10 keyed by (seed, superpoint id, step)):
    counts / ids i64 [S], slot i32 [S] -> sample_idx i32 [S, npts], M f64 [S, 3, 3] or None, noise f32 [n_valid, npts, nfeat]
    or None -- the inputs of `load_superpoints` (reference learning/spg.py:207-214, 241-257)."""
    _req(counts, torch.int64, 'counts'); _req(ids, torch.int64, 'ids'); _req(slot, torch.int32, 'slot')
    S = slot.numel()
    if counts.numel() != S or ids.numel() != S:
        raise ValueError('counts / ids / slot disagree on the number of superpoints')
    dev = counts.device
    sidx = torch.empty(S, npts, dtype=torch.int32, device=dev)
    M = torch.empty(S, 3, 3, dtype=torch.float64, device=dev) if augment else None
    noise = torch.empty(n_valid, npts, nfeat, dtype=torch.float32, device=dev) if (augment and jitter) else None
    check(lib().spg_loader_random(_ptr(counts), _ptr(ids), _ptr(slot), S, int(npts), int(nfeat), int(seed) & (2 ** 64 - 1),
                                  int(step) & 0xFFFFFFFF, int(bool(augment)), float(scale), int(bool(rot)), float(mirror_prob),
                                  int(bool(jitter)), _ptr(sidx), _ptr(M), _ptr(noise), _stream()), 'spg_loader_random')
    return sidx, M, noise


# --------------------------------------------------------------------------------------------------
# loss
# --------------------------------------------------------------------------------------------------
class _CrossEntropyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, mean):
        logits = _req(logits.contiguous(), torch.float32, 'logits')
        target = _req(target.contiguous(), torch.int64, 'target')
        N, C = logits.shape
        buf = torch.empty(N + 2, dtype=torch.float32, device=logits.device)          # lse [N] | loss | normaliser
        check(lib().spg_cross_entropy_fwd(_ptr(logits), _ptr(target), _ptr(weight), N, C, int(ignore_index), int(mean),
                                          buf[N:].data_ptr(), _ptr(buf), buf[N + 1:].data_ptr(), _stream()), 'spg_cross_entropy_fwd')
        ctx.save_for_backward(logits, target, buf)
        ctx.weight, ctx.ignore_index, ctx.mean = weight, int(ignore_index), int(mean)
        _CrossEntropyFunction.last_normaliser = buf[N + 1:N + 2]      # sum of the class weights of the labelled rows (device)
        return buf[N]

    @staticmethod
    def backward(ctx, grad_loss):
        logits, target, buf = ctx.saved_tensors
        N, C = logits.shape
        g = torch.empty_like(logits)
        grad_loss = grad_loss.contiguous().float()
        check(lib().spg_cross_entropy_bwd(_ptr(logits), _ptr(target), _ptr(ctx.weight), _ptr(buf), buf[N + 1:].data_ptr(), _ptr(grad_loss),
                                          N, C, ctx.ignore_index, ctx.mean, _ptr(g), _stream()), 'spg_cross_entropy_bwd')
        return g, None, None, None, None


def cross_entropy(logits, target, weight=None, ignore_index=-100, reduction='mean', return_normaliser=False):
    """torch.nn.functional.cross_entropy for [N, C] logits and class-index targets (the form learning/main.py:205 uses),
    forward and backward one HIP launch each.  return_normaliser: also the [1] device tensor sum_i weight[target_i] over the
    labelled rows -- the loss weight w_r of a data-parallel rank (superpoint_graph_amd/dist.py), without a host copy."""
    if reduction not in ('mean', 'sum'):
        raise NotImplementedError("reduction must be 'mean' or 'sum'")
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise ValueError('cross_entropy expects logits [N, C] and targets [N]')
    if weight is not None:
        weight = _req(weight.contiguous(), torch.float32, 'weight')
    loss = _CrossEntropyFunction.apply(logits, target, weight, ignore_index, reduction == 'mean')
    if return_normaliser:
        return loss, _CrossEntropyFunction.last_normaliser
    return loss


# --------------------------------------------------------------------------------------------------
# evaluation accounting
# --------------------------------------------------------------------------------------------------
def eval_accumulate(logits, label_mode, label_vec, confusion, counters):
    """logits f32 [N, C] or [S, N, C]; label_mode i64 [N]; label_vec i64 [N, C]; confusion i64 [C, C] and counters i64 [2]
    are accumulated in place.  Returns pred i64 [N]."""
    _req(logits, torch.float32, 'logits'); _req(label_mode, torch.int64, 'label_mode'); _req(label_vec, torch.int64, 'label_vec')
    _req(confusion, torch.int64, 'confusion'); _req(counters, torch.int64, 'counters')
    S = 1 if logits.dim() == 2 else logits.shape[0]
    N, C = logits.shape[-2], logits.shape[-1]
    if label_vec.shape != (N, C) or label_mode.shape != (N,) or confusion.shape != (C, C):
        raise ValueError('shapes: logits [S,]N,C; label_vec N,C; label_mode N; confusion C,C')
    pred = torch.empty(N, dtype=torch.int64, device=logits.device)
    check(lib().spg_eval_accumulate(_ptr(logits), S, N * C, N, C, _ptr(label_mode), _ptr(label_vec), _ptr(pred),
                                    _ptr(confusion), _ptr(counters), _stream()), 'spg_eval_accumulate')
    return pred
