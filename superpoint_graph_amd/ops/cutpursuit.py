"""The integer min cut and the l0 cut-pursuit solver built on it (csrc/spg_cutpursuit.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from .._lib import check, lib
from ._core import _as_vec, _int_vec, _on_gpu, _ptr, _raise_flagged, _raise_nonfinite, _req, _stream, _workspace
from .edges import EdgeGraph, connected_components


# --------------------------------------------------------------------------------------------------
# l0 cut pursuit (csrc/spg_cutpursuit.hip): the min cut and the partition solver that libcp.cutpursuit /
# cutpursuit2 stand for.  UNPINNED against libcp (absent from the reference, unseeded k-means); tests/cutpursuit_restatement.py
# restates both and the device agrees with it exactly.
# --------------------------------------------------------------------------------------------------
MINCUT_LIMIT = 1 << 28
MINCUT_MAX_PULSES = 1 << 16          # (profiles/cutpursuit_bench.txt: the largest count measured is far below 1 / 8 of this)
CP_MAX_D = 32
_MINCUT_RANGE, _MINCUT_UNFINISHED = 1, 2      # bits of spg_mincut's status word (info[0])


def min_cut(graph: EdgeGraph, cap, cost0, cost1, max_pulses: Optional[int] = None, return_info: bool = False):
    """label uint8 [n] minimising sum_v cost_label(v) + sum_e cap_e [label_u != label_v]: cap integer [E], cost0 / cost1 integer [n]
    (the prices of labels 0 and 1), every value in [0, 2^28).  Among the minimisers the one with the fewest ones; self-loops and
    zero capacities are inert, parallel edges add up.  Integer push-relabel in pulses (spg_mincut): the result does not depend on
    scheduling.  ValueError for a value outside the range, RuntimeError when max_pulses pulses do not finish it.
    return_info: also {'pulses', 'launches', 'levels'}."""
    graph._use()
    n, E = graph.n, graph.E
    cap, cost0, cost1 = (_int_vec(t, count, torch.int64, name) for t, count, name in ((cap, E, 'cap'), (cost0, n, 'cost0'), (cost1, n, 'cost1')))
    max_pulses = MINCUT_MAX_PULSES if max_pulses is None else int(max_pulses)
    L, dev = lib(), graph.device
    label = torch.empty(n, dtype=torch.uint8, device=dev)
    info = (ctypes.c_int64 * 4)()
    ws = _workspace(L.spg_mincut_workspace_bytes, n, E, dev=dev)
    check(L.spg_mincut(_ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends), E, n, _ptr(cap), _ptr(cost0), _ptr(cost1), max_pulses,
                       _ptr(label), ctypes.cast(info, ctypes.c_void_p), _ptr(ws), ws.numel(), _stream()), 'spg_mincut')
    _raise_flagged(info[0], {_MINCUT_RANGE: (ValueError, 'min_cut: cap, cost0 and cost1 must lie in [0, 2^28)'),
                             _MINCUT_UNFINISHED: (RuntimeError, f'min_cut: vertices are still active after max_pulses = {max_pulses} pulses')})
    if return_info:
        return label, {'pulses': int(info[1]), 'launches': int(info[2]), 'levels': int(info[3])}
    return label


def _cp_sums(key, mq, q, K):
    """W i64 [K] = sum mq, S i64 [K, D] = sum mq * q over the vertices with key >= 0"""
    n, D = q.shape
    W = torch.empty(K, dtype=torch.int64, device=q.device)
    S = torch.empty(K, D, dtype=torch.int64, device=q.device)
    check(lib().spg_cp_accumulate(_ptr(key), _ptr(mq), _ptr(q), n, D, K, _ptr(W), _ptr(S), _stream()), 'spg_cp_accumulate')
    return W, S


def _cp_dist(q, key, C):
    n, D = q.shape
    out = torch.empty(n, dtype=torch.float64, device=q.device)
    check(lib().spg_cp_dist(_ptr(q), _ptr(key), _ptr(C), n, D, int(C.shape[0]), _ptr(out), _stream()), 'spg_cp_dist')
    return out


def _cp_farthest(dist, key, mq, K):
    """-> (idx i64 [K]: the first positive-weight vertex of every key with the largest dist, n if none; that dist f64 [K])"""
    n = int(dist.numel())
    best = torch.empty(K, dtype=torch.int64, device=dist.device)
    idx = torch.empty(K, dtype=torch.int32, device=dist.device)
    check(lib().spg_cp_farthest(_ptr(dist), _ptr(key), _ptr(mq), n, K, _ptr(best), _ptr(idx), _stream()), 'spg_cp_farthest')
    return idx.long(), best.view(torch.float64)


def _cp_means(W, S):
    has = (W > 0)[:, None]
    return torch.where(has, S.double() / W.double().clamp(min=1.0)[:, None], torch.zeros((), dtype=torch.float64, device=W.device))


def _cp_recentre(C, key, lab, mq, q):
    key2 = torch.where(key >= 0, 2 * key + lab, key)
    W, S = _cp_sums(key2.contiguous(), mq, q, int(C.shape[0]))
    return torch.where((W > 0)[:, None], S.double() / W.double().clamp(min=1.0)[:, None], C).contiguous()


def _cp_exp(x):
    return int(np.frexp(float(x))[1])


def _cp_ldexp(x, k):
    """x * 2^k for a float64 tensor and a host integer k (exact: 2.0 ** k is a float64 for every k that can occur with float32 input)"""
    return x * (2.0 ** int(k))


def _cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam):
    W, S = _cp_sums(comp, mq, q, ncom)
    fid = (mq.double() * _cp_dist(q, comp, _cp_means(W, S).contiguous())).sum()
    cutw = w64[comp[src] != comp[tgt]].sum()
    fid, cutw = torch.stack([fid, cutw]).tolist()
    return float(np.ldexp(fid, -(km + 2 * kf)) + lam * cutw)


def _cp_first_of_groups(sorted_keys):
    first = torch.ones_like(sorted_keys, dtype=torch.bool)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return first


def _cp_renumber(r):
    """ids r i64 [n] -> (i32 [n] numbered 0.. by smallest member, count)"""
    rs, order = torch.sort(r, stable=True)
    first = _cp_first_of_groups(rs)
    roots, member = rs[first], order[first]                       # (stable: the first of a group is its smallest member)
    new = torch.zeros(int(r.max().item()) + 1, dtype=torch.int64, device=r.device)
    new[roots[torch.argsort(member)]] = torch.arange(roots.numel(), device=r.device)
    return new[r].to(torch.int32).contiguous(), int(roots.numel())


def _cp_merge_small(comp, ncom, src, tgt, w, cutoff):
    """the cutoff rounds of cut_pursuit -> (comp i32, ncom, rounds)"""
    dev, E = comp.device, int(w.numel())
    wq = torch.zeros(E, dtype=torch.int64, device=dev)
    wmax = float(w.max().item()) if E else 0.0
    if wmax > 0:
        wq = torch.round(_cp_ldexp(w.double(), 30 - _cp_exp(wmax))).long()
    rounds = 0
    while True:
        c = comp.long()
        size = torch.bincount(c, minlength=ncom)
        a, b = c[src], c[tgt]
        x = a != b
        pa, pb, pw = torch.cat([a[x], b[x]]), torch.cat([b[x], a[x]]), torch.cat([wq[x], wq[x]])
        keep = size[pa] < cutoff
        pa, pb, pw = pa[keep], pb[keep], pw[keep]
        if pa.numel() == 0:
            return comp, ncom, rounds
        pair, inv = torch.unique(pa * ncom + pb, return_inverse=True)
        tot = torch.zeros(pair.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, pw)
        ca, cb = pair // ncom, pair % ncom
        # per small component the neighbour with the largest summed weight, lowest id on ties: pairs are sorted by (ca, cb); a stable
        # sort by descending weight, then a stable sort by ca, leaves the winner first in every group
        o1 = torch.sort(tot, descending=True, stable=True)[1]
        o2 = torch.sort(ca[o1], stable=True)[1]
        order = o1[o2]
        first = _cp_first_of_groups(ca[order])
        ptr = torch.arange(ncom, device=dev)
        ptr[ca[order][first]] = cb[order][first]
        ids = torch.arange(ncom, device=dev)
        mutual = (ptr[ptr] == ids) & (ids < ptr)
        ptr = torch.where(mutual, ids, ptr)
        for _ in range(max(1, int(ncom).bit_length())):
            ptr = ptr[ptr]
        comp, ncom = _cp_renumber(ptr[c])
        rounds += 1


def cut_pursuit(obs, graph: EdgeGraph, edge_weight, node_weight=None, reg_strength=None, cutoff: int = 0, weight_decay: float = 1.0,
                max_ite: int = 5, kmeans_ite: int = 3, flow_steps: int = 2, max_pulses: Optional[int] = None, return_stats: bool = False):
    """l0 cut pursuit: a piecewise-constant x minimising sum_v m_v |x_v - f_v|^2 + reg_strength sum_e w_e [x_u != x_v] greedily by
    binary splits of every component (DESIGN.md section 4.11j states the algorithm; tests/cutpursuit_restatement.py restates it).
    obs f32 [n, D <= 32], edge_weight f32 [E] >= 0, node_weight f32 [n] >= 0 or None (all 1).
    -> (in_component i32 [n] numbered by smallest member, n_com, values f32 [n_com, D] the weighted means, energies: the float64
    energy after every iteration).  Observations and weights are quantised once (20 and 10 bits below the largest), all sums over
    vertices are int64 and the cuts are integer min cuts (min_cut), so the partition does not depend on scheduling.
    return_stats: also {'pulses': per min cut, 'launches', 'merge_rounds'}."""
    graph._use()
    if reg_strength is None:
        raise TypeError('cut_pursuit: reg_strength is required')
    n, E, dev = graph.n, graph.E, graph.device
    obs = _req(obs, torch.float32, 'obs')
    if obs.dim() != 2 or obs.shape[0] != n or obs.shape[1] < 1:
        raise ValueError(f'obs must be [{n}, D] with D >= 1, got {tuple(obs.shape)}')
    D = int(obs.shape[1])
    if D > CP_MAX_D:
        raise ValueError(f'cut_pursuit: D <= {CP_MAX_D} expected, got D = {D}')
    w = _as_vec(_on_gpu(edge_weight, 'edge_weight'), torch.float32, E, 'edge_weight')
    m = torch.ones(n, dtype=torch.float32, device=dev) if node_weight is None else _on_gpu(node_weight, 'node_weight')
    m = _as_vec(m, torch.float32, n, 'node_weight')
    zero = torch.zeros(1, dtype=torch.float32, device=dev)
    finite = torch.isfinite(obs).all() & torch.isfinite(w).all() & torch.isfinite(m).all()
    head = torch.stack([(~finite).float(), obs.abs().max(), m.max(), m.min(), torch.cat([w, zero]).min()]).tolist()
    _raise_nonfinite(int(head[0]))
    if not np.isfinite(float(reg_strength)) or reg_strength < 0:
        raise ValueError(f'cut_pursuit: reg_strength >= 0 and finite expected, got {reg_strength}')
    if head[3] < 0:
        raise ValueError('cut_pursuit: node_weight >= 0 expected')
    if head[4] < 0:
        raise ValueError('cut_pursuit: edge_weight >= 0 expected')
    kf, km = 20 - _cp_exp(head[1]), 10 - _cp_exp(head[2])
    q = torch.round(_cp_ldexp(obs.double(), kf)).to(torch.int32).contiguous()
    mq = torch.round(_cp_ldexp(m.double(), km)).to(torch.int32).contiguous()
    qd, mqd, w64 = q.double(), mq.double(), w.double()
    src, tgt = graph.ends[:, 0].long(), graph.ends[:, 1].long()
    comp, ncom = torch.zeros(n, dtype=torch.int32, device=dev), 1
    sat = torch.zeros(n, dtype=torch.bool, device=dev)
    cut = torch.zeros(E, dtype=torch.bool, device=dev)
    minus1 = torch.full((), -1, dtype=torch.int32, device=dev)
    energies, pulses, launches = [], [], 0
    for t in range(int(max_ite)):
        lam = float(reg_strength) * float(weight_decay) ** t
        K = ncom
        key = torch.where(sat, minus1, comp).contiguous()
        W, S = _cp_sums(key, mq, q, K)
        i0, _ = _cp_farthest(_cp_dist(q, key, _cp_means(W, S).contiguous()), key, mq, K)
        C0 = qd[i0.clamp(max=n - 1)].contiguous()
        i1, far = _cp_farthest(_cp_dist(q, key, C0), key, mq, K)
        C1 = qd[i1.clamp(max=n - 1)]
        done = (W == 0) | (far <= 0)
        sat = sat | done[comp.long()]
        key = torch.where(sat, minus1, comp).contiguous()
        if bool(sat.all().item()):
            energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
            break
        C = torch.stack([C0, C1], 1).reshape(2 * K, D).contiguous()
        k0 = torch.where(key >= 0, 2 * key, minus1).contiguous()
        k1 = torch.where(key >= 0, 2 * key + 1, minus1).contiguous()
        lab = torch.zeros(n, dtype=torch.int32, device=dev)
        for _ in range(int(kmeans_ite)):
            lab = (_cp_dist(q, k1, C) < _cp_dist(q, k0, C)).to(torch.int32)
            C = _cp_recentre(C, key, lab, mq, q)
        for _ in range(int(flow_steps)):
            u = mqd * (_cp_dist(q, k0, C) - _cp_dist(q, k1, C))
            capf = torch.where(cut, torch.zeros((), dtype=torch.float64, device=dev),
                               _cp_ldexp(lam * w64, km + 2 * kf))
            M = float(torch.cat([u.abs(), capf]).max().item())
            p = 27 - _cp_exp(M) if M > 0 else 0
            uq = torch.round(_cp_ldexp(u, p)).long()
            capq = torch.round(_cp_ldexp(capf, p)).long()
            lab8, info = min_cut(graph, capq, uq.clamp(min=0), (-uq).clamp(min=0), max_pulses=max_pulses, return_info=True)
            pulses.append(info['pulses'])
            launches += info['launches']
            lab = lab8.to(torch.int32)
            C = _cp_recentre(C, key, lab, mq, q)
        newcut = ~cut & (lab[src] != lab[tgt])
        c = comp.long()
        ones = torch.zeros(ncom, dtype=torch.int64, device=dev).index_add_(0, c, lab.long())
        size = torch.bincount(c, minlength=ncom)
        sat = sat | ((ones == 0) | (ones == size))[c]
        if not bool(newcut.any().item()):
            energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
            break
        comp, ncom, _ = connected_components(graph, (~(cut | newcut)).to(torch.uint8))
        cut = comp[src] != comp[tgt]
        energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
        if bool(sat.all().item()):
            break
    rounds = 0
    if cutoff > 0:
        comp, ncom, rounds = _cp_merge_small(comp, ncom, src, tgt, w, int(cutoff))
    W, S = _cp_sums(comp, mq, q, ncom)
    c = comp.long()
    P = torch.zeros(ncom, D, dtype=torch.int64, device=dev).index_add_(0, c, q.long())
    size = torch.bincount(c, minlength=ncom)
    num = torch.where((W > 0)[:, None], S, P).double()
    den = torch.where(W > 0, W, size).double()
    values = _cp_ldexp(num / den[:, None], -kf).float()
    if return_stats:
        return comp, ncom, values, energies, {'pulses': pulses, 'launches': launches, 'merge_rounds': rounds}
    return comp, ncom, values, energies
