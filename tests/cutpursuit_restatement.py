"""The l0 cut pursuit of DESIGN.md section 4.11j, restated in numpy: the synchronous push-relabel min cut of ops.min_cut (same
pulses, same global-relabel cadence, so the pulse counts are the device's) and the partition solver of ops.cut_pursuit.  Every
decision that can change a label is integer arithmetic or a float64 operation rounded on its own, so the device must agree
exactly.  UNPINNED against libcp (the reference's copy is an empty submodule and its k-means start is unseeded); the min cut has
an outside judge, scipy's maximum_flow (test_cutpursuit_restatement.py)."""
import math

import numpy as np

RELABEL_EVERY = 16        # pulses between two global relabels (MC_RELABEL_EVERY of csrc/spg_cutpursuit.hip)
CAP_LIMIT = 1 << 28


# ------------------------------------------------------------------------------------------------------------------
# min cut
# ------------------------------------------------------------------------------------------------------------------
def _arcs(src, tgt, cap):
    """arc 2e = src -> tgt, arc 2e + 1 = tgt -> src (the inc entries of ops.EdgeGraph); self-loops carry nothing"""
    E = len(src)
    tail = np.empty(2 * E, np.int64)
    tail[0::2], tail[1::2] = src, tgt
    head = tail[np.arange(2 * E) ^ 1]
    res = np.repeat(np.asarray(cap, np.int64), 2)
    res[tail == head] = 0
    return tail, head, res


def _global_relabel(n, tail, head, res, rsink):
    """exact distance to the sink in the residual graph (sink = 0); n + 2 = the sink cannot be reached"""
    INF = n + 2
    h = np.where(rsink > 0, 1, INF).astype(np.int64)
    k = 1
    while True:
        hit = (res > 0) & (h[tail] == INF) & (h[head] == k)
        if not hit.any():
            return h
        h[tail[hit]] = k + 1
        k += 1


def min_cut(n, src, tgt, cap, cost0, cost1, max_pulses=None, relabel_every=RELABEL_EVERY):
    """-> (label uint8 [n], pulses).  label 1 = the vertices that reach the sink in the residual graph of a maximum preflow:
    the minimiser of sum cost_label + sum cap [label_u != label_v] with the fewest ones."""
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    cap, cost0, cost1 = (np.asarray(a, np.int64) for a in (cap, cost0, cost1))
    for name, a in (('cap', cap), ('cost0', cost0), ('cost1', cost1)):
        if a.size and (a.min() < 0 or a.max() >= CAP_LIMIT):
            raise ValueError(f'{name} must lie in [0, 2^28)')
    tail, head, res = _arcs(src, tgt, cap)
    A, INF = len(tail), n + 2
    excess, rsink = cost1.copy(), cost0.copy()
    h = _global_relabel(n, tail, head, res, rsink)
    pulses = 0
    while True:
        active = (excess > 0) & (h < INF)
        if not active.any():
            break
        if max_pulses is not None and pulses >= max_pulses:
            raise RuntimeError(f'min_cut: still active after max_pulses = {max_pulses} pulses')
        # push: to the sink if it can, else along the first admissible incident arc
        tosink = active & (rsink > 0)
        amt = np.minimum(excess, rsink)[tosink]
        excess[tosink] -= amt
        rsink[tosink] -= amt
        cand = active & ~tosink
        adm = cand[tail] & (res > 0) & (h[tail] == h[head] + 1)
        first = np.full(n, A, np.int64)
        np.minimum.at(first, tail[adm], np.nonzero(adm)[0])
        pv = np.nonzero(first < A)[0]
        pa = first[pv]
        amount = np.minimum(excess[pv], res[pa])
        # gather
        res[pa] -= amount
        res[pa ^ 1] += amount
        excess[pv] -= amount
        np.add.at(excess, head[pa], amount)
        # relabel the active vertices that pushed nothing, from the updated residuals and the heights of this pulse
        rl = cand.copy()
        rl[pv] = False
        newh = np.full(n, INF, np.int64)
        ok = rl[tail] & (res > 0)
        np.minimum.at(newh, tail[ok], h[head[ok]] + 1)
        h = np.where(rl, np.minimum(newh, INF), h)
        pulses += 1
        if pulses % relabel_every == 0:
            h = _global_relabel(n, tail, head, res, rsink)
    h = _global_relabel(n, tail, head, res, rsink)
    return (h < INF).astype(np.uint8), pulses


def cut_value(label, src, tgt, cap, cost0, cost1):
    label = np.asarray(label, np.int64)
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    unary = np.where(label == 1, np.asarray(cost1, np.int64), np.asarray(cost0, np.int64)).sum()
    return int(unary + (np.asarray(cap, np.int64) * (label[src] != label[tgt])).sum())


# ------------------------------------------------------------------------------------------------------------------
# the partition solver
# ------------------------------------------------------------------------------------------------------------------
def _exp_of(x):
    return math.frexp(float(x))[1]


def quantise(obs, node_weight):
    obs = np.asarray(obs, np.float32)
    n = obs.shape[0]
    kf = 20 - _exp_of(np.abs(obs).max() if obs.size else 0.0)
    q = np.rint(np.ldexp(obs.astype(np.float64), kf)).astype(np.int64)
    m = np.ones(n, np.float32) if node_weight is None else np.asarray(node_weight, np.float32)
    km = 10 - _exp_of(m.max() if n else 0.0)
    mq = np.rint(np.ldexp(m.astype(np.float64), km)).astype(np.int64)
    return q, kf, mq, km


def _sums(key, mq, q, K):
    W, S = np.zeros(K, np.int64), np.zeros((K, q.shape[1]), np.int64)
    m = key >= 0
    np.add.at(W, key[m], mq[m])
    np.add.at(S, key[m], mq[m, None] * q[m])
    return W, S


def _dist(q, key, C):
    """squared distance of every vertex to row key of C, float64, dimension by dimension, each product and sum rounded on its
    own; 0 where key < 0"""
    acc = np.zeros(q.shape[0], np.float64)
    k = np.maximum(key, 0)
    for d in range(q.shape[1]):
        diff = q[:, d].astype(np.float64) - C[k, d]
        acc = acc + diff * diff
    acc[key < 0] = 0.0
    return acc


def _farthest(dist, key, ok, K, n):
    """per row of key: the largest dist among ok and the first vertex that has it (n: no vertex)"""
    best = np.full(K, -1.0)
    np.maximum.at(best, key[ok], dist[ok])
    hit = ok & (dist == best[np.maximum(key, 0)])
    idx = np.full(K, n, np.int64)
    np.minimum.at(idx, key[hit], np.nonzero(hit)[0])
    return idx, best


def _recentre(C, key, lab, mq, q):
    key2 = np.where(key >= 0, 2 * key + lab, -1)
    W, S = _sums(key2, mq, q, C.shape[0])
    has = W > 0
    C = C.copy()
    C[has] = S[has].astype(np.float64) / W[has].astype(np.float64)[:, None]
    return C


def components(n, src, tgt, active):
    """components over the active edges, numbered by smallest member"""
    s, t = src[active], tgt[active]
    lab = np.arange(n)
    while True:
        new = lab.copy()
        np.minimum.at(new, s, lab[t])
        np.minimum.at(new, t, lab[s])
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    uniq, inv = np.unique(lab, return_inverse=True)
    return inv.astype(np.int64), len(uniq)


def energy(q, kf, mq, km, comp, ncom, src, tgt, w, lam):
    """sum m |x - f|^2 + lam sum w [x_u != x_v] of the piecewise-constant weighted-mean solution on comp, float64"""
    W, S = _sums(comp, mq, q, ncom)
    C = np.zeros(S.shape, np.float64)
    has = W > 0
    C[has] = S[has].astype(np.float64) / W[has].astype(np.float64)[:, None]
    fid = np.ldexp((mq.astype(np.float64) * _dist(q, comp, C)).sum(), -(km + 2 * kf))
    return float(fid + lam * w.astype(np.float64)[comp[src] != comp[tgt]].sum())


def _renumber(r, n):
    """ids of r -> 0.. by smallest member"""
    first = np.full(int(r.max()) + 1, n, np.int64)
    np.minimum.at(first, r, np.arange(n))
    roots = np.nonzero(first < n)[0]
    new = np.zeros(len(first), np.int64)
    new[roots[np.argsort(first[roots], kind='stable')]] = np.arange(len(roots))
    return new[r], len(roots)


def merge_small(comp, ncom, src, tgt, w, cutoff):
    n = len(comp)
    wq = np.zeros(len(w), np.int64)
    if len(w) and w.max() > 0:
        wq = np.rint(np.ldexp(w.astype(np.float64), 30 - _exp_of(w.max()))).astype(np.int64)
    rounds = 0
    while True:
        size = np.bincount(comp, minlength=ncom)
        a, b = comp[src], comp[tgt]
        x = a != b
        pa, pb, pw = np.concatenate([a[x], b[x]]), np.concatenate([b[x], a[x]]), np.concatenate([wq[x], wq[x]])
        keep = size[pa] < cutoff
        pa, pb, pw = pa[keep], pb[keep], pw[keep]
        if len(pa) == 0:
            return comp, ncom, rounds
        pair, inv = np.unique(pa * ncom + pb, return_inverse=True)
        tot = np.zeros(len(pair), np.int64)
        np.add.at(tot, inv, pw)
        ca, cb = pair // ncom, pair % ncom
        best = np.full(ncom, -1, np.int64)
        np.maximum.at(best, ca, tot)
        hit = tot == best[ca]
        ptr = np.arange(ncom)
        to = np.full(ncom, ncom, np.int64)
        np.minimum.at(to, ca[hit], cb[hit])
        has = to < ncom
        ptr[has] = to[has]
        mutual = (ptr[ptr] == np.arange(ncom)) & (np.arange(ncom) < ptr)
        ptr[mutual] = np.arange(ncom)[mutual]
        for _ in range(max(1, int(ncom).bit_length())):
            ptr = ptr[ptr]
        comp, ncom = _renumber(ptr[comp], n)
        rounds += 1


def cut_pursuit(obs, src, tgt, edge_weight, node_weight=None, reg_strength=0.0, cutoff=0, weight_decay=1.0, max_ite=5,
                kmeans_ite=3, flow_steps=2, stats=None, cut_fn=min_cut):
    """-> (in_component int32 [n], n_com, values f32 [n_com, D], energies list of float64).  stats: a dict that receives the
    pulse count of every min cut ('pulses') and the merge rounds.  cut_fn: another solver of the same canonical min cut with
    min_cut's signature (tools/cutpursuit_bench.py times this restatement with scipy's maximum_flow)."""
    obs = np.asarray(obs, np.float32)
    n, D = obs.shape
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    w = np.asarray(edge_weight, np.float32)
    E = len(src)
    q, kf, mq, km = quantise(obs, node_weight)
    w64 = w.astype(np.float64)
    comp, ncom = np.zeros(n, np.int64), 1
    sat = np.zeros(n, bool)
    cut = np.zeros(E, bool)
    energies, pulses = [], []
    for t in range(max_ite):
        lam = reg_strength * weight_decay ** t
        K = ncom
        key = np.where(sat, -1, comp)
        W, S = _sums(key, mq, q, K)
        mean = np.zeros((K, D), np.float64)
        has = W > 0
        mean[has] = S[has].astype(np.float64) / W[has].astype(np.float64)[:, None]
        pos = (mq > 0) & (key >= 0)
        i0, _ = _farthest(_dist(q, key, mean), key, pos, K, n)
        C0 = q[np.minimum(i0, n - 1)].astype(np.float64)
        i1, far = _farthest(_dist(q, key, C0), key, pos, K, n)
        C1 = q[np.minimum(i1, n - 1)].astype(np.float64)
        done = (W == 0) | (far <= 0)
        sat = sat | done[comp]
        key = np.where(sat, -1, comp)
        if (key < 0).all():
            energies.append(energy(q, kf, mq, km, comp, ncom, src, tgt, w, lam))
            break
        C = np.stack([C0, C1], 1).reshape(2 * K, D)
        k0, k1 = np.where(key >= 0, 2 * key, -1), np.where(key >= 0, 2 * key + 1, -1)
        lab = np.zeros(n, np.int64)
        for _ in range(kmeans_ite):
            lab = (_dist(q, k1, C) < _dist(q, k0, C)).astype(np.int64)
            C = _recentre(C, key, lab, mq, q)
        for _ in range(flow_steps):
            u = mq.astype(np.float64) * (_dist(q, k0, C) - _dist(q, k1, C))
            capf = np.where(cut, 0.0, np.ldexp(lam * w64, km + 2 * kf))
            M = max(np.abs(u).max(), capf.max() if E else 0.0)
            p = 27 - _exp_of(M) if M > 0 else 0
            uq = np.rint(np.ldexp(u, p)).astype(np.int64)
            capq = np.rint(np.ldexp(capf, p)).astype(np.int64)
            lab8, np_ = cut_fn(n, src, tgt, capq, np.maximum(uq, 0), np.maximum(-uq, 0))
            pulses.append(np_)
            lab = lab8.astype(np.int64)
            C = _recentre(C, key, lab, mq, q)
        newcut = ~cut & (lab[src] != lab[tgt])
        ones, size = np.zeros(ncom, np.int64), np.bincount(comp, minlength=ncom)
        np.add.at(ones, comp, lab)
        const = (ones == 0) | (ones == size)
        sat = sat | const[comp]
        if not newcut.any():
            energies.append(energy(q, kf, mq, km, comp, ncom, src, tgt, w, lam))
            break
        comp, ncom = components(n, src, tgt, ~(cut | newcut))
        cut = comp[src] != comp[tgt]
        energies.append(energy(q, kf, mq, km, comp, ncom, src, tgt, w, lam))
        if sat.all():
            break
    rounds = 0
    if cutoff > 0:
        comp, ncom, rounds = merge_small(comp, ncom, src, tgt, w, cutoff)
    W, S = _sums(comp, mq, q, ncom)
    size = np.bincount(comp, minlength=ncom)
    P = np.zeros((ncom, D), np.int64)
    np.add.at(P, comp, q)
    num = np.where((W > 0)[:, None], S, P).astype(np.float64)
    den = np.where(W > 0, W, size).astype(np.float64)
    values = np.ldexp(num / den[:, None], -kf).astype(np.float32)
    if stats is not None:
        stats['pulses'], stats['merge_rounds'] = pulses, rounds
    return comp.astype(np.int32), ncom, values, energies
