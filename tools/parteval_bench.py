"""Evaluation of a predicted partition on the device (csrc/spg_parteval.hip) timed with hipEvents: ops.partition_scores and
ops.seal_weights (with the PartitionIndex it needs) at the training batch (5e4 vertices, 2.5e5 edges) and at a whole cloud (1e7
vertices, 5e7 edges); next to them the same expressions as torch ops on the same device (what a user would run without these
kernels), and -- training size only -- the reference-style host functions (a Python loop over the components, numpy masks over
the edges).  Medians; kernel launches are counted with torch.profiler.
    python tools/parteval_bench.py [--no-large] [--no-host]      (GPU only)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superpoint_graph_amd import ops
from edgeloss_bench import launches, timed

C, TOL, FACTOR = 8, 2, 5.0


def make(n, k, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    src = torch.arange(n, device='cuda').repeat_interleave(k)
    tgt = (src + torch.randint(1, 200, (n * k,), device='cuda', generator=g)) % n
    cell = 2000
    obj = (torch.arange(n, device='cuda') // cell).to(torch.int32)
    pred = ((torch.arange(n, device='cuda') + cell // 3) // (3 * cell)).to(torch.int32)
    trans = (obj[src] != obj[tgt]).to(torch.uint8)
    labels = torch.zeros(n, C + 1, dtype=torch.int32, device='cuda')
    labels[torch.arange(n, device='cuda'), (1 + obj % C).long()] = torch.randint(1, 7, (n,), device='cuda', generator=g, dtype=torch.int32)
    return src, tgt, obj, pred, int(pred.max().item()) + 1, trans, labels


def torch_relax(b, src, tgt, n, tol):
    r = b.clone()
    marks = torch.zeros(n, dtype=torch.bool, device=b.device)
    for _ in range(tol):
        on = r != 0
        marks[src[on]] = True
        marks[tgt[on]] = True
        ms = marks[src]
        r[1] |= ms.any()
        r[0] |= ~ms.all()
        r |= marks[tgt]
    return r


def torch_counts(a, b):
    return torch.bincount(a.long() * 2 + b.long(), minlength=4).reshape(2, 2)


def torch_scores(src, tgt, n, pred, n_com, trans, labels):
    p = pred.long()
    sums = torch.zeros(n_com, C, dtype=torch.int64, device=pred.device).index_add_(0, p, labels[:, 1:].long())
    label_com = sums.argmax(1)
    confusion = torch.zeros(C, C, dtype=torch.int64, device=pred.device).index_add_(0, label_com, sums).t()
    pt = p[src] != p[tgt]
    t = trans != 0
    return confusion, label_com[p], torch_counts(t, torch_relax(pt, src, tgt, n, TOL)), torch_counts(torch_relax(t, src, tgt, n, TOL), pt)


def torch_seal(src, tgt, pred, n_com, obj, trans):
    p = pred.long()
    keys, counts = torch.unique((p << 32) | obj.long(), return_counts=True)
    freq = torch.zeros(n_com, dtype=torch.int64, device=pred.device).scatter_reduce_(0, keys >> 32, counts, 'amax')
    wpc = torch.bincount(p, minlength=n_com) - freq
    w = 1.0 + torch.maximum(wpc[p[src]], wpc[p[tgt]]).double() * FACTOR
    return torch.where(trans != 0, w, 1.0).float()


def host_reference_style(src, tgt, n, pred, n_com, obj, trans, labels):
    """the reference's procedures on the host: a loop over the components, numpy masks over all the edges"""
    comps = [np.flatnonzero(pred == c) for c in range(n_com)]
    t0 = time.perf_counter()
    full = np.zeros(n, np.uint32)
    for c in comps:
        full[c] = labels[c, 1:].sum(0).argmax()
    cm = np.zeros((C, C))
    for i in range(n):
        cm[:, full[i]] += labels[i, 1:]

    def relax(b):
        r, tv = b.copy(), np.zeros(n, np.uint8)
        for _ in range(TOL):
            tv[src[r.nonzero()]] = True
            tv[tgt[r.nonzero()]] = True
            r[tv[src]] = True
            r[tv[tgt] > 0] = True
        return r
    pt = pred[src] != pred[tgt]
    rp, rt = relax(pt), relax(trans)
    br = 100 * ((trans == rp) * trans).sum() / trans.sum()
    bp = 100 * ((rt == pt) * pt).sum() / pt.sum()
    t_scores = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    wpc = np.empty(n_com, np.uint32)
    for i, c in enumerate(comps):
        wpc[i] = len(c) - np.unique(obj[c], return_counts=True)[1].max()
    w = np.ones(len(src), np.float32)
    nz = trans.nonzero()
    w[nz] += np.stack((wpc[pred[src[nz]]], wpc[pred[tgt[nz]]])).max(0) * FACTOR
    t_seal = (time.perf_counter() - t0) * 1e3
    return t_scores, t_seal, cm.astype(np.int64), br, bp, w


def main():
    sizes = [(50_000, 5, 20)] + ([] if '--no-large' in sys.argv else [(10_000_000, 5, 3)])
    for n, k, reps in sizes:
        src, tgt, obj, pred, n_com, trans, labels = make(n, k)
        E = n * k
        graph = ops.EdgeGraph(src, tgt, n)
        hip_scores = lambda: ops.partition_scores(graph, pred, n_com, trans, labels, TOL)
        hip_seal = lambda: ops.seal_weights(graph, ops.PartitionIndex(pred, n_com), obj, trans, FACTOR)
        tor_scores = lambda: torch_scores(src, tgt, n, pred, n_com, trans, labels)
        tor_seal = lambda: torch_seal(src, tgt, pred, n_com, obj, trans)
        s, r = hip_scores(), tor_scores()
        same = bool(torch.equal(s['confusion'], r[0]) and torch.equal(s['full_pred'].long(), r[1]) and torch.equal(s['br_counts'], r[2])
                    and torch.equal(s['bp_counts'], r[3]))
        same_w = bool(torch.equal(hip_seal().view(torch.int32), tor_seal().view(torch.int32)))
        print(f'n = {n}, E = {E}, {n_com} predicted components, C = {C}, tolerance {TOL} ({int(trans.sum())} transition edges):', flush=True)
        print(f'  partition_scores HIP         {timed(hip_scores, reps):9.3f} ms  ({launches(hip_scores)} kernels, one host sync)')
        print(f'  partition_scores torch       {timed(tor_scores, reps):9.3f} ms  ({launches(tor_scores)} kernels); equal outputs: {same}')
        print(f'  index + seal_weights HIP     {timed(hip_seal, reps):9.3f} ms  ({launches(hip_seal)} kernels, two host syncs)')
        print(f'  seal_weights torch           {timed(tor_seal, reps):9.3f} ms  ({launches(tor_seal)} kernels); bit-equal weights: {same_w}', flush=True)
        if n <= 100_000 and '--no-host' not in sys.argv:
            h = [a.cpu().numpy() for a in (src, tgt, pred, obj, trans, labels)]
            t_scores, t_seal, cm, br, bp, w = host_reference_style(h[0], h[1], n, h[2], n_com, h[3], h[4], h[5])
            c = s['br_counts'].cpu().numpy()
            ok = np.array_equal(cm, s['confusion'].cpu().numpy()) and br == 100 * c[1, 1] / (c[1, 0] + c[1, 1])
            ok_w = np.array_equal(w.view(np.uint32), hip_seal().cpu().numpy().view(np.uint32))
            print(f'  evaluate() body, host        {t_scores:9.3f} ms  (loops over components and vertices, masks over the edges); equal to the device: {ok}')
            print(f'  compute_weights_SEAL, host   {t_seal:9.3f} ms  (np.unique per component); bit-equal to the device: {ok_w}', flush=True)
        del graph
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
