"""Graph contrastive loss on the device (csrc/spg_edgeloss.hip) timed with hipEvents: EdgeGraph build, fused forward + backward
(ops.contrastive_edge_loss) and the cross-partition weights, at the training batch (5e4 vertices, 2.5e5 edges) and at a whole
cloud (1e7 vertices, 5e7 edges); next to it the same expressions as torch ops on the same device (what a user would run without
these kernels), and -- training size only -- the reference-style host loop for the weights (scipy components + one mask per
boundary pair).  Kernel launches are counted with torch.profiler.
    python tools/edgeloss_bench.py [--no-large] [--no-host]      (GPU only)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superpoint_graph_amd import ops


def make(n, k, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    src = torch.arange(n, device='cuda').repeat_interleave(k)
    tgt = (src + torch.randint(1, 200, (n * k,), device='cuda', generator=g)) % n
    emb = torch.nn.functional.normalize(torch.randn(n, 4, device='cuda', generator=g), dim=1)
    cell = 2000
    obj, pred = src.new_tensor(0), None
    obj = (torch.arange(n, device='cuda') // cell)
    pred = ((torch.arange(n, device='cuda') + cell // 3) // (3 * cell)).to(torch.int32)
    trans = (obj[src] != obj[tgt]).to(torch.uint8)
    w = torch.where(trans != 0, 20.0, 1.0).float()
    return src, tgt, emb, trans, w, pred


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        fn(); torch.cuda.synchronize()
    return sum(e.count for e in p.key_averages() if e.device_type.name != 'CPU' and 'Memcpy' not in e.key and 'Memset' not in e.key)


def torch_step(emb, src, tgt, trans, w):
    emb = emb.detach().requires_grad_(True)
    diff = ((emb[src] - emb[tgt]) ** 2).sum(1)
    intra, inter = trans == 0, trans == 1
    l1 = 0.2 * (w[intra] * (torch.sqrt(1 + diff[intra] / 0.2 ** 2) - 1)).sum()
    l2 = torch.clamp(-w[inter] * torch.sqrt(diff[inter] + 1e-10) + w[inter], min=0).sum()
    ((l1 + l2) / src.numel() * 1000).backward()
    return emb.grad


def hip_step(emb, graph, trans, w):
    emb = emb.detach().requires_grad_(True)
    l1, l2, _ = ops.contrastive_edge_loss(emb, graph, trans, w)
    ((l1 + l2) / graph.E * 1000).backward()
    return emb.grad


def host_xpart(n, src, tgt, trans, pred, factor):
    """the reference's procedure (losses.py:130-166) on the host: components, then one mask over the transition edges per pair"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    active = (trans == 0) & (pred[src] == pred[tgt])
    k, comp = connected_components(coo_matrix((np.ones(int(active.sum()), np.int8), (src[active], tgt[active])), shape=(n, n)), directed=False)
    size = np.bincount(comp, minlength=k)
    e = np.flatnonzero(trans)
    a, b = comp[src[e]], comp[tgt[e]]
    key = np.minimum(a, b) * k + np.maximum(a, b)
    _, first, cnt = np.unique(key, return_index=True, return_counts=True)
    w = np.ones(len(src), np.float32)
    for i, c in zip(first, cnt):
        m = ((a == a[i]) & (b == b[i])) | ((b == a[i]) & (a == b[i]))
        w[e[m]] = w[e[m]] + min(size[a[i]], size[b[i]]) / c * factor
    return w


def main():
    sizes = [(50_000, 5, 20)] + ([] if '--no-large' in sys.argv else [(10_000_000, 5, 3)])
    for n, k, reps in sizes:
        src, tgt, emb, trans, w, pred = make(n, k)
        E = n * k
        t_build = timed(lambda: ops.EdgeGraph(src, tgt, n), reps)
        graph = ops.EdgeGraph(src, tgt, n)
        t_hip = timed(lambda: hip_step(emb, graph, trans, w), reps)
        t_torch = timed(lambda: torch_step(emb, src, tgt, trans, w), reps)
        t_xp = timed(lambda: ops.crosspartition_weights(graph, pred, trans, 50.0), reps)
        err = float((hip_step(emb, graph, trans, w) - torch_step(emb, src, tgt, trans, w)).abs().max())
        print(f'n = {n}, E = {E}, d = 4, TVH_zhang / euclidian ({int(trans.sum())} transition edges):', flush=True)
        print(f'  EdgeGraph build              {t_build:9.3f} ms  ({launches(lambda: ops.EdgeGraph(src, tgt, n))} kernels, one host sync)')
        print(f'  HIP forward + backward       {t_hip:9.3f} ms  ({launches(lambda: hip_step(emb, graph, trans, w))} kernels incl. the torch scalar ops of the loss)')
        print(f'  torch composite fwd + bwd    {t_torch:9.3f} ms  ({launches(lambda: torch_step(emb, src, tgt, trans, w))} kernels); max|grad difference| {err:.2e}')
        print(f'  build + HIP fwd + bwd        {t_build + t_hip:9.3f} ms')
        print(f'  cross-partition weights HIP  {t_xp:9.3f} ms  ({launches(lambda: ops.crosspartition_weights(graph, pred, trans, 50.0))} kernels, host syncs: one per component round)', flush=True)
        if n <= 100_000 and '--no-host' not in sys.argv:
            h = [a.cpu().numpy() for a in (src, tgt, trans, pred)]
            t0 = time.perf_counter()
            wh = host_xpart(n, h[0], h[1], h[2] != 0, h[3], 50.0)
            t_host = (time.perf_counter() - t0) * 1e3
            wd = ops.crosspartition_weights(graph, pred, trans, 50.0).cpu().numpy()
            print(f'  cross-partition weights host {t_host:9.3f} ms  (scipy components + a mask per boundary pair); bit-equal to the device: {np.array_equal(wh.view(np.uint32), wd.view(np.uint32))}', flush=True)
        del graph
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
