"""Batches of the learned partition on the device (csrc/spg_tiles.hip) timed with hipEvents around the library calls themselves
(outputs allocated beforehand, no host synchronisation inside the timed region): the neighbourhood tiles at 1e4, 1e6 and 4e6
vertices, k = 20, with and without rgb, with plain and with non-temporal stores -- device time (median, min - max), bytes written
per second and their fraction of 8 TB/s -- next to the reference's numpy expression (graph_processing.py:393-401) on this host
plus the host-to-device copy its tiles would have needed; and ops.random_subgraph on a k-nearest-neighbour-like graph of 1e6
vertices at size 1e4 and on a path of 1e4 vertices (one vertex per level: the worst case of the level-synchronous kernel).
First measurements: there is no threshold on any of these numbers.
    python tools/tiles_bench.py [--no-large] [--no-host]      (GPU only)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superpoint_graph_amd import ops
from superpoint_graph_amd._lib import check, lib

K, PEAK = 20, 8e12


def spread(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def make_cloud(n, seed=0):
    """Points in scan order with neighbours among the 400 points around them: the locality of a voxel-ordered cloud."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    xyz = torch.rand(n, 3, device='cuda', generator=g) * 10
    rgb = torch.rand(n, 3, device='cuda', generator=g)
    nei = (torch.arange(n, device='cuda')[:, None] + torch.randint(-200, 201, (n, K), device='cuda', generator=g)).clamp_(0, n - 1).to(torch.int32)
    nei[:, 0] = torch.arange(n, device='cuda', dtype=torch.int32)
    return xyz, rgb, nei.contiguous(), torch.rand(n, device='cuda', generator=g), torch.rand(n, 2, device='cuda', generator=g)


def tiles_call(xyz, rgb, nei, e, xyn, use_rgb, stream):
    n, F, G = xyz.shape[0], 6 if use_rgb else 3, 7
    clouds = torch.empty(n, F, K, device='cuda')
    cg, diam = torch.empty(n, G, device='cuda'), torch.empty(n, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    L, st = lib(), torch.cuda.current_stream().cuda_stream

    def fn():
        check(L.spg_neighbourhood_tiles(xyz.data_ptr(), rgb.data_ptr(), n, nei.data_ptr(), 0, K, K, None, n, 1 if use_rgb else 0, e.data_ptr(),
                                        xyn.data_ptr(), 1, 0, 1 if stream else 0, clouds.data_ptr(), cg.data_ptr(), diam.data_ptr(), err.data_ptr(), st))
    return fn, clouds, err


def host_expression(xyz, rgb, nei, use_rgb):
    t0 = time.perf_counter()
    clouds = xyz[nei, ]
    diameters = np.sqrt(clouds.var(1).sum(1))
    clouds = (clouds - xyz[:, np.newaxis, :]) / (diameters[:, np.newaxis, np.newaxis] + 1e-10)
    if use_rgb:
        clouds = np.concatenate([clouds, rgb[nei, ]], axis=2)
    clouds = clouds.transpose([0, 2, 1])
    t_expr = (time.perf_counter() - t0) * 1e3
    t = torch.from_numpy(clouds)              # (as graph_loader returns it: a transposed view; run_batch's .cuda() makes it contiguous)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = t.cuda()
    torch.cuda.synchronize()
    return t_expr, (time.perf_counter() - t0) * 1e3, d


def bench_tiles(n, reps, host):
    xyz, rgb, nei, e, xyn = make_cloud(n)
    for use_rgb in (1, 0):
        F = 6 if use_rgb else 3
        written = n * (F * K + 7 + 1) * 4
        print(f'tiles: n = {n}, k = {K}, F = {F} ({written / 1e6:.1f} MB written):', flush=True)
        got = None
        for stream in (0, 1):
            fn, clouds, err = tiles_call(xyz, rgb, nei, e, xyn, use_rgb, stream)
            med, lo, hi = spread(fn, reps)
            assert int(err.item()) == 0
            print(f'  device, {"non-temporal" if stream else "plain       "} stores  {med:9.4f} ms  ({lo:.4f} - {hi:.4f}, {reps} runs)  {written / (med * 1e-3) / 1e9:8.1f} GB/s written'
                  f' = {100 * written / (med * 1e-3) / PEAK:5.1f} % of 8 TB/s', flush=True)
            got = clouds if got is None else got
            assert torch.equal(got.view(torch.int32), clouds.view(torch.int32)), 'the two store forms differ'
            del fn, clouds
        if host:
            t_expr, t_copy, d = host_expression(xyz.cpu().numpy(), rgb.cpu().numpy(), nei.cpu().numpy().astype(np.int64), use_rgb)
            equal = bool(torch.equal(d.contiguous().view(torch.int32), got.view(torch.int32)))
            print(f'  host numpy expression        {t_expr:9.1f} ms  + copy of its tiles to the device {t_copy:9.1f} ms; bit-equal to the device: {equal}', flush=True)
            del d
        del got
        torch.cuda.empty_cache()


def subgraph_call(graph, size, seeds):
    n, E = graph.n, graph.E
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    sv = torch.zeros(n, dtype=torch.uint8, device='cuda')
    se = torch.empty(E, dtype=torch.uint8, device='cuda')
    state = torch.zeros(3, dtype=torch.int64, device='cuda')
    ws = torch.empty(L.spg_random_subgraph_workspace_bytes(n), dtype=torch.uint8, device='cuda')
    seeds = torch.tensor(seeds, dtype=torch.int64, device='cuda')

    def fn():
        sv.zero_(); state.zero_()
        check(L.spg_random_subgraph(graph.rowptr.data_ptr(), graph.inc.data_ptr(), graph.ends.data_ptr(), E, n, size, seeds.data_ptr(), seeds.numel(),
                                    sv.data_ptr(), se.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return fn, state


def bench_subgraph(reps):
    g = torch.Generator(device='cuda').manual_seed(1)
    n, k = 1_000_000, 5
    src = torch.arange(n, device='cuda').repeat_interleave(k)
    tgt = (src + torch.randint(1, 200, (n * k,), device='cuda', generator=g)) % n
    cases = [('k-nn-like graph, n = 1e6, E = 5e6, size 1e4', ops.EdgeGraph(src, tgt, n), 10_000, [n // 2]),
             ('path, n = 1e4, size 1e4 (one vertex per level)', ops.EdgeGraph(torch.arange(9_999, device='cuda'), torch.arange(1, 10_000, device='cuda'), 10_000), 10_000, [0]),
             ('path, n = 1e4, size 1e4, from the middle', ops.EdgeGraph(torch.arange(9_999, device='cuda'), torch.arange(1, 10_000, device='cuda'), 10_000), 10_000, [5_000])]
    for name, graph, size, seeds in cases:
        fn, state = subgraph_call(graph, size, seeds)
        med, lo, hi = spread(fn, reps, warm=1)
        print(f'random_subgraph: {name}: {med:9.3f} ms  ({lo:.3f} - {hi:.3f}, {reps} runs); n_seen {int(state[0])}, seeds used {int(state[1])}', flush=True)
    graph = cases[0][1]
    se, sv, _, _, _ = ops.random_subgraph(graph, 10_000, [n // 2])
    fn = lambda: ops.induced_subgraph(graph, sv, se)
    med, lo, hi = spread(fn, reps)
    print(f'induced_subgraph: n = 1e6, E = 5e6, 1e4 selected (with its host read of the two counts): {med:9.3f} ms  ({lo:.3f} - {hi:.3f})', flush=True)


def main():
    host = '--no-host' not in sys.argv
    print(torch.cuda.get_device_name(0), '; host threads', torch.get_num_threads(), flush=True)
    for n, reps in [(10_000, 30), (1_000_000, 20)] + ([] if '--no-large' in sys.argv else [(4_000_000, 10)]):
        bench_tiles(n, reps, host)
    bench_subgraph(7)


if __name__ == '__main__':
    main()
