"""Neighbourhood sub-sampling of a training sample (step 1 of learning/spg.py: loader), host path against device path, in one
process on one box: per sample the host time of SuperpointGraph.permute_vertices -> random_neighborhoods -> k_big_enough, the host
time of ops.sample_spg on the scene's resident graph (the same draws of the permutation and the centres included; its one
synchronisation of the sampler's stream included), and the device time of spg_sample_spg's launches by hipEvents (outputs allocated
beforehand, nothing else in the timed region).  Medians of --reps runs (at least 10), every run with its own seed.  Scenes:
synth.scene at 1000 / 5000 and 10 000 / 50 000 superpoints / superedges; --spg_augm_nneigh 100 --spg_augm_order 3
--spg_augm_hardcutoff 512 --ptn_minpts 40.  First measurements: there is no threshold on any of these numbers.
    python tools/spg_sample_bench.py [--reps 15] [--out profiles/spg_sample_bench.txt]      (GPU only)"""
import argparse, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superpoint_graph_amd import ops, synth
from superpoint_graph_amd._lib import check, lib
from superpoint_graph_amd.learning import spg

NNEIGH, ORDER, CUT, MINPTS = 100, 3, 512, 40


def draws(n, seed):
    random.seed(seed)
    perm = list(range(n))
    random.shuffle(perm)
    return perm, random.sample(range(n), k=NNEIGH)


def host_path(G, seed):
    random.seed(seed)
    t0 = time.perf_counter()
    perm = list(range(G.vcount()))
    random.shuffle(perm)
    H = G.permute_vertices(perm)
    H = spg.random_neighborhoods(H, NNEIGH, ORDER)
    if 0 < CUT < H.vcount():
        H = spg.k_big_enough(H, MINPTS, CUT)
    return (time.perf_counter() - t0) * 1e3, H


def device_path(rg, seed):
    t0 = time.perf_counter()
    perm, centres = draws(rg.n, seed)
    t1 = time.perf_counter()
    s = ops.sample_spg(rg, perm, centres, ORDER, MINPTS, CUT)
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3, s


def device_time(rg, seed, reps):
    """The launches of spg_sample_spg alone, on the current stream."""
    n, E, F, dev = rg.n, rg.E, int(rg.feats.shape[1]), rg.device
    perm, centres = (torch.tensor(v, device=dev) for v in draws(n, seed))
    i64 = torch.int64
    vids, degs, head = torch.empty(n, dtype=i64, device=dev), torch.empty(n, dtype=i64, device=dev), torch.empty(3, dtype=i64, device=dev)
    edges, kept = torch.empty(E, 2, dtype=i64, device=dev), torch.empty(E, dtype=i64, device=dev)
    feats = torch.empty(E, F, device=dev)
    L = lib()
    ws = torch.empty(L.spg_sample_spg_workspace_bytes(n, E), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fn():
        check(L.spg_sample_spg(rg.graph.ends.data_ptr(), E, n, perm.data_ptr(), centres.data_ptr(), NNEIGH, rg.sizes.data_ptr(), rg.feats.data_ptr(),
                               F, ORDER, MINPTS, CUT, vids.data_ptr(), edges.data_ptr(), kept.data_ptr(), feats.data_ptr(), degs.data_ptr(),
                               head.data_ptr(), ws.data_ptr(), ws.numel(), st))
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def fmt(ts):
    return f'{np.median(ts):9.3f} ms  ({min(ts):.3f} - {max(ts):.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'spg_sample_bench.txt'))
    a = ap.parse_args()
    reps = max(a.reps, 10)
    lines = [f'spg_sample_bench: {torch.cuda.get_device_name(0)}; nneigh {NNEIGH}, order {ORDER}, hardcutoff {CUT}, minpts {MINPTS}; '
             f'median (min - max) of {reps} runs, one seed per run']
    for n_sp, n_edges in ((1000, 5000), (10000, 50000)):
        sc = synth.scene(seed=0, n_sp=n_sp, n_edges=n_edges, n_pts=4)
        sizes = np.clip(np.round(np.random.RandomState(5).lognormal(np.log(60.0), 1.0, n_sp)), 1, 5000).astype(np.int64)
        E = len(sc['edges'])
        G = spg.SuperpointGraph(n_sp, sc['edges'], True, {'f': list(sc['edge_feats'])}, {'v': list(range(n_sp)), 's': list(sizes)})
        rg = ops.ResidentSPG(sc['edges'], sc['edge_feats'], sizes, n_sp)
        for seed in range(3):                                          # warm both paths
            host_path(G, seed); device_path(rg, seed)
        host, dev, drw = [], [], []
        for seed in range(100, 100 + reps):
            th, H = host_path(G, seed)
            td, tdraw, s = device_path(rg, seed)
            assert np.array_equal(np.array(H.vs['v']), s.vids.numpy()) and np.array_equal(np.asarray(H._edges), s.edges.cpu().numpy())
            host.append(th); dev.append(td); drw.append(tdraw)
        lines += [f'{n_sp} superpoints, {E} superedges (sample of seed {100 + reps - 1}: {s.n} vertices, {s.E} edges; both paths agree on every run)',
                  f'  host path, host time                       {fmt(host)}',
                  f'  device path, host time (ops.sample_spg)    {fmt(dev)}   of which the draws of perm and centres {np.median(drw):.3f} ms',
                  f'  device path, device time (hipEvents)       {fmt(device_time(rg, 100, reps))}']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
