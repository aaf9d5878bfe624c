"""Exact kNN on the device (csrc/spg_knn.hip) timed: compute_graph_nn_2(., 10, 45)'s search (ops.knn, k = 45, self query) on
surface-like clouds, and interpolate_labels' 1-NN of a larger query set against a reference set, with the workspace bytes and
scipy cKDTree(workers=16) on the same box for comparison.
    python tools/knn_bench.py [n ...]  [--interp N_QUERY N_REF]  [--no-cpu]      (GPU only)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from superpoint_graph_amd import _lib, ops


def surface(n, seed=0, side=None):
    rng = np.random.default_rng(seed)
    side = np.sqrt(n / 1000.0) if side is None else side        # ~1000 points per square metre
    u, v = rng.uniform(0, side, n), rng.uniform(0, side, n)
    return np.stack([u, v, 0.5 * np.sin(u / 3) + 0.3 * np.cos(v / 5)], 1).astype(np.float32)


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    args = sys.argv[1:]
    cpu = '--no-cpu' not in args
    interp = None
    if '--interp' in args:
        i = args.index('--interp')
        interp = (int(args[i + 1]), int(args[i + 2]))
        del args[i:i + 3]
    sizes = [int(a) for a in args if not a.startswith('--')] or [200_000, 1_000_000, 10_000_000]
    L = _lib.lib()
    for n in sizes:
        xyz = surface(n)
        x = torch.from_numpy(xyz).cuda()
        reps = 5 if n <= 1_000_000 else 2
        dt = timed(lambda: ops.knn(x, 45), reps)
        ws = L.spg_knn_workspace_bytes(n, 0, 45)
        line = f'knn self k=45: {n} points: {dt * 1e3:.2f} ms (build + query) = {n / dt / 1e6:.1f} M points/s, workspace {ws / 1e6:.0f} MB'
        if cpu and n <= 1_000_000:
            from scipy.spatial import cKDTree
            t0 = time.perf_counter()
            cKDTree(xyz).query(xyz, 46, workers=16)
            line += f'; scipy cKDTree(workers=16) {time.perf_counter() - t0:.2f} s'
        print(line, flush=True)
    if interp:
        nq, nr = interp
        ref = torch.from_numpy(surface(nr, 1)).cuda()
        q = torch.from_numpy(surface(nq, 2, side=np.sqrt(nr / 1000.0))).cuda()      # the full cloud over the pruned one's extent
        index = ops.KnnIndex(ref, query_capacity=nq)
        dt = timed(lambda: index.query(q, 1, distances=False), 1)
        ws = L.spg_knn_workspace_bytes(nr, nq, 1)
        print(f'knn 1-NN: {nq} queries against {nr} points: {dt * 1e3:.1f} ms = {nq / dt / 1e6:.0f} M queries/s, '
              f'workspace {ws / 1e6:.0f} MB', flush=True)


if __name__ == '__main__':
    main()
