"""First timing of the device cut pursuit (ops.cut_pursuit) -> profiles/cutpursuit_bench.txt.

Two synthetic scenes: one at the scale of the learned-partition tests and one of 100 000 vertices with k_nn_adj 10.  Per scene:
wall time of one ops.cut_pursuit call (synchronised; the host reads it makes are part of it), pulses per min cut, kernel
launches of the min cuts, and the only baseline there is: the numpy restatement (tests/cutpursuit_restatement.py) with scipy's
maximum_flow as its cut, on this machine's CPU.  The partitions of the two are compared.  Also prints the pulse counts of the
min-cut test cases, from which ops.MINCUT_MAX_PULSES is chosen (at least 8 times the largest).

    python tools/cutpursuit_bench.py [--large 100000] [--skip-host-large]"""
import argparse
import os
import sys
import time

import numpy as np
import scipy
import scipy.sparse as sp
import torch
from scipy.sparse.csgraph import maximum_flow
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cutpursuit_cases as CASES                      # noqa: E402
import cutpursuit_restatement as R                    # noqa: E402
from superpoint_graph_amd import ops                  # noqa: E402


def scene(n, k, n_regions, D, noise, seed):
    """n points in a box, planted regions = the Voronoi cells of n_regions seeds, observations = region value + noise, kNN graph"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)).astype(np.float32) * np.float32([10, 10, 3])
    seeds = xyz[rng.choice(n, n_regions, replace=False)]
    planted = cKDTree(seeds).query(xyz)[1]
    obs = (rng.random((n_regions, D))[planted] + noise * rng.standard_normal((n, D))).astype(np.float32)
    nn = cKDTree(xyz).query(xyz, k + 1)[1][:, 1:]
    src = np.repeat(np.arange(n), k)
    tgt = nn.reshape(-1)
    return obs, src.astype(np.int64), tgt.astype(np.int64), planted


def scipy_cut(n, src, tgt, cap, cost0, cost1):
    """the canonical min cut by scipy's maximum_flow (min_cut's signature; no pulses)"""
    s, t = n, n + 1
    keep = src != tgt
    rows = np.concatenate([src[keep], tgt[keep], np.full(n, s), np.arange(n)])
    cols = np.concatenate([tgt[keep], src[keep], np.arange(n), np.full(n, t)])
    vals = np.concatenate([cap[keep], cap[keep], cost1, cost0])
    A = sp.coo_matrix((vals, (rows, cols)), shape=(n + 2, n + 2)).tocsr().astype(np.int32)
    out = maximum_flow(A, s, t)
    resid = (A - out.flow).tocoo()
    ok = resid.data > 0
    rev = sp.csr_matrix((np.ones(ok.sum(), np.int8), (resid.col[ok], resid.row[ok])), shape=A.shape)     # head -> tails
    reach = np.zeros(n + 2, bool)
    reach[t] = True
    frontier = np.array([t])
    while len(frontier):
        nxt = np.unique(rev[frontier].indices)
        frontier = nxt[~reach[nxt]]
        reach[frontier] = True
    return reach[:n].astype(np.uint8), 0


def same_partition(a, b):
    pairs = np.unique(np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def run(name, obs, src, tgt, k_nn_adj, reg, cutoff, host):
    n, E = len(obs), len(src)
    w = np.ones(E, np.float32)
    lam = reg / (4 * k_nn_adj)
    g = ops.EdgeGraph(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), n)
    obs_d, w_d = torch.from_numpy(obs).cuda(), torch.from_numpy(w).cuda()
    times = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        comp, ncom, values, energies, stats = ops.cut_pursuit(obs_d, g, w_d, reg_strength=lam, cutoff=cutoff, weight_decay=0.7,
                                                              return_stats=True)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times = times[1:]
    print(f'{name}: n = {n}, E = {E} (k_nn_adj {k_nn_adj}), D = {obs.shape[1]}, reg_strength / (4 k) = {lam:.4g}, cutoff {cutoff}, decay 0.7')
    print(f'  device: {ncom} components after {len(energies)} iterations, {stats["merge_rounds"]} merge rounds; '
          f'wall time per call, median of 3 after a warm-up: {np.median(times) * 1e3:.1f} ms ({", ".join(f"{t * 1e3:.1f}" for t in times)})')
    print(f'  min cuts: {len(stats["pulses"])}, pulses per cut {stats["pulses"]} (largest {max(stats["pulses"], default=0)}), '
          f'kernel launches of the min cuts per call {stats["launches"]}')
    if host:
        t0 = time.perf_counter()
        ref = R.cut_pursuit(obs, src, tgt, w, None, reg_strength=lam, cutoff=cutoff, weight_decay=0.7, cut_fn=scipy_cut)
        th = time.perf_counter() - t0
        print(f'  host restatement with scipy {scipy.__version__} maximum_flow as the cut, one run: {th:.2f} s; '
              f'ratio host / device {th / np.median(times):.1f}x; same partition: {same_partition(ref[0], comp.cpu().numpy())} '
              f'(identical numbering: {np.array_equal(ref[0], comp.cpu().numpy())})')
    return max(stats['pulses'], default=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--large', type=int, default=100000)
    ap.add_argument('--skip-host-large', action='store_true')
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    worst = 0
    counts = {}
    for name, c in sorted(CASES.mincut_cases().items()):
        counts[name] = R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])[1]
    print('pulses of the min-cut test cases (restatement = device, asserted in tests/test_gpu_cutpursuit.py): '
          + ', '.join(f'{k} {v}' for k, v in counts.items()))
    worst = max(counts.values())
    obs, src, tgt, _ = scene(4096, 5, 12, 4, 0.05, seed=1)
    worst = max(worst, run('learned-partition scale', obs, src, tgt, 5, 0.8, 10, True))
    obs, src, tgt, _ = scene(a.large, 10, 60, 4, 0.05, seed=2)
    worst = max(worst, run('large scene', obs, src, tgt, 10, 0.8, 10, not a.skip_host_large))
    print(f'largest pulse count seen: {worst}; ops.MINCUT_MAX_PULSES = {ops.MINCUT_MAX_PULSES} = {ops.MINCUT_MAX_PULSES / max(worst, 1):.0f}x')


if __name__ == '__main__':
    main()
