"""Side benchmark of the recurrent graph convolution at the state widths 8, 16, 64 and 128 (csrc/spg_ecc_wide.hip):
python tools/wide_cell_bench.py [--n 1000] [--e 5000] [--r 10] [--reps 100]
Forward + backward of graphnet.GraphNetwork('gru_R_<vv>' / 'lstm_R_<vv>') in training mode on one synthetic scene, for every new width
and filter mode, and beside them the 32-wide PER-ITERATION path (spg_tune key 8 = 1) of the same run.  Warm-up, then events around
`reps` repeats.  Printed per row: us per forward + backward, us per iteration (/ R), the same relative to the 32-wide per-iteration
figure of that cell and filter mode, and what the arithmetic alone would give (nc^2 / 32^2 for matrix filters -- cell and filters --
and for the cell under vector filters, whose filters grow with nc / 32 only).  Figures for profiles/wide_cell_bench.txt; no threshold."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from oracle import spg_oracle as O  # noqa: E402
from superpoint_graph_amd import _lib, synth  # noqa: E402
from superpoint_graph_amd.learning import ecc, graphnet  # noqa: E402

FNET = [13, 32, 128, 64]


def timeit(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3       # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--e', type=int, default=5000)
    ap.add_argument('--r', type=int, default=10)
    ap.add_argument('--reps', type=int, default=100)
    a = ap.parse_args()
    dev = 'cuda'
    L = _lib.lib()
    col = synth.collate_numpy([synth.scene(0, n_sp=a.n, n_edges=a.e)])
    idxn, degs, ef, _ = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    idxn, degs, ef = torch.from_numpy(idxn), torch.from_numpy(degs), torch.from_numpy(ef).float()
    N, E = int(degs.numel()), int(idxn.numel())
    print(f'# python tools/wide_cell_bench.py: N = {N}, E = {E}, R = {a.r}, forward + backward of the module (training mode), {a.reps} repeats')
    print(f"{'cell':5s} {'nc':>4s} {'filters':8s} {'path':28s} {'us fwd+bwd':>11s} {'us / iteration':>15s} {'x 32-wide':>10s} {'arithmetic':>11s}")
    base = {}
    old = L.spg_tune(8, 1)                      # the 32-wide rows: one launch per iteration, like the other widths
    try:
        for cell in ('gru', 'lstm'):
            for matrix in (True, False):
                for nc in (32, 8, 16, 64, 128):
                    if matrix and nc > 64:
                        continue
                    torch.manual_seed(0)
                    net = graphnet.GraphNetwork(f'{cell}_{a.r}_{int(not matrix)}', nc, list(FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1).to(dev).train()
                    gi = ecc.GraphConvInfo.from_buffers(idxn.clone(), degs.clone(), ef.clone(), None, None)
                    net.set_info([gi], 1)
                    x = torch.randn(N, nc, device=dev, requires_grad=True)
                    go = torch.randn(N, nc * (a.r + 1), device=dev)

                    def step():
                        net.zero_grad(set_to_none=True)
                        x.grad = None
                        net(x).backward(go)
                    t = timeit(step, a.reps)
                    if nc == 32:
                        base[cell, matrix] = t
                    rel = t / base[cell, matrix]
                    arith = (nc / 32) ** 2
                    path = 'per-iteration (key 8 = 1)' if nc == 32 else 'wide kernels, per iteration'
                    print(f"{cell:5s} {nc:4d} {'matrix' if matrix else 'vector':8s} {path:28s} {t:11.1f} {t / a.r:15.1f} {rel:10.2f} {arith:11.2f}", flush=True)
    finally:
        L.spg_tune(8, old)


if __name__ == '__main__':
    main()
