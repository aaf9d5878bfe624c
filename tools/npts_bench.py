#!/usr/bin/env python3
"""Cost of PointNet above 128 points per superpoint at a constant 128 000 points:
python tools/npts_bench.py [--windows W] [--steps K] [--warmup N] [--out FILE]

Shapes: 1000 x 128 (the baseline: one segment per superpoint, the code path of every build before the segment plan), 500 x 256,
250 x 512 (two / four segments of 128 points) and 800 x 160 (two segments of 80 points: the 80-point tile forms).  Production model
(bench.build_model), five superedges per superpoint.  Two figures per shape, each the MEDIAN over W windows of K calls (a window ends
in a device synchronise; the shapes alternate window by window, so drift of the box hits all of them alike):
  pointnet   forward + backward of model.ptn in train mode, through the module (autograd node around the two library calls)
  step       zero_grad + spg_train_step (FusedStep) + clamp / Adam: PointNet, RNN-ECC, classifier, loss, optimiser -- the RNN-ECC
             part shrinks with the number of superpoints, so this ratio is not PointNet's alone
Ratios are to the baseline shape.  A ratio is reported, not asserted."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SHAPES = [(1000, 128), (500, 256), (250, 512), (800, 160)]
N_FEAT, N_CLASSES, CONFIG = 14, 13, 'gru_10_0,f_13'


def make_shape(n_sp, n_pts, dev):
    from superpoint_graph_amd import fused, synth
    from superpoint_graph_amd.flat import FlatParameters
    from superpoint_graph_amd.learning import spg
    scene = synth.scene(0, n_sp=n_sp, n_edges=5 * n_sp, n_feat=N_FEAT, n_pts=n_pts, n_classes=N_CLASSES)
    targets, GIs, (meta, flag, clouds, diam) = spg.eccpc_collate([spg.sample_from_scene(scene, 'scene0')])
    assert tuple(clouds.shape[1:]) == (N_FEAT, n_pts) and clouds.shape[0] >= 0.99 * n_sp, tuple(clouds.shape)      # (the embeddable superpoints)
    model = bench.build_model(CONFIG, dev, N_FEAT).train()
    model.ecc.set_info(GIs, 1)
    arena = FlatParameters(model, lazy_zero=True, host_counters=True)
    step = fused.FusedStep(model, arena, reduction='mean', ptn_mem_monger=True)
    clouds_d, diam_d, label = clouds.to(dev), diam.to(dev), targets[:, 0].to(dev)
    g = torch.randn(clouds.shape[0], 32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def pointnet_call():
        arena.zero_grad()
        model.ptn(clouds_d, diam_d).backward(g)

    def step_call():
        arena.zero_grad()
        step(flag, clouds_d, diam_d, GIs[0], label)
        arena.adam_step(lr=1e-3, weight_decay=0.0, grad_clip=1.0)
    return dict(pointnet=pointnet_call, step=step_call)


def window(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/npts_bench.py needs a GPU: nothing is timed on the CPU')
    dev = torch.device('cuda', 0)
    calls = {s: make_shape(s[0], s[1], dev) for s in SHAPES}
    times = {(s, what): [] for s in SHAPES for what in ('pointnet', 'step')}
    for what in ('pointnet', 'step'):
        for s in SHAPES:
            for _ in range(a.warmup):
                calls[s][what]()
        for _ in range(a.windows):
            for s in SHAPES:
                times[(s, what)].append(window(calls[s][what], a.steps))
    from superpoint_graph_amd import ops
    lines = [f'PointNet above 128 points per superpoint at {SHAPES[0][0] * SHAPES[0][1]} points ({torch.cuda.get_device_name(0)}; {CONFIG}, '
             f'{N_FEAT} features; median of {a.windows} windows of {a.steps} calls, {a.warmup} warm-up calls; min - max in brackets)',
             f'{"shape":>11s} {"segments":>9s} {"pointnet fwd+bwd":>28s} {"ratio":>6s} {"fused step + Adam":>28s} {"ratio":>6s}']
    base = {what: statistics.median(times[(SHAPES[0], what)]) for what in ('pointnet', 'step')}
    for s in SHAPES:
        ps, nseg = ops.model.pointnet_segments(s[1])
        cols = []
        for what in ('pointnet', 'step'):
            t = times[(s, what)]
            med = statistics.median(t)
            cols.append(f'{med * 1e3:8.3f} ms [{min(t) * 1e3:6.3f} - {max(t) * 1e3:6.3f}] {med / base[what]:6.3f}')
        lines.append(f'{s[0]:>5d} x {s[1]:<3d} {nseg:>3d} x {ps:<3d}   {cols[0]} {cols[1]}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
