"""Times supervized_partition.graph_processing.build_structure on one synthetic scene (default 100 000 points, s3dis rule, pruned)
on the GPU: warm-up, then the median over several runs of the whole call (host clock around a synchronise) and of every stage
(device events around the same ops called by hand: prune, kNN, compute_geof, the three launches of csrc/spg_structure.hip, the
EdgeGraph), next to the numpy restatement of the same glue (tests/structure_restatement.py: structure()) on the host.
    python tools/structure_bench.py [--points 100000] [--runs 9] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import structure_restatement as R  # noqa: E402
from superpoint_graph_amd import _lib, ops  # noqa: E402
from superpoint_graph_amd.ops._core import _ptr, _stream  # noqa: E402
from superpoint_graph_amd.supervized_partition import graph_processing as GP  # noqa: E402

K_LOCAL, K_ADJ, N_LABELS, VOXEL = 20, 5, 13, 0.03


def scene(n, seed=0):
    rng = np.random.default_rng(seed)
    side = (n / 100000) ** 0.5 * 10
    xyz = (rng.uniform(0, 1, size=(n, 3)) * [side, side, 3]).astype(np.float32)
    objects = (np.floor(xyz[:, 0] / 2) * 64 + np.floor(xyz[:, 1] / 2) + 1).astype(np.int32)
    return xyz, rng.integers(0, 256, size=(n, 3)).astype(np.uint8), (objects % N_LABELS).astype(np.uint8), objects


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def stages(xyz, rgb, labels, objects, n_objects):
    """the ops of build_structure one by one -> ({stage: ms}, the arrays the host restatement starts from)"""
    L, t = _lib.lib(), {}
    (px, prgb, plab, hist), t['prune'] = timed(lambda: ops.prune(xyz, float(np.float32(VOXEL)), rgb, labels, objects, N_LABELS, n_objects))
    (nei, _), t['knn'] = timed(lambda: ops.knn(px, K_LOCAL, distances=False))
    geof, t['compute_geof'] = timed(lambda: ops.compute_geof(px, nei.reshape(-1), K_LOCAL))
    n, dev = int(px.shape[0]), px.device
    f32, i64, u8 = torch.float32, torch.int64, torch.uint8
    frame, err = torch.empty(5, dtype=f32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(L.spg_structure_frame_workspace_bytes(n), 256), dtype=u8, device=dev)
    elevation, xyn, rgbf = torch.empty(n, dtype=f32, device=dev), torch.empty(n, 2, dtype=f32, device=dev), torch.empty(n, 3, dtype=f32, device=dev)
    ids, src, tgt = (torch.empty(m, dtype=i64, device=dev) for m in (n, n * K_ADJ, n * K_ADJ))
    trans, active = torch.empty(n * K_ADJ, dtype=u8, device=dev), torch.empty(n * K_ADJ, dtype=u8, device=dev)
    g = geof.clone()
    _, t['structure_frame'] = timed(lambda: _lib.check(L.spg_structure_frame(_ptr(px), n, _ptr(frame), _ptr(err), _ptr(ws), ws.numel(), _stream())))
    _, t['structure_vertices'] = timed(lambda: _lib.check(L.spg_structure_vertices(
        _ptr(px), n, _ptr(frame), _ptr(prgb), _ptr(hist), int(hist.shape[1]), 1, None, 0, _ptr(elevation), _ptr(xyn), _ptr(rgbf), _ptr(g), _ptr(ids),
        _stream())))
    _, t['structure_edges'] = timed(lambda: _lib.check(L.spg_structure_edges(_ptr(nei), n, K_LOCAL, K_ADJ, _ptr(ids), _ptr(src), _ptr(tgt),
                                                                              _ptr(trans), _ptr(active), _ptr(err), _stream())))
    _, t['edge_graph'] = timed(lambda: ops.EdgeGraph(src, tgt, n))
    return t, (px, nei, hist, geof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=100000)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('structure_bench: needs the GPU (no CPU timing stands in for it)')
    xyz, rgb, labels, objects = scene(a.points)
    n_objects = int(objects.max()) + 1
    d = [torch.from_numpy(v).cuda() for v in (xyz, rgb, labels, objects)]
    args = types.SimpleNamespace(k_nn_local=K_LOCAL, k_nn_adj=K_ADJ, voxel_width=VOXEL, compute_geof=1, plane_model=0, use_voronoi=0.0)

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = GP.build_structure(*d, args, 's3dis', N_LABELS, n_objects=n_objects)
        torch.cuda.synchronize()
        return s, (time.perf_counter() - t0) * 1e3
    for _ in range(3):                                    # warm-up: code objects, rocPRIM's choices, the allocator
        whole(), stages(*d, n_objects)
    total = [whole()[1] for _ in range(a.runs)]
    per = [stages(*d, n_objects) for _ in range(a.runs)]
    px, nei, hist, geof = (v.cpu().numpy() for v in per[-1][1])
    host = []
    for _ in range(max(3, a.runs // 3)):
        t0 = time.perf_counter()
        ref = R.structure(px, nei, K_ADJ, hist, 'objects', geof)
        host.append((time.perf_counter() - t0) * 1e3)
    s = whole()[0]
    assert np.array_equal(s.is_transition.cpu().numpy(), ref['is_transition']) and np.array_equal(s.objects.cpu().numpy(), ref['objects'])
    med = {k: statistics.median(p[0][k] for p in per) for k in per[0][0]}
    glue = med['structure_frame'] + med['structure_vertices'] + med['structure_edges']
    n, C = len(px), hist.shape[1]
    bytes_glue = n * (12 + 12 + 3 + 4 * C + 4 + 8 + 12 + 8 + 8) + n * K_LOCAL * 4 + n * K_ADJ * (8 + 8 + 1 + 1 + 16)
    lines = [f'build_structure, synthetic scene: {a.points} points -> {n} vertices after prune (voxel {VOXEL}), {C} object columns, '
             f'k_nn_local {K_LOCAL}, k_nn_adj {K_ADJ}; {torch.cuda.get_device_name(0)}; median of {a.runs} runs after 3 warm-up runs',
             f'whole call (host clock, synchronised): median {statistics.median(total):.3f} ms, min {min(total):.3f}, max {max(total):.3f}',
             'stages (device events around the op called by hand; host reads of the op included):']
    lines += [f'  {k:20s} {v:9.3f} ms' for k, v in med.items()]
    lines += [f'glue of csrc/spg_structure.hip (frame + vertices + edges): {glue:.3f} ms for about {bytes_glue / 1e6:.1f} MB moved '
              f'({bytes_glue / glue / 1e6:.1f} GB/s; launch-bound at this size)',
              f'numpy restatement of the same glue on the host (tests/structure_restatement.py structure()): median {statistics.median(host):.3f} ms '
              f'of {len(host)} runs; results equal (is_transition, objects)']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
