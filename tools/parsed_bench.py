"""Times learning/parsed.py: preprocess_scene on one synthetic S3DIS-room-sized scene (default 1 000 000 points, 1 500 superpoints,
the s3dis recipe with z / 4 - 0.5) on the GPU: warm-up, then the median over several runs of the whole call (host clock around a
synchronise) and of the three stages by hand (device events: the scene statistics, the row gather, the class count), next to the
numpy restatement of the same body on the host (tests/parsed_restatement.py: scene()).  The gather is set against its byte
roofline: per row 4 (component index) + 12 (xyz) + 3 (rgb, uint8) + 16 (geof) bytes read and 4 * ncols
written, at the bandwidth --peak-gbs (default 8000: the MI355X's HBM3E figure).
    python tools/parsed_bench.py [--points 1000000] [--components 1500] [--runs 9] [--out FILE]"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import parsed_cases as C  # noqa: E402
import parsed_restatement as R  # noqa: E402
from superpoint_graph_amd import ops  # noqa: E402
from superpoint_graph_amd.ops._core import _ptr, _stream  # noqa: E402
from superpoint_graph_amd.learning import parsed  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--components', type=int, default=1500)
    ap.add_argument('--runs', type=int, default=9)
    ap.add_argument('--peak-gbs', type=float, default=8000.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n = a.points
    case = C.make('bench', 's3dis', C.room(n, 0.0, 1), 1, components=C.partition(n, a.components, 1))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    xyz, rgb, geof, labels = t(case['xyz']), t(case['rgb']), t(case['geof']), t(case['labels'])
    off = np.zeros(len(case['components']) + 1, np.int64)
    np.cumsum([len(c) for c in case['components']], out=off[1:])
    idx = t(np.concatenate(case['components']).astype(np.int32))
    n_trim = int(sum(len(c) > 10000 for c in case['components']))

    def whole():
        random.seed(case['seed'])
        t0 = time.perf_counter()
        p = parsed.preprocess_scene('s3dis', xyz, rgb, (off, idx), geof=geof, labels=labels)
        torch.cuda.synchronize()
        return p, (time.perf_counter() - t0) * 1e3

    L = ops.lib()
    P, S = _ptr, _stream
    s32, s64, cen = ops.scene_stats(xyz, True)
    off_d = torch.from_numpy(off).cuda()
    rows = int(off[-1])
    points = torch.empty(rows, 15, dtype=torch.float32, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    ws = torch.empty(max(L.spg_parsed_workspace_bytes(n), 256), dtype=torch.uint8, device='cuda')
    count = torch.empty(13, dtype=torch.int64, device='cuda')
    stage = {
        'scene statistics (3 passes)': lambda: ops.check(L.spg_parsed_stats(P(xyz), n, 1, P(s32), P(s64), P(cen), P(err), P(ws), ws.numel(), S())),
        'row gather': lambda: ops.check(L.spg_parsed_rows(0, P(xyz), n, P(rgb), 0, P(geof), None, 0, P(s32), P(s64), P(off_d), P(off_d), len(off) - 1,
                                                         P(idx), 0, None, None, rows, P(points), P(err), S())),
        'class count': lambda: ops.check(L.spg_class_count(P(labels), 0, n, 13, P(count), S())),
    }
    for _ in range(3):
        whole()
        for fn in stage.values():
            fn()
    torch.cuda.synchronize()
    total = statistics.median(whole()[1] for _ in range(a.runs))
    ms = {k: statistics.median(timed(fn)[1] for _ in range(a.runs)) for k, fn in stage.items()}
    p = whole()[0]
    assert n_trim == 0 and torch.equal(p.points.view(torch.int32), points.view(torch.int32))

    random.seed(case['seed'])
    t0 = time.perf_counter()
    host = R.scene(case)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = p.points.cpu().numpy()
    exact = np.array_equal(np.delete(got, R.DIST_COLUMN, 1).view(np.uint32),
                           np.delete(np.concatenate(host['datasets'], 0).astype(np.float32), R.DIST_COLUMN, 1).view(np.uint32))
    moved = rows * (4 + 12 + 3 + 16 + 4 * 15)
    floor_ms = moved / (a.peak_gbs * 1e9) * 1e3
    lines = [f'n = {n}, {len(off) - 1} superpoints, {rows} rows of 15 columns (s3dis recipe, rgb uint8, int32 component indices), median of {a.runs}:',
             f'  preprocess_scene, whole call    {total:9.3f} ms  (host clock; statistics, gather, class count, three host reads, table uploads)']
    lines += [f'  {k:<31} {v:9.3f} ms  (device events)' for k, v in ms.items()]
    lines += [f'  row gather, byte roofline       {floor_ms:9.3f} ms  ({moved / 1e6:.1f} MB at {a.peak_gbs:.0f} GB/s: 35 B read + 60 B written per row) '
              f'-> the gather runs at {100 * floor_ms / ms["row gather"]:.1f} % of it ({moved / ms["row gather"] / 1e6:.0f} GB/s)',
              f'  numpy restatement, host         {host_ms:9.3f} ms  (features + gather + class count, one run); every exact column bit-equal to the device: {exact}']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
