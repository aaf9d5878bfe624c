"""The result writers measured (GPU only): writes profiles/result_text_bench.txt; with --resources (needs hipcc, no GPU)
profiles/result_text_resources.txt.

Two tables at 10^6 and 10^7 rows: a label column (uint8 values 1 ... 8, the Semantic3D submission) and `x y z r g b` (float32
coordinates of a scene tens of metres wide, uint8 colours: a PLY vertex).
* device time (events) of spg_format_measure (length kernel + rocPRIM scan) and spg_format_write on resident columns; bytes/s =
  the text written over measure + write, against the measured HBM copy rate;
* end to end: format on the device in blocks, copy to a page-locked buffer, write to a file (the writers' path:
  provider.write_label_file / provider.write_ply on host arrays, upload included), host wall time ending with the file closed;
* the comparators on the same host in the same process, alternated: numpy.savetxt(fmt='%d') on the labels, and plyfile's text
  path restated (one numpy.savetxt(stream, [record], '%.18g') per record) on 10^5 rows, SCALED to the row count (it is
  linear in the rows; running it on 10^7 rows would take minutes).
Warm-up first, medians of --reps, one process.
    python tools/result_text_bench.py [--rows 1000000 10000000] [--reps 5] [--out profiles/result_text_bench.txt]
    python tools/result_text_bench.py --resources"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY = 6.29e12            # bytes/s, the measured float4 copy of an MI355X (8.0e12 on paper)
PLYFILE_ROWS = 100_000


def resources(path):
    from superpoint_graph_amd._lib import CSRC
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', 'spg_format.hip', '-o', os.devnull,
           '-Rpass-analysis=kernel-resource-usage']
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    out = ['compiler resources of csrc/spg_format.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):']
    name = None
    for line in r.stderr.splitlines():
        if 'Function Name:' in line:
            name = line.split('Function Name:')[1].split('[')[0].strip()
            keep, row = 'format_' in name or 'error_colour' in name, []
        elif name and keep:
            for key in ('VGPRs:', 'TotalSGPRs:', 'ScratchSize [bytes/lane]:', 'Occupancy [waves/SIMD]:', 'LDS Size [bytes/block]:'):
                if key in line:
                    row.append(f'{key} {line.split(key)[1].split("[-R")[0].strip()}')
            if 'LDS Size' in line:
                out.append(f'  {name}: ' + ', '.join(row))
                name = None
    out.append('No kernel of the unit uses scratch memory: a field lives in three 64-bit registers filled through selects, the fixed-point')
    out.append('words and digit groups are indexed by unrolled loops only, and the column table is a kernel argument read with uniform indices.')
    with open(path, 'w') as f:
        f.write('\n'.join(out) + '\n')
    print('\n'.join(out))


def events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def wall(fn, reps, warm=True):
    if warm:
        fn()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        s.append(time.perf_counter() - t0)
    return statistics.median(s), s


def device_times(name, columns, reps, say):
    import ctypes

    import torch
    from superpoint_graph_amd._lib import check, lib
    from superpoint_graph_amd.ops.text import FORMAT_KINDS, FORMAT_MAX_FIELD, _format_columns
    flat, n = _format_columns(columns)
    L, st, nc = lib(), torch.cuda.current_stream().cuda_stream, len(flat)
    ptrs = (ctypes.c_void_p * nc)(*[t.data_ptr() for t in flat])
    kinds = (ctypes.c_int * nc)(*[FORMAT_KINDS[t.dtype] for t in flat])
    strides = (ctypes.c_long * nc)(*[int(t.stride(0)) for t in flat])
    ws = torch.empty(L.spg_format_workspace_bytes(n, nc), dtype=torch.uint8, device='cuda')
    row_start = torch.empty(n + 1, dtype=torch.int64, device='cuda')
    measure = lambda: check(L.spg_format_measure(ptrs, kinds, strides, nc, n, row_start.data_ptr(), ws.data_ptr(), ws.numel(), st))
    t_m, all_m = events(measure, reps)
    total = int(row_start[n])
    out = torch.empty(total, dtype=torch.uint8, device='cuda')
    write = lambda: check(L.spg_format_write(ptrs, kinds, strides, nc, n, row_start.data_ptr(), total, out.data_ptr(), total, st))
    t_w, all_w = events(write, reps)
    rate = total / ((t_m + t_w) * 1e-3)
    say(f'  {name:10s} {n:9d} rows  {total / 1e6:7.1f} MB ({total / n:5.1f} B/row)  measure {t_m:7.3f} ms ({", ".join(f"{r:.3f}" for r in all_m)})  '
        f'write {t_w:7.3f} ms ({", ".join(f"{r:.3f}" for r in all_w)})  {rate / 1e9:7.1f} GB/s of text = {100 * rate / HBM_COPY:5.2f} % of the roof')
    # The other layout, format ONCE into fixed slots and compact afterwards, bounded from below with the same kernels: the write kernel
    # on row_start = r * slot (every row at the start of a slot of the longest possible row), the scan of the lengths (torch.cumsum
    # stands in for it) and a plain device copy of the text's bytes, which a compaction kernel cannot beat.
    slot = sum(FORMAT_MAX_FIELD[t.dtype] + 1 for t in flat)
    slots = torch.empty(n * slot, dtype=torch.uint8, device='cuda')
    slot_start = torch.arange(n + 1, dtype=torch.int64, device='cuda') * slot
    t_s, all_s = events(lambda: check(L.spg_format_write(ptrs, kinds, strides, nc, n, slot_start.data_ptr(), n * slot, slots.data_ptr(), n * slot, st)), reps)
    lengths = row_start[1:] - row_start[:-1]
    t_c, _ = events(lambda: torch.cumsum(lengths, 0), reps)
    t_p, _ = events(lambda: out.copy_(slots[:total]), reps)
    say(f'  {"":10s} slots variant, lower bound: format once into {slot}-byte slots {t_s:7.3f} ms ({", ".join(f"{r:.3f}" for r in all_s)}) + scan {t_c:.3f} ms '
        f'+ copy of the text {t_p:.3f} ms = {t_s + t_c + t_p:7.3f} ms against {t_m + t_w:7.3f} ms of measure + write')


def savetxt_records(path, xyz, rgb):
    """plyfile's text path restated: one numpy.savetxt per record"""
    with open(path, 'wb') as f:
        for i in range(len(xyz)):
            np.savetxt(f, [[xyz[i, 0], xyz[i, 1], xyz[i, 2], rgb[i, 0], rgb[i, 1], rgb[i, 2]]], '%.18g', newline='\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[1_000_000, 10_000_000])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'result_text_bench.txt'))
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--resources-out', default=os.path.join(ROOT, 'profiles', 'result_text_resources.txt'))
    args = ap.parse_args()
    if args.resources:
        return resources(args.resources_out)
    import torch
    from superpoint_graph_amd.partition import provider as P
    assert torch.cuda.is_available(), 'result_text_bench needs a GPU'
    log = []

    def say(line):
        print(line, flush=True)
        log.append(line)
    say(f'{torch.cuda.get_device_name(0)}; numpy {np.__version__}; medians of {args.reps} after one warm-up (all runs in brackets)')
    rng = np.random.default_rng(5)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'out.txt')
    say(f'device time by events, columns resident; roof = {HBM_COPY / 1e12:.2f} TB/s measured HBM copy')
    data = {}
    for n in args.rows:
        labels = rng.integers(1, 9, n).astype(np.uint8)
        xyz = (rng.standard_normal((n, 3)) * np.array([30.0, 30.0, 3.0])).astype(np.float32)
        rgb = rng.integers(0, 256, (n, 3), dtype=np.uint64).astype(np.uint8)
        data[n] = (labels, xyz, rgb)
        device_times('labels', [torch.from_numpy(labels).cuda()], args.reps, say)
        device_times('xyzrgb', [torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()], args.reps, say)
    say(f'end to end on host arrays (upload, format in blocks of {P._WRITE_BLOCK} rows, copy to a page-locked buffer, write to a temporary folder), host wall time')
    for n in args.rows:
        labels, xyz, rgb = data[n]
        t_dev, all_dev = wall(lambda: P.write_label_file(path, labels, 0), args.reps)
        size = os.path.getsize(path)
        t_np, all_np = wall(lambda: np.savetxt(path, labels, delimiter=' ', fmt='%d'), 1 if n > 2_000_000 else 3, warm=n <= 2_000_000)
        assert os.path.getsize(path) == size
        say(f'  labels {n:9d} rows: write_label_file {t_dev * 1e3:8.1f} ms ({", ".join(f"{t * 1e3:.1f}" for t in all_dev)}); numpy.savetxt(fmt="%d") '
            f'{t_np:6.2f} s ({", ".join(f"{t:.2f}" for t in all_np)}); ratio {t_np / t_dev:.0f}x')
        t_dev, all_dev = wall(lambda: P.write_ply(path, xyz, rgb), args.reps)
        size = os.path.getsize(path)
        m = min(n, PLYFILE_ROWS)
        t_ply, all_ply = wall(lambda: savetxt_records(path, xyz[:m], rgb[:m]), 1, warm=False)
        say(f'  xyzrgb {n:9d} rows: write_ply {t_dev * 1e3:8.1f} ms ({", ".join(f"{t * 1e3:.1f}" for t in all_dev)}), {size / 1e6:.1f} MB; one '
            f'savetxt("%.18g") per record on {m} rows {t_ply:.2f} s = {t_ply / m * 1e6:.1f} us per vertex, SCALED to {n} rows: {t_ply / m * n:.1f} s; '
            f'ratio {t_ply / m * n / t_dev:.0f}x')
        # where the end-to-end time goes: the copy and the file write of the same bytes alone
        text = torch.empty(size, dtype=torch.uint8, device='cuda')
        pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
        t_copy, _ = wall(lambda: pinned.copy_(text), args.reps)

        def file_write():
            with open(path, 'wb') as f:
                f.write(memoryview(pinned.numpy()))
        t_file, _ = wall(file_write, args.reps)
        say(f'         of which, for the {size / 1e6:.1f} MB alone: device -> page-locked copy {t_copy * 1e3:.1f} ms, file write {t_file * 1e3:.1f} ms')
    with open(args.out, 'w') as f:
        f.write('\n'.join(log) + '\n')


if __name__ == '__main__':
    main()
