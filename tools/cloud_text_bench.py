"""The raw cloud readers measured (GPU only): writes profiles/cloud_text_bench.txt and profiles/cloud_text_errors.txt.

Input: 10 000 000 Semantic3D lines `x y z i r g b` held in memory (about 376 MB): a seeded block of 100 000 distinct lines, written
100 times (generating ten million distinct lines in Python takes longer than everything measured; neither parser can profit
from the repetition, the copies lie 3.8 MB apart).
* device time (events) of the three library calls of ops.parse_cloud_text on the resident bytes: spg_text_index (count kernel,
  rocPRIM maximum and scan, head), spg_text_lines (place kernel), spg_text_parse; bytes/s = the bytes each call must move (counted below) over that time, against the measured HBM copy rate;
* host wall time of upload (from a page-locked buffer) + ops.parse_cloud_text, ending in a synchronise;
* pandas.read_csv on the same bytes on the same host in the same call, alternated with the device path, three repeats each;
* the compiler's registers / LDS / scratch of the kernels (hipcc -Rpass-analysis=kernel-resource-usage, when hipcc is there);
* the case table: lines, refused lines and code per case of tests/cloud_text_cases.py, bit-equal to the restatement or not.
    python tools/cloud_text_bench.py [--lines 10000000] [--reps 3] [--out profiles/cloud_text_bench.txt] [--cases-out ...]"""
import argparse
import io
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cloud_text_cases as C  # noqa: E402
import cloud_text_restatement as R  # noqa: E402
from superpoint_graph_amd import ops  # noqa: E402
from superpoint_graph_amd.ops.text import _text_roles  # noqa: E402
from superpoint_graph_amd._lib import CSRC, check, lib  # noqa: E402

HBM_COPY = 6.29e12            # bytes/s, the measured float4 copy of an MI355X (8.0e12 on paper)


def events(fn, reps):
    """median device milliseconds of fn() over reps, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def kernels(text, reps, say):
    L, st, dev = lib(), torch.cuda.current_stream().cuda_stream, text.device
    nb = text.numel()
    ws = torch.empty(L.spg_text_workspace_bytes(nb), dtype=torch.uint8, device=dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    index = lambda: check(L.spg_text_index(text.data_ptr(), nb, 1, head.data_ptr(), ws.data_ptr(), ws.numel(), st))
    t_index, all_index = events(index, reps)
    n = int(head[0])
    line_start = torch.empty(n, dtype=torch.int64, device=dev)
    lines = lambda: check(L.spg_text_lines(text.data_ptr(), nb, n, line_start.data_ptr(), ws.data_ptr(), ws.numel(), st))
    t_lines, all_lines = events(lines, reps)
    xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(n, 3, dtype=torch.uint8, device=dev)
    err = torch.empty(4, dtype=torch.int64, device=dev)
    roles = _text_roles(7, (0, 1, 2), (4, 5, 6), None)
    parse = lambda: check(L.spg_text_parse(text.data_ptr(), nb, line_start.data_ptr(), n, 7, roles, xyz.data_ptr(), rgb.data_ptr(),
                                           None, err.data_ptr(), st))
    t_parse, all_parse = events(parse, reps)
    assert err.tolist()[3] == 0
    say(f'device time, median of {reps} (all runs), and the bytes each call must move over it; roof = {HBM_COPY / 1e12:.2f} TB/s measured HBM copy')
    rows = [('spg_text_index', t_index, all_index, nb), ('spg_text_lines', t_lines, all_lines, nb + 8 * n)]
    rows += [('spg_text_parse', t_parse, all_parse, nb + 8 * n + 15 * n)]
    for name, t, runs, moved in rows:
        rate = moved / (t * 1e-3)
        say(f'  {name:34s} {t:8.3f} ms  ({", ".join(f"{r:.3f}" for r in runs)})  {moved / 1e6:8.1f} MB  {rate / 1e9:8.1f} GB/s = '
            f'{100 * rate / HBM_COPY:5.1f} % of the roof')
    return n


def resources(say):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        say('compiler resources: hipcc not found, not recorded')
        return
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', 'spg_text.hip', '-o', os.devnull,
           '-Rpass-analysis=kernel-resource-usage']
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    say('compiler resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):')
    name = None
    for line in r.stderr.splitlines():
        if 'Function Name:' in line:
            name = line.split('Function Name:')[1].split('[')[0].strip()
            keep = 'text_' in name
            row = []
        elif name and keep:
            for key in ('VGPRs:', 'TotalSGPRs:', 'ScratchSize [bytes/lane]:', 'Occupancy [waves/SIMD]:', 'LDS Size [bytes/block]:'):
                if key in line:
                    row.append(f'{key} {line.split(key)[1].split("[-R")[0].strip()}')
            if 'LDS Size' in line:
                say(f'  {name}: ' + ', '.join(row))
                name = None


def case_table(path):
    layout = ops.text_layout()
    out = [f'# name, bytes, lines, refused lines, code, bit-equal to tests/cloud_text_restatement.py; layout {layout}']
    spec = lambda c: {k: c[k] for k in ('n_cols', 'xyz_cols', 'rgb_cols', 'label_col')}

    def same(a, b):
        return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())
    for name, c in C.parse_cases(layout) + C.refusal_cases(layout):
        text = torch.frombuffer(bytearray(c['data']), dtype=torch.uint8).cuda() if c['data'] else torch.empty(0, dtype=torch.uint8, device='cuda')
        try:
            ref = R.parse(c['data'], **spec(c))
        except R.Refused as e:
            ref = e
        try:
            got = ops.parse_cloud_text(text, **spec(c))
            n, refused, code = got[3], 0, 0
            ok = not isinstance(ref, R.Refused) and got[3:] == ref[3:] and all(
                same(None if a is None else a.cpu().numpy(), None if b is None else b + b.dtype.type(0)) for a, b in zip(got[:3], ref[:3]))
        except ops.CloudTextError as e:
            n, refused, code = len(R.lines_of(c['data'])[0]), e.refused, e.code
            ok = isinstance(ref, R.Refused) and (e.code, e.line, e.offset, e.refused) == (ref.code, ref.line, ref.offset, ref.refused)
        out.append(f'{name:32s} {len(c["data"]):6d} {n:4d} {refused:2d} {code:2d}  {"equal" if ok else "DIFFERENT"}')
    with open(path, 'w') as f:
        f.write('\n'.join(out) + '\n')
    return sum('DIFFERENT' in line for line in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lines', type=int, default=10_000_000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cloud_text_bench.txt'))
    ap.add_argument('--cases-out', default=os.path.join(ROOT, 'profiles', 'cloud_text_errors.txt'))
    ap.add_argument('--no-pandas', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'cloud_text_bench needs a GPU'
    log = []

    def say(line):
        print(line, flush=True)
        log.append(line)
    different = case_table(args.cases_out)
    say(f'case table: {args.cases_out}: {different} case(s) different')
    block = C.sema_text(2024, 100_000)
    data = block * (args.lines // 100_000) + C.sema_text(2025, args.lines % 100_000)
    say(f'{torch.cuda.get_device_name(0)}; input: {args.lines} Semantic3D lines, {len(data)} bytes ({len(data) / args.lines:.1f} per line), in memory')
    pinned = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
    text = pinned.cuda()
    n = kernels(text, args.reps, say)
    assert n == args.lines
    del text
    torch.cuda.empty_cache()

    def device_path():
        t0 = time.perf_counter()
        out = ops.parse_cloud_text(pinned.to('cuda', non_blocking=True), 7, (0, 1, 2), (4, 5, 6))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    device_path()
    dev_s, pd_s, values = [], [], None
    for _ in range(args.reps):
        t, out = device_path()
        dev_s.append(t)
        if not args.no_pandas:
            import pandas as pd
            t0 = time.perf_counter()
            values = pd.read_csv(io.BytesIO(data), sep=' ', header=None).values
            pd_s.append(time.perf_counter() - t0)
    say(f'host wall time, upload from a page-locked buffer + ops.parse_cloud_text + synchronise: median {statistics.median(dev_s) * 1e3:.1f} ms '
        f'({", ".join(f"{t * 1e3:.1f}" for t in dev_s)}) = {len(data) / statistics.median(dev_s) / 1e9:.2f} GB/s of text')
    if pd_s:
        same_xyz = np.array_equal((np.array(values[:, 0:3], dtype='float32') + np.float32(0)).view(np.uint32), out[0].cpu().numpy().view(np.uint32))
        same_rgb = np.array_equal(np.array(values[:, 4:7], dtype='uint8'), out[1].cpu().numpy())
        say(f'pandas {__import__("pandas").__version__} read_csv(sep=" ", header=None) on the same bytes, alternated: median '
            f'{statistics.median(pd_s):.2f} s ({", ".join(f"{t:.2f}" for t in pd_s)})')
        say(f'ratio pandas / device path (upload included): {statistics.median(pd_s) / statistics.median(dev_s):.0f}x; '
            f'xyz bit-equal to pandas: {same_xyz}, rgb equal: {same_rgb}')
    resources(say)
    with open(args.out, 'w') as f:
        f.write('\n'.join(log) + '\n')


if __name__ == '__main__':
    main()
