"""Writes tests/golden/part_reduce_parent.npz: the bits of the partition units' fixed-order reductions (tests/part_reduce_cases.py)
as the commit BEFORE they moved into csrc/spg_part.h computes them on an MI355X.  Run it on a checkout and build of that commit --
the whole tree, its Python wrappers (then one file, now the superpoint_graph_amd/ops package) included -- never on a later one: the
file is the record that the move changed no bit.

  <case>/<field>    what part_reduce_cases.CASES[case] returns: small results whole, per-point arrays as SHA-256 digests
  parent_commit     the commit the record was taken on (--commit, default: git rev-parse HEAD)

Run from the repository root: python tools/gen_part_reduce_golden.py [--commit HASH] [--out PATH]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import part_reduce_cases as C    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'part_reduce_parent.npz'))
    a = ap.parse_args()
    commit = a.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    from superpoint_graph_amd import ops
    out = {'parent_commit': np.array(commit)}
    for name, run in C.CASES.items():
        first, again = run(ops), run(ops)
        for field, value in first.items():
            assert value.dtype == again[field].dtype and value.tobytes() == again[field].tobytes(), (name, field, 'two runs differ')
            out[f'{name}/{field}'] = value
        print(name, {k: (v.tolist() if v.size <= 6 and v.dtype != np.uint8 else v.tobytes().hex()[:12]) for k, v in first.items()})
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), 'bytes, parent', commit)


if __name__ == '__main__':
    main()
