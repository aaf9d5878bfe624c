#!/usr/bin/env python3
"""Print every spg_*_workspace_bytes of the partition units for a fixed table of shapes (one line per query).

  SPG_HIP_LIB=/path/to/libspg_hip.so tools/partition_workspace_bytes.py

Run on two builds and compare line by line (profiles/partition_workspace_bytes.txt): a workspace must not grow.
"""
import ctypes
import os

NS = (1, 64, 65, 257, 100000)
ES = (0, 1, 300, 400000)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.environ.get('SPG_HIP_LIB') or os.path.join(here, '..', 'superpoint_graph_amd', 'csrc', 'libspg_hip.so')
    L = ctypes.CDLL(path)
    l, i = ctypes.c_long, ctypes.c_int

    def q(name, argtypes, *args):
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, ctypes.c_size_t
        print(f'{name}({", ".join(str(a) for a in args)}) = {f(*args)}')

    for n in NS:
        for which in (0, 1, 2):
            q('spg_spg_workspace_bytes', (i, l), which, n)
        q('spg_prune_workspace_bytes', (l,), n)
        for nq in (0,) + NS:
            q('spg_knn_workspace_bytes', (l, l, i), n, nq, 1)
        q('spg_cc_workspace_bytes', (l,), n)
        q('spg_relax_edges_workspace_bytes', (l,), n)
        q('spg_random_subgraph_workspace_bytes', (l,), n)
        for n_com in sorted({1, n}):
            q('spg_partition_index_workspace_bytes', (l, l), n, n_com)
            q('spg_component_mode_workspace_bytes', (l, l), n, n_com)
        for E in ES:
            q('spg_edgegraph_workspace_bytes', (l, l), n, E)
            q('spg_xpart_workspace_bytes', (l, l), n, E)
            q('spg_induced_subgraph_workspace_bytes', (l, l), n, E)
    for E in ES:
        q('spg_edge_forward_workspace_bytes', (l,), E)


if __name__ == '__main__':
    main()
