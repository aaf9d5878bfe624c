"""Writes tests/golden/knn_graph.npz from the REFERENCE implementation (needs the reference checkout next to this repository:
SPG_REFERENCE or /root/reference, scikit-learn):  compute_graph_nn_2(xyz, 10, 45) and compute_graph_nn(xyz, 10) of
partition/graphs.py on two small clouds -- surface-like with exact duplicates, and grid-snapped (ties) -- and the 1-NN labels of
provider.interpolate_labels, called the way it calls scikit-learn.
    python tools/gen_knn_golden.py"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('SPG_REFERENCE', '/root/reference')


def load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clouds():
    rng = np.random.default_rng(11)
    n = 2400
    u, v = rng.uniform(0, 4, n), rng.uniform(0, 3, n)
    surf = np.stack([u, v, 0.3 * np.sin(u) + 0.05 * rng.normal(size=n)], 1).astype(np.float32)
    dup = rng.choice(n, 150, replace=False)
    surf[dup[:75]] = surf[dup[75:]]                         # exact duplicates
    g = rng.integers(0, 14, size=(2600, 3)).astype(np.float32) * np.float32(0.25)
    g[:, 2] *= np.float32(0.2)                              # grid-snapped: many equal distances
    return {'a': surf, 'b': g}


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    from sklearn.neighbors import NearestNeighbors
    graphs = load('partition/graphs.py', 'ref_graphs')
    out = {}
    for tag, xyz in clouds().items():
        g2, target2 = graphs.compute_graph_nn_2(xyz, 10, 45)
        g1 = graphs.compute_graph_nn(xyz, 10)
        out[f'{tag}_xyz'] = xyz
        for k in ('source', 'target', 'distances'):
            out[f'{tag}_nn2_{k}'] = g2[k]
            out[f'{tag}_nn1_{k}'] = g1[k]
        out[f'{tag}_nn2_target2'] = target2
    # interpolate_labels (provider.py:681-687): labels of cloud a's first 800 points on jittered copies of cloud a
    rng = np.random.default_rng(12)
    xyz = out['a_xyz'][:800]
    hist = rng.integers(0, 5, size=(800, 6)).astype(np.uint32)
    labels = np.argmax(hist, axis=1)
    up = (out['a_xyz'] + rng.normal(scale=0.02, size=out['a_xyz'].shape)).astype(np.float32)
    nn = NearestNeighbors(n_neighbors=1, algorithm='kd_tree').fit(xyz)
    _, neighbor = nn.kneighbors(up)
    out['interp_xyz'], out['interp_up'], out['interp_hist'] = xyz, up, hist
    out['interp_labels'] = labels[neighbor].flatten()
    path = os.path.join(ROOT, 'tests', 'golden', 'knn_graph.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
