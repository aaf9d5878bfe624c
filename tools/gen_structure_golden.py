"""Writes tests/golden/scene_structure.npz from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE): the per-file body of main() of supervized_partition/graph_processing.py, run
through main() itself on three synthetic scenes -- s3dis with voxel_width 0, s3dis pruned, vkitti pruned -- with --plane_model 0,
and graph_loader(train=False) for ver_value 'geof' and 'geofrgb' on the pruned s3dis scene.  The reference file is loaded at run
time (tools/gen_tiles_golden.py: load_reference, which stubs the modules this machine lacks); main() gets a temporary ROOT_PATH
with the folder names it insists on; the readers are replaced by functions that return the prepared arrays, libply_c.prune /
compute_geof / connected_comp by the numpy restatements of oracle/spg_partition_oracle.py and tests/edge_loss_restatement.py,
compute_graph_nn_2 by the brute-force order of tests/knn_restatement.py, write_structure by a capture and read_structure by
the captured arrays in the dtypes the file would have.
    python tools/gen_structure_golden.py"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import edge_loss_restatement as ELR  # noqa: E402
import knn_restatement as KR  # noqa: E402
from gen_edgeloss_golden import REF  # noqa: E402
from gen_tiles_golden import load_reference  # noqa: E402
from oracle import spg_partition_oracle as P  # noqa: E402

K_NN_LOCAL, K_NN_ADJ, N_LABELS, VOXEL = 20, 5, 13, 0.15
FIELDS = ('xyz', 'rgb', 'source', 'target', 'nei', 'is_transition', 'labels', 'objects', 'geof', 'elevation', 'xyn')
LOADER_FIELDS = ('edg_source', 'edg_target', 'is_transition', 'labels', 'objects', 'clouds', 'clouds_global', 'nei', 'xyz')


def make_raw(rng, n_main, n_twin, n_dup, n_col, n_island):
    """A slab; twins (a second point 4 mm from a slab point, of another object and label: histogram ties after pruning); a block of
    identical points of object 0 (its voxel: an all-zero row of objects[:, 1:]); a column of constant xy beside the slab (collinear
    neighbourhoods); an island far away."""
    main = (rng.uniform(0, 3, size=(n_main, 3)) * [1, 1, 0.3]).astype(np.float32)
    twin = main[:n_twin] + np.float32(0.004)
    dup = np.tile(np.float32([1.5, 2.25, 0.5]), (n_dup, 1))
    col = np.stack([np.full(n_col, 3.75), np.full(n_col, 1.25), np.linspace(0.05, 0.85, n_col)], 1).astype(np.float32)
    island = (rng.uniform(0, 0.5, size=(n_island, 3)) + [40, 40, 0]).astype(np.float32)
    xyz = np.concatenate([main, twin, dup, col, island]).astype(np.float32)
    obj_main = (1 + np.floor(main[:, 0]) * 3 + np.floor(np.minimum(main[:, 1], 2.99))).astype(np.uint32)
    objects = np.concatenate([obj_main, obj_main[:n_twin] % 9 + 1, np.zeros(n_dup, np.uint32), np.full(n_col, 10, np.uint32),
                              np.full(n_island, 11, np.uint32)]).astype(np.uint32)
    labels = (objects % N_LABELS).astype(np.uint8)
    labels[n_main:n_main + n_twin] = (labels[:n_twin] + 5) % (N_LABELS + 1)        # (the upper-bound label is counted too)
    rgb = rng.integers(0, 256, size=(len(xyz), 3)).astype(np.uint8)
    return dict(xyz=xyz, rgb=rgb, labels=labels, objects=objects)


def graph_nn_2(xyz, k1, k2, voronoi=0.0):
    assert voronoi == 0
    idx, d2 = KR.knn(xyz, k2)
    n = len(xyz)
    graph = {'is_nn': True, 'source': np.repeat(np.arange(n), k1).astype(np.uint32), 'target': idx[:, :k1].reshape(-1).astype(np.uint32),
             'distances': KR.dist32(d2[:, :k1]).reshape(-1)}
    return graph, idx.reshape(-1).astype(np.uint32)


def as_read_back(c, read_geof):
    """The captured arguments of write_structure after the file's dtypes and read_structure's casts."""
    labels = np.asarray(c['labels'])
    labels = labels.astype(np.int32 if labels.ndim > 1 and labels.shape[1] > 1 else np.uint8).squeeze()
    local = c['geof'].astype(np.float32) if read_geof else c['nei'].astype(np.uint32)
    return (c['xyz'].astype(np.float32), c['rgb'].astype(np.float32), c['source'].astype(int).squeeze(), c['target'].astype(int).squeeze(),
            c['is_transition'].astype(np.uint8), local, labels, c['objects'].astype(np.uint32), c['elevation'].astype(np.float32),
            c['xyn'].astype(np.float32))


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    G, _ = load_reference()
    lib = types.SimpleNamespace()
    pruned = {}

    def prune(xyz, voxel, rgb, labels, objects, n_labels, n_objects):
        r = P.prune(xyz, voxel, rgb, labels, objects, n_labels, n_objects)
        pruned['hist'] = r[3]
        return r
    lib.prune = prune
    lib.compute_geof = lambda xyz, target, k: P.geof(xyz, target, k)
    lib.connected_comp = lambda n, src, tgt, active, cutoff: (None, ELR.components(n, src.astype(np.int64), tgt.astype(np.int64), active)[0].astype(np.uint32))
    G.libply_c = lib
    G.compute_graph_nn_2 = graph_nn_2
    captured = {}

    def write_structure(file_name, xyz, rgb, graph_nn, target_local_geometry, is_transition, labels, objects, geof, elevation, xyn):
        captured.update(xyz=xyz, rgb=rgb, source=graph_nn['source'], target=graph_nn['target'], nei=target_local_geometry,
                        is_transition=is_transition, labels=labels, objects=objects, geof=geof, elevation=elevation, xyn=xyn)
    G.write_structure = write_structure

    rng = np.random.default_rng(47)
    raws = [make_raw(rng, 300, 20, 25, 20, 30), make_raw(rng, 1200, 60, 25, 40, 120), make_raw(rng, 1100, 60, 25, 40, 100)]
    plans = [('s3dis', 0.0), ('s3dis', VOXEL), ('vkitti', VOXEL)]
    out = {'k_nn_local': np.int32(K_NN_LOCAL), 'k_nn_adj': np.int32(K_NN_ADJ), 'n_labels': np.int32(N_LABELS),
           'datasets': np.array([p[0] for p in plans]), 'voxel_width': np.array([p[1] for p in plans])}
    records = []
    for i, (raw, (dataset, voxel)) in enumerate(zip(raws, plans)):
        G.read_s3dis_format = lambda f, raw=raw: (raw['xyz'].copy(), raw['rgb'].copy(), raw['labels'].copy(), raw['objects'].copy())
        G.read_vkitti_format = lambda f, raw=raw: (raw['xyz'].copy(), raw['rgb'].copy(), raw['labels'].copy())
        captured.clear(), pruned.clear()
        with tempfile.TemporaryDirectory() as root:
            folders = ['Area_%d' % a for a in range(1, 7)] if dataset == 's3dis' else ['0%d' % a for a in range(1, 7)]
            for f in folders:
                os.makedirs(os.path.join(root, 'data', f))
            if dataset == 's3dis':
                os.makedirs(os.path.join(root, 'data', folders[0], 'room'))
            else:
                open(os.path.join(root, 'data', folders[0], 'scene.npy'), 'w').close()
            argv = sys.argv
            sys.argv = ['graph_processing.py', '--ROOT_PATH', root, '--dataset', dataset, '--k_nn_local', str(K_NN_LOCAL), '--k_nn_adj',
                        str(K_NN_ADJ), '--voxel_width', str(voxel), '--plane_model', '0', '--compute_geof', '1']
            try:
                G.main()
            finally:
                sys.argv = argv
        assert captured, 'main() wrote no structure'
        rec = {k: np.asarray(v).copy() for k, v in captured.items()}
        records.append(rec)
        for k in ('xyz', 'rgb', 'labels', 'objects'):
            out[f'scene{i}/raw_{k}'] = raw[k]
        for k in FIELDS:
            out[f'scene{i}/{k}'] = rec[k]
        if dataset == 's3dis' and voxel > 0:
            out[f'scene{i}/objects_hist'] = pruned['hist']

    # ---- graph_loader with the hand-crafted vertex values, on the pruned s3dis scene ----
    for ver_value in ('geof', 'geofrgb'):
        G.read_structure = lambda entry, read_geof: tuple(np.array(a) for a in as_read_back(records[1], read_geof))
        args = types.SimpleNamespace(ver_value=ver_value, learned_embeddings=0, k_nn_local=K_NN_LOCAL, use_rgb=1, global_feat='eXYrgb',
                                     max_ver_train=0, pc_augm_rot=0, pc_augm_jitter=0)
        sample = G.graph_loader('db/Area_1/room.h5', False, args, 'db')
        out[f'loader_{ver_value}/short_name'] = np.array(sample[0])
        for k, v in zip(LOADER_FIELDS, sample[1:]):
            out[f'loader_{ver_value}/{k}'] = v.numpy() if hasattr(v, 'numpy') else np.asarray(v)

    # ---- the record is not degenerate ----
    h = out['scene1/objects_hist']
    top = h[:, 1:].max(1)
    assert ((h[:, 1:] == top[:, None]).sum(1) > 1)[top > 0].any(), 'no tie in an object histogram'
    assert (top == 0).any(), 'no all-zero row of objects[:, 1:]'
    lab = out['scene2/labels']
    assert ((lab == lab.max(1, keepdims=True)).sum(1) > 1).any(), 'no tie in a label histogram'
    for i, rec in enumerate(records):
        n = len(rec['xyz'])
        far = rec['xyz'][:, 0] > 20
        assert far.any() and not far[rec['target'].astype(np.int64)[~far[rec['source'].astype(np.int64)]]].any(), 'the island is not separate'
        assert rec['is_transition'].any() and not rec['is_transition'].all()
        assert np.isnan(rec['geof']).any() == (i == 0), 'the identical points survive only without pruning (their geof is NaN)'
        assert rec['nei'].shape == (n, K_NN_LOCAL) and n > K_NN_LOCAL
    assert len(np.unique(out['scene2/objects'])) > 3 and out['scene2/objects'].max() + 1 == len(np.unique(out['scene2/objects']))
    assert out['loader_geofrgb/clouds'].shape[1] == 7 and out['loader_geof/clouds'].shape[1] == 4
    path = os.path.join(ROOT, 'tests', 'golden', 'scene_structure.npz')
    np.savez_compressed(path, **out)
    print('vertices', [len(r['xyz']) for r in records], '; components of the vkitti scene', int(out['scene2/objects'].max()) + 1,
          '; all-zero object rows', int((top == 0).sum()))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
