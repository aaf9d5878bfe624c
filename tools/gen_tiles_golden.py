"""Writes tests/golden/graph_tiles.npz from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE): graph_loader and graph_collate of supervized_partition/graph_processing.py
on three synthetic scenes of a few hundred vertices, k_nn_local = 20, global_feat = 'eXYrgb', use_rgb 1 and 0.  The reference
file is loaded at run time; the modules it imports and this machine may lack (h5py, transforms3d, igraph, torchnet, sklearn,
plyfile, libply_c, libcp, learning.spg, partition.*) are stubbed, read_structure is replaced by an in-memory one, and
libply_c.random_subgraph -- whose seeds come from an unseeded rand() and which needs Boost -- by the restatement of
tests/graph_tiles_restatement.py with fixed seeds.  The rotation is on only if transforms3d imports; `rotation` records it.
    python tools/gen_tiles_golden.py"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import graph_tiles_restatement as R  # noqa: E402
from gen_edgeloss_golden import REF  # noqa: E402
from gen_parteval_golden import _Stub  # noqa: E402

K_NN_LOCAL, K_NN_ADJ, N_CLASSES, GLOBAL_FEAT = 20, 5, 8, 'eXYrgb'
SIGMA, CLIP = 0.002, 0.005                       # graph_processing.py:542
FIELDS = ('edg_source', 'edg_target', 'is_transition', 'labels', 'objects', 'clouds', 'clouds_global', 'nei', 'xyz')


def load_reference():
    try:
        importlib.import_module('transforms3d')
        rotation = True
    except ImportError:
        rotation = False
    for m in ('h5py', 'transforms3d', 'igraph', 'torchnet', 'sklearn', 'sklearn.linear_model', 'plyfile', 'libcp', 'learning', 'learning.spg',
              'partition', 'partition.ply_c', 'partition.ply_c.libply_c', 'partition.graphs', 'partition.provider'):
        if m == 'transforms3d' and rotation:
            continue
        try:
            if m.split('.')[0] in ('learning', 'partition', 'libcp'):
                raise ImportError
            importlib.import_module(m)
        except ImportError:
            sys.modules[m] = _Stub(m)
    path_before = list(sys.path)
    spec = importlib.util.spec_from_file_location('ref_graph_processing', os.path.join(REF, 'supervized_partition', 'graph_processing.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path[:] = path_before
    return mod, rotation


def knn_brute(xyz, k):
    d = ((xyz[:, None, :].astype(np.float64) - xyz[None, :, :].astype(np.float64)) ** 2).sum(2)
    return np.argsort(d, axis=1, kind='stable')[:, :k]


def make_scene(rng, n_main, n_island, n_dup):
    """A slab of n_main points, an island of n_island points far away (its adjacency stays inside: a component of its own) and n_dup
    copies of one point with dyadic coordinates (their neighbourhoods are all-identical: diameter exactly 0)."""
    main = rng.uniform(0, 3, size=(n_main, 3)).astype(np.float32) * np.float32([1, 1, 0.3])
    island = (rng.uniform(0, 0.5, size=(n_island, 3)) + [40, 40, 0]).astype(np.float32)
    dup = np.tile(np.float32([1.5, 2.25, 0.5]), (n_dup, 1))
    xyz = np.concatenate([main, dup, island]).astype(np.float32)
    n = len(xyz)
    nb = knn_brute(xyz, K_NN_LOCAL + 1)
    local = nb[:, :K_NN_LOCAL].astype(np.uint32)                       # the point itself first, as compute_graph_nn_2 stores it
    src = np.repeat(np.arange(n), K_NN_ADJ).astype(np.int64)
    tgt = nb[:, 1:K_NN_ADJ + 1].reshape(-1).astype(np.int64)
    objects = (1 + np.floor(xyz[:, 0]) * 3 + np.floor(np.minimum(xyz[:, 1], 2.99))).astype(np.uint32)
    objects[n_main + n_dup:] = objects[:n_main].max() + 1
    labels = np.zeros((n, 1 + N_CLASSES), np.int32)
    labels[np.arange(n), 1 + objects % N_CLASSES] = rng.integers(1, 5, n)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.float32)
    elevation = (xyz[:, 2] - xyz[:, 2].min()).astype(np.float32)
    ma, mi = xyz[:, :2].max(0, keepdims=True), xyz[:, :2].min(0, keepdims=True)
    xyn = ((xyz[:, :2] - mi) / (ma - mi + 1e-8)).astype(np.float32)
    return dict(xyz=xyz, rgb=rgb, edg_source=src, edg_target=tgt, is_transition=(objects[src] != objects[tgt]).astype(np.uint8),
                local_geometry=local, labels=labels, objects=objects, elevation=elevation, xyn=xyn)


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    G, rotation = load_reference()
    rng = np.random.default_rng(31)
    scenes = [make_scene(rng, 170, 24, 24), make_scene(rng, 150, 30, 0), make_scene(rng, 140, 0, 0)]
    names = ['db/Area_1/room_a.h5', 'db/Area_1/room_b.h5', 'db/Area_2/room_c.h5']
    by_name = dict(zip(names, scenes))
    keys = ('xyz', 'rgb', 'edg_source', 'edg_target', 'is_transition', 'local_geometry', 'labels', 'objects', 'elevation', 'xyn')
    G.read_structure = lambda entry, read_geof: tuple(by_name[entry][k].copy() for k in keys)
    out = {'rotation': np.uint8(rotation), 'k_nn_local': np.int32(K_NN_LOCAL), 'global_feat': np.array(GLOBAL_FEAT), 'names': np.array(names)}
    for i, s in enumerate(scenes):
        for k in keys:
            out[f'scene{i}/{k}'] = s[k]
    seeds_now = []

    def random_subgraph(n_ver, src, tgt, size):
        se, sv, seen, used, _ = R.random_subgraph(n_ver, src.astype(np.int64), tgt.astype(np.int64), size, seeds_now)
        assert seen >= size, 'the seeds ran out'
        random_subgraph.last = (se, sv, seen, used)
        return se, sv
    sys.modules['partition.ply_c.libply_c'].random_subgraph = random_subgraph
    G.libply_c = sys.modules['partition.ply_c.libply_c']

    def run(tag, scene, train, use_rgb, max_ver, seeds=(), np_seed=0):
        args = types.SimpleNamespace(ver_value='ptn', learned_embeddings=1, k_nn_local=K_NN_LOCAL, use_rgb=use_rgb, global_feat=GLOBAL_FEAT,
                                     max_ver_train=max_ver, pc_augm_rot=int(rotation), pc_augm_jitter=1)
        seeds_now[:] = list(seeds)
        np.random.seed(np_seed)
        sample = G.graph_loader(names[scene], train, args, 'db')
        out[f'{tag}/meta'] = np.array([scene, int(train), use_rgb, max_ver, np_seed], np.int64)
        out[f'{tag}/short_name'] = np.array(sample[0])
        for k, v in zip(FIELDS, sample[1:]):
            out[f'{tag}/{k}'] = v.numpy() if hasattr(v, 'numpy') else np.asarray(v)
        if train:
            n = len(scenes[scene]['xyz'])
            np.random.seed(np_seed)                       # the same draws again, in augment_cloud_whole's order
            if rotation:
                import math
                import transforms3d
                out[f'{tag}/ref_index'] = np.int64(np.random.randint(n))
                out[f'{tag}/M'] = transforms3d.axangles.axangle2mat([0, 0, 1], np.random.uniform(0, 2 * math.pi)).astype('f4')
            out[f'{tag}/noise_xyz'] = np.clip(SIGMA * np.random.standard_normal((n, 3)), -CLIP, CLIP).astype(np.float32)
            if use_rgb:
                out[f'{tag}/noise_rgb'] = np.clip(SIGMA * np.random.standard_normal((n, 3)), -CLIP, CLIP).astype(np.float32)
            out[f'{tag}/seeds'] = np.array(list(seeds), np.int64)
            if 0 < max_ver < n:
                se, sv, seen, used = random_subgraph.last
                out[f'{tag}/selected_edg'], out[f'{tag}/selected_ver'] = se, sv
                out[f'{tag}/n_seen'], out[f'{tag}/n_seeds_used'] = np.int64(seen), np.int64(used)
        return sample

    run('eval_rgb', 0, False, 1, 0)
    run('eval_norgb', 0, False, 0, 0)
    n1 = len(scenes[1]['xyz'])
    island1 = 150                                          # first vertex of scene 1's island (30 vertices, a component of its own)
    s_a = run('train_a', 1, True, 1, 100, seeds=[island1 + 3, island1 + 7, 5, 9, 11], np_seed=101)
    s_b = run('train_b', 2, True, 1, 0, np_seed=102)       # max_ver_train = 0: no subsampling
    s_c = run('train_c', 0, True, 1, 80, seeds=[12, 40, 41], np_seed=103)
    run('train_norgb', 0, True, 0, 90, seeds=[100, 3], np_seed=104)
    batch = G.graph_collate([s_a, s_b, s_c])
    out['collate/short_name'] = np.array(batch[0])
    clouds, clouds_global, nei = batch[6]
    for k, v in zip(('edg_source', 'edg_target', 'is_transition', 'labels', 'objects'), batch[1:6]):
        out[f'collate/{k}'] = v.numpy() if hasattr(v, 'numpy') else np.asarray(v)
    out['collate/clouds'], out['collate/clouds_global'], out['collate/nei'], out['collate/xyz'] = clouds.numpy(), clouds_global.numpy(), np.asarray(nei), batch[7]
    # ---- the record is not degenerate ----
    assert (out['eval_rgb/clouds_global'][:, 0] == 0).any(), 'no diameter is 0'
    assert int(out['train_a/n_seen']) == 101 and int(out['train_c/n_seen']) == 81, 'no sample holds size + 1 vertices'
    assert int(out['train_a/n_seeds_used']) == 3, 'the island must be exhausted, its second seed skipped and a third one used'
    sel = out['train_a/selected_ver'] != 0
    reach = ~sel[scenes[1]['local_geometry'][sel].astype(np.int64)]
    assert reach.any(), 'no selected neighbourhood reaches outside the selection'
    assert n1 == len(sel) and sel[island1:].all()
    sizes = [len(s[4]) for s in (s_a, s_b, s_c)]
    maxes = [int(s[5].max()) for s in (s_a, s_b, s_c)]
    assert np.array_equal(out['collate/objects'][sizes[0]:sizes[0] + sizes[1]], s_b[5].numpy() + maxes[0]), 'object offsets are not the cumulative max()'
    path = os.path.join(ROOT, 'tests', 'golden', 'graph_tiles.npz')
    np.savez_compressed(path, **out)
    print('rotation', rotation, '; vertices', [len(s['xyz']) for s in scenes], '; zero diameters', int((out['eval_rgb/clouds_global'][:, 0] == 0).sum()),
          '; train_a n_seen', int(out['train_a/n_seen']), 'seeds used', int(out['train_a/n_seeds_used']), '; neighbours outside the selection', int(reach.sum()))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
