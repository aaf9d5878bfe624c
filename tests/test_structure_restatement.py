"""CPU: the numpy restatement of the scene structure (tests/structure_restatement.py) against the record of the reference's
main() and graph_loader (tests/golden/scene_structure.npz, tools/gen_structure_golden.py): integers equal, floats bit for bit.
And what of the feature needs no device: the model of the hand-crafted vertex values, spatialEmbedder, the refusals of
build_structure that are decided before anything is uploaded, the stores handing geof through."""
import os
import types

import numpy as np
import pytest
import torch

import structure_restatement as R
from conftest import GOLDEN

INT_FIELDS = {'source': 'edg_source', 'target': 'edg_target', 'nei': 'nei', 'is_transition': 'is_transition', 'objects': 'objects',
              'rgb': 'rgb', 'labels': 'labels'}
FLOAT_FIELDS = ('xyz', 'elevation', 'xyn', 'geof')


@pytest.fixture(scope='module')
def record():
    return np.load(os.path.join(GOLDEN, 'scene_structure.npz'))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_restatement_equals_the_record(record, i):
    g = record
    dataset, voxel = str(g['datasets'][i]), float(g['voxel_width'][i])
    mine = R.build(g[f'scene{i}/raw_xyz'], g[f'scene{i}/raw_rgb'], g[f'scene{i}/raw_labels'], g[f'scene{i}/raw_objects'], dataset,
                   int(g['n_labels']), voxel, int(g['k_nn_local']), int(g['k_nn_adj']))
    for theirs, ours in INT_FIELDS.items():
        ref = g[f'scene{i}/{theirs}']
        assert np.array_equal(np.asarray(mine[ours]).reshape(ref.shape).astype(np.int64), ref.astype(np.int64)), (i, theirs)
    for k in FLOAT_FIELDS:
        ref = g[f'scene{i}/{k}']
        assert ref.dtype == np.float32 and mine[k].shape == ref.shape and np.array_equal(bits(mine[k]), bits(ref)), (i, k)
    if dataset == 's3dis' and voxel > 0:
        assert np.array_equal(R.hard_ids(g[f'scene{i}/objects_hist'], 'objects'), g[f'scene{i}/objects'].astype(np.int64))


def test_record_holds_the_cases_it_claims(record):
    g = record
    h = g['scene1/objects_hist']
    top = h[:, 1:].max(1)
    assert (top == 0).any() and (((h[:, 1:] == top[:, None]).sum(1) > 1) & (top > 0)).any()          # an all-zero row, ties
    lab = g['scene2/labels']
    assert ((lab == lab.max(1, keepdims=True)).sum(1) > 1).any()
    x0 = g['scene0/xyz']
    assert (np.unique(x0, axis=0, return_counts=True)[1] > int(g['k_nn_local'])).any()                  # the identical points
    assert np.isnan(g['scene0/geof']).any()
    for i in range(3):
        xyz, src, tgt = g[f'scene{i}/xyz'], g[f'scene{i}/source'].astype(np.int64), g[f'scene{i}/target'].astype(np.int64)
        far = xyz[:, 0] > 20
        assert far.any() and (far[src] == far[tgt]).all()                                               # the island
        col = (xyz[:, 0] == np.float32(3.75)) & (xyz[:, 1] == np.float32(1.25))
        assert col.sum() >= 5                                                                           # the constant-xy column
        assert 300 <= len(xyz) <= 1500
    assert g['scene2/objects'].max() + 1 == len(np.unique(g['scene2/objects'])) > 3


def test_hard_ids_known_answers():
    h = np.array([[9, 0, 0, 0], [0, 0, 0, 0], [1, 2, 2, 0], [0, 0, 3, 3], [5, 1, 0, 7]])
    assert R.hard_ids(h, 'objects').tolist() == [1, 1, 1, 2, 3]
    assert R.hard_ids(h, 'labels').tolist() == [0, 0, 1, 2, 3]


def test_loader_clouds_equal_the_record(record):
    g = record
    for v, width in (('geof', 4), ('geofrgb', 7)):
        ref = g[f'loader_{v}/clouds']
        mine = R.clouds(g['scene1/geof'], g['scene1/rgb'], v)
        assert ref.dtype == np.float32 and ref.shape == (len(g['scene1/xyz']), width) and np.array_equal(bits(mine), bits(ref))
        assert g[f'loader_{v}/clouds_global'].tolist() == [0] and g[f'loader_{v}/nei'].tolist() == [0]
        assert np.array_equal(g[f'loader_{v}/objects'], g['scene1/objects'].astype(np.int64))


# ---- the parts of the feature that need no device ----
def test_create_model_of_the_hand_crafted_values():
    from superpoint_graph_amd.supervized_partition.supervized_partition import create_model
    for v in ('geof', 'geofrgb'):
        model = create_model(types.SimpleNamespace(ver_value=v, learned_embeddings=0, cuda=0))
        params = list(model.named_parameters())
        assert [k for k, _ in params] == ['placeholder'] and params[0][1].shape == () and not hasattr(model, 'ptn')
        model.load_state_dict({'placeholder': torch.tensor(0.25)}, strict=True)        # a reference checkpoint of such a model
        assert model.placeholder.item() == 0.25


def test_spatial_embedder_returns_its_clouds():
    from superpoint_graph_amd.supervized_partition.graph_processing import spatialEmbedder
    clouds = torch.arange(8.0).reshape(2, 4)
    assert spatialEmbedder(types.SimpleNamespace(cuda=0)).run_batch(None, clouds, torch.tensor([0]), None) is clouds


def test_build_structure_refusals_name_their_reason():
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition.graph_processing import STRUCTURE_DEFAULTS, build_structure
    assert STRUCTURE_DEFAULTS == dict(k_nn_local=20, k_nn_adj=5, voxel_width=0.03, compute_geof=1, plane_model=1, use_voronoi=0.0)
    xyz, rgb, lab, obj = np.zeros((30, 3), np.float32), np.zeros((30, 3), np.uint8), np.zeros(30, np.uint8), np.zeros(30, np.uint32)
    ns = types.SimpleNamespace
    with pytest.raises(NotImplementedError, match='cutpursuit2'):
        build_structure(xyz, rgb, lab, None, ns(plane_model=0), 'sema3d', 8)
    with pytest.raises(NotImplementedError, match='qhull'):
        build_structure(xyz, rgb, lab, obj, ns(plane_model=0, use_voronoi=0.5), 's3dis', 13)
    with pytest.raises(NotImplementedError, match='RANSAC'):
        build_structure(xyz, rgb, lab, obj, ns(), 's3dis', 13)                                        # plane_model defaults to 1
    with pytest.raises(NotImplementedError, match='KNN_MAX_K'):
        build_structure(xyz, rgb, lab, obj, ns(plane_model=0, k_nn_local=ops.KNN_MAX_K + 1), 's3dis', 13)
    with pytest.raises(ValueError, match='unknown data set'):
        build_structure(xyz, rgb, lab, obj, ns(plane_model=0), 'custom_dataset', 10)


def test_memory_store_hands_geof_through():
    from superpoint_graph_amd.supervized_partition.graph_processing import STRUCTURE_KEYS, MemorySceneStore
    scene = {k: np.full(2, i) for i, k in enumerate(STRUCTURE_KEYS)}
    scene['geof'] = np.full((2, 4), 0.5, np.float32)
    store = MemorySceneStore({'a': scene, 'b': tuple(scene[k] for k in STRUCTURE_KEYS)})
    assert store.read_structure('a', True)[5] is scene['geof'] and store.read_structure('a', False)[5] is scene['local_geometry']
    assert all(x is scene[k] for x, k in zip(store.read_structure('a', True), STRUCTURE_KEYS) if k != 'local_geometry')
    with pytest.raises(KeyError, match='geof'):
        store.read_structure('b', True)
