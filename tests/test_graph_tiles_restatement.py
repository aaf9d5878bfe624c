"""The numpy restatements of tests/graph_tiles_restatement.py against the reference's record tests/golden/graph_tiles.npz
(tools/gen_tiles_golden.py: graph_loader / graph_collate of supervized_partition/graph_processing.py): integers equal, floats bit
for bit.  No GPU."""
import os
import types

import numpy as np
import pytest

import graph_tiles_restatement as R
from conftest import GOLDEN

TAGS = ('eval_rgb', 'eval_norgb', 'train_a', 'train_b', 'train_c', 'train_norgb')
COLLATED = ('train_a', 'train_b', 'train_c')
SCENE_KEYS = ('xyz', 'rgb', 'edg_source', 'edg_target', 'is_transition', 'local_geometry', 'labels', 'objects', 'elevation', 'xyn')


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'graph_tiles.npz'))


def scene_of(rec, i):
    return {k: rec[f'scene{i}/{k}'] for k in SCENE_KEYS}


def restated(rec, tag):
    scene, train, use_rgb, max_ver, _ = (int(v) for v in rec[f'{tag}/meta'])
    args = types.SimpleNamespace(k_nn_local=int(rec['k_nn_local']), use_rgb=use_rgb, global_feat=str(rec['global_feat']), max_ver_train=max_ver)
    opt = lambda key: rec[f'{tag}/{key}'] if f'{tag}/{key}' in rec.files else None   # noqa: E731
    assert int(rec['rotation']) == 0, 'the record was made without the rotation; see tools/gen_tiles_golden.py'
    return R.loader(scene_of(rec, scene), bool(train), args, seeds=opt('seeds'), noise_xyz=opt('noise_xyz'), noise_rgb=opt('noise_rgb'))


def same(a, ref, what):
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if ref.dtype.kind == 'f':
        assert a.dtype == ref.dtype == np.float32, (what, a.dtype, ref.dtype)
        assert np.array_equal(a.view(np.uint32), ref.view(np.uint32)), f'{what}: not bit-equal ({int((a.view(np.uint32) != ref.view(np.uint32)).sum())} elements differ)'
    else:
        assert np.array_equal(a.astype(np.int64), ref.astype(np.int64)), what


@pytest.mark.parametrize('tag', TAGS)
def test_loader_restatement_equals_the_record(rec, tag):
    out = restated(rec, tag)
    for key in ('edg_source', 'edg_target', 'is_transition', 'labels', 'objects', 'clouds', 'clouds_global', 'xyz'):
        same(out[key], rec[f'{tag}/{key}'], f'{tag}/{key}')
    if 'selected_ver' in out:
        same(out['selected_ver'], rec[f'{tag}/selected_ver'], 'selected_ver')
        same(out['selected_edg'], rec[f'{tag}/selected_edg'], 'selected_edg')
        assert out['n_seen'] == int(rec[f'{tag}/n_seen']) and out['n_seeds_used'] == int(rec[f'{tag}/n_seeds_used'])
    assert np.array_equal(rec[f'{tag}/nei'], [0])


def test_collate_restatement_equals_the_record(rec):
    batch = R.collate([restated(rec, tag) for tag in COLLATED])
    for key, v in batch.items():
        same(v, rec[f'collate/{key}'], f'collate/{key}')
    assert np.array_equal(rec['collate/nei'], [[0], [0], [0]])


def test_the_record_is_not_degenerate(rec):
    assert (rec['eval_rgb/clouds_global'][:, 0] == 0).any(), 'some diameter is 0'
    zero = rec['eval_rgb/clouds_global'][:, 0] == 0
    assert not np.isnan(rec['eval_rgb/clouds']).any() and (rec['eval_rgb/clouds'][zero, :3] == 0).all()
    size = int(rec['train_a/meta'][3])
    assert int(rec['train_a/n_seen']) == size + 1 == int((rec['train_a/selected_ver'] != 0).sum()), 'size + 1 vertices'
    # a seed was skipped: three seeds consumed, the second one inside the component the first one exhausted
    assert int(rec['train_a/n_seeds_used']) == 3
    scene = scene_of(rec, int(rec['train_a/meta'][0]))
    first = R.random_subgraph(len(scene['xyz']), scene['edg_source'], scene['edg_target'], size, rec['train_a/seeds'][:1])
    assert first[2] < size and first[1][int(rec['train_a/seeds'][1])] == 1
    # a selected vertex whose neighbourhood reaches outside the selection
    sel = rec['train_a/selected_ver'] != 0
    assert (~sel[scene['local_geometry'][sel].astype(np.int64)]).any()
    # duplicate points
    assert len(np.unique(rec['scene0/xyz'], axis=0)) < len(rec['scene0/xyz'])
    # the object offsets are the cumulative max(), not max() + 1
    n = [len(rec[f'{t}/labels']) for t in COLLATED]
    mx = [int(rec[f'{t}/objects'].max()) for t in COLLATED]
    got = rec['collate/objects']
    assert np.array_equal(got[n[0]:n[0] + n[1]], rec['train_b/objects'] + mx[0])
    assert np.array_equal(got[n[0] + n[1]:], rec['train_c/objects'] + mx[0] + mx[1])
    assert not np.array_equal(got[n[0]:n[0] + n[1]], rec['train_b/objects'] + mx[0] + 1)
    # one sample of the batch is not subsampled
    assert len(rec['train_b/labels']) == len(rec['scene2/xyz'])
    # at scale 1e-3 the float32 and the float64 form of the denominator differ
    xyz = (rec['scene0/xyz'] * np.float32(1e-3)).astype(np.float32)
    clouds, diam = R.tiles(xyz, rec['scene0/local_geometry'], 20)
    c = xyz[rec['scene0/local_geometry'].astype(np.int64)]
    f64 = ((c - xyz[:, None, :]) / (diam[:, None, None].astype(np.float64) + 1e-10)).astype(np.float32).transpose(0, 2, 1)
    assert (f64 != clouds).any()


@pytest.mark.parametrize('k', [1, 2, 5, 20, 33])
def test_tiles_restatement_equals_numpy(k):
    """The explicit float32 sequence against the reference's numpy expression (graph_processing.py:393-396) itself."""
    rng = np.random.default_rng(k)
    for scale, offset in ((1e-3, 0), (1, 0), (30, 1000), (1e-3, 1000)):
        xyz = (rng.normal(size=(150, 3)) * scale + offset).astype(np.float32)
        nei = rng.integers(0, 150, size=(150, 40))
        nei[:10] = nei[:10, :1]                               # duplicate neighbours
        clouds, diam = R.tiles(xyz, nei, k)
        c = xyz[nei[:, :k]]
        d = np.sqrt(c.var(1).sum(1))
        ref = ((c - xyz[:, np.newaxis, :]) / (d[:, np.newaxis, np.newaxis] + 1e-10)).transpose([0, 2, 1])
        same(diam, d, 'diameters')
        same(clouds, ref, 'clouds')


def test_random_subgraph_restatement_overshoot():
    # path 0-1-2-3-4, seed 0, size 3: 0, 1, 2 selected; 2 is still queued and examines its first neighbour 1 (selected): 3 vertices
    src, tgt = np.arange(4), np.arange(1, 5)
    assert R.random_subgraph(5, src, tgt, 3, [0])[2] == 3
    # seed 2: 2 -> 1, 3 (size reached at the end of 2's list); 1 examines its first neighbour 0: unselected, taken: 4 vertices
    se, sv, seen, used, _ = R.random_subgraph(5, src, tgt, 3, [2])
    assert seen == 4 and sv.tolist() == [1, 1, 1, 1, 0] and se.tolist() == [1, 1, 1, 0]
    with pytest.raises(ValueError):
        R.random_subgraph(5, src, tgt, 6, [0])
    # exhaustion and continuation
    src2, tgt2 = np.array([0, 2]), np.array([1, 3])
    a = R.random_subgraph(4, src2, tgt2, 3, [0, 1])
    assert a[2] == 2 and a[3] == 2
    b = R.random_subgraph(4, src2, tgt2, 3, [3], state=a[4])
    assert b[2] == 4 and b[1].tolist() == [1, 1, 1, 1]
