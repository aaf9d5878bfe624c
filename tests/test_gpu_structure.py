"""GPU: the scene structure of the learned partition made on the device (csrc/spg_structure.hip through ops.scene_structure;
supervized_partition.graph_processing.build_structure, DeviceScene.from_device, structure_arrays, the 'geof' / 'geofrgb' vertex
values) against the record of the reference's main() and graph_loader (tests/golden/scene_structure.npz) and the numpy
restatement of tests/structure_restatement.py (itself checked against that record on the CPU).

Integers equal; elevation, xyn, rgb / 255 and the doubled geof column bit for bit -- with one exception: the SIGN of a zero is
not compared (`same` below).  np.min over values that hold both -0.0 and +0.0 may return either, so `x - min` can be -0.0 or
+0.0 on either side; the values are compared with == there and bit for bit everywhere else.
geof itself stays judged by its restatement (oracle.spg_partition_oracle.geof, float64) within partition_cases.GEOF_ATOL on the
comparable entries, as tests/test_gpu_partition_edges.py judges ops.compute_geof; prune is compared exactly, as it is there."""
import os
import types

import numpy as np
import pytest
import torch

import partition_cases as C
import structure_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NS = types.SimpleNamespace


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(a, ref, what):
    """integers equal; float32 bit for bit, zeros of either sign alike, NaN where the reference has NaN."""
    a, ref = host(a) if torch.is_tensor(a) else np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if ref.dtype.kind == 'f':
        assert a.dtype == ref.dtype == np.float32, (what, a.dtype, ref.dtype)
        ok = (a.view(np.uint32) == ref.view(np.uint32)) | ((a == 0) & (ref == 0)) | (np.isnan(a) & np.isnan(ref))
        assert ok.all(), f'{what}: {int((~ok).sum())} of {ok.size} elements differ, first at {np.argwhere(~ok)[0].tolist()}'
    else:
        assert np.array_equal(a.astype(np.int64), ref.astype(np.int64)), what


def geof_within_bound(geof_doubled, xyz, nei, k, what):
    """the scene's geof (column 3 doubled) against the float64 restatement, by the measure of tests/partition_cases.py"""
    g = np.array(geof_doubled, dtype=np.float32)
    g[:, 3] = g[:, 3] / np.float32(2)                                     # (exact)
    m = C.geof_measure(g, dict(xyz=xyz, target=np.asarray(nei).reshape(-1), k_nn=k))
    print(what, 'geof worst', m['worst'], 'masked', m['masked'], 'nan rows', m['nan_rows'])
    assert m['nan_equal'] and (m['worst'] <= C.GEOF_ATOL).all(), (what, m)


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'scene_structure.npz'))


def ids_of(rec, i):
    """(id_mode, keyword arguments) of ops.scene_structure for the recorded arrays of scene i"""
    if str(rec['datasets'][i]) == 'vkitti':
        return 'labels', dict(hist=dev(rec[f'scene{i}/labels'].astype(np.int32)))
    if float(rec['voxel_width'][i]) > 0:
        return 'objects', dict(hist=dev(rec[f'scene{i}/objects_hist'].astype(np.int32)))
    return 'given', dict(ids=dev(rec[f'scene{i}/objects'].astype(np.int32)))


# ----------------------------------------------------------------------------------------------------------------------
# 1. ops.scene_structure on the recorded (pruned) arrays against the record
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 1, 2])
def test_scene_structure_against_the_record(hip, rec, i):
    from superpoint_graph_amd import ops
    k_local, k_adj = int(rec['k_nn_local']), int(rec['k_nn_adj'])
    xyz = dev(rec[f'scene{i}/xyz'])
    nei, _ = ops.knn(xyz, k_local, distances=False)
    geof_in = rec[f'scene{i}/geof'].copy()
    geof_in[:, 3] = geof_in[:, 3] / np.float32(2)                          # (exact: the record's column is a doubled float32)
    id_mode, kw = ids_of(rec, i)
    s = ops.scene_structure(xyz, nei, k_adj, id_mode=id_mode, geof=dev(geof_in), rgb=dev(rec[f'scene{i}/rgb'].astype(np.uint8)), **kw)
    assert all(torch.is_tensor(s[k]) and s[k].is_cuda for k in ('edg_source', 'edg_target', 'nei', 'is_transition', 'hard_ids', 'objects',
                                                                 'elevation', 'xyn', 'geof', 'rgb'))
    assert s['edg_source'].dtype == s['edg_target'].dtype == s['objects'].dtype == torch.int64 and s['is_transition'].dtype == torch.uint8
    for mine, theirs in (('edg_source', 'source'), ('edg_target', 'target'), ('nei', 'nei'), ('is_transition', 'is_transition'),
                         ('objects', 'objects'), ('elevation', 'elevation'), ('xyn', 'xyn'), ('geof', 'geof')):
        same(s[mine], rec[f'scene{i}/{theirs}'], f'scene{i}/{theirs}')          # (objects of the vkitti scene: the numbering too)
    same(s['rgb'], rec[f'scene{i}/rgb'].astype(np.float32) / np.float32(255), f'scene{i}/rgb')
    if id_mode == 'labels':
        same(s['hard_ids'], rec[f'scene{i}/labels'].argmax(1), 'hard labels')
        assert int(s['objects'].max()) + 1 == len(np.unique(rec[f'scene{i}/objects'])) > 3
    else:
        assert s['objects'] is s['hard_ids']
    assert s['graph'].E == len(xyz) * k_adj and s['nei'] is nei


# ----------------------------------------------------------------------------------------------------------------------
# 2. the smallest shapes at which the kernels can go wrong, against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def histogram(rng, n, C):
    """counts with ties (two equal maxima, the first must win), all-zero rows and rows that are zero from column 1 on"""
    h = rng.integers(0, 4, size=(n, C)).astype(np.int32)
    h[::5] = 0
    h[1::7, 1:] = 0
    h[1::7, 0] = 3
    t = np.arange(2, n, 3)
    h[t, rng.integers(0, C, len(t))] = 9
    h[t, rng.integers(0, C, len(t))] = 9
    return h


SHAPES = {
    'n22_labels_C14': dict(n=22, rule='labels', C=14),                     # n = k_nn_local + 2: every vertex sees all but one
    'n22_objects_C2': dict(n=22, rule='objects', C=2),                     # one column to choose from
    'n4099_objects_C70': dict(n=4099, rule='objects', C=70),               # 17 workgroups, ragged tail; more columns than a wave
    'n4099_labels_C3': dict(n=4099, rule='labels', C=3),                   # 4 lanes per row
    'n4099_given_offset': dict(n=4099, rule='given', offset=1e5),          # coordinates offset by 1e5
    'n300_flat_xy': dict(n=300, rule='given', flat=True),                  # xy extent exactly 0: xyn all 0
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_scene_structure_shapes(hip, name):
    from superpoint_graph_amd import ops
    c = SHAPES[name]
    n, k_local, k_adj = c['n'], 20, 5
    rng = np.random.default_rng(n + len(name))
    xyz = (rng.normal(size=(n, 3)) + c.get('offset', 0.0)).astype(np.float32)
    if c.get('flat'):
        xyz[:, :2] = np.float32([-1.25, 7.5])
    geof = rng.uniform(size=(n, 4)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    if c['rule'] == 'given':
        ids = rng.integers(0, 6, n).astype(np.int64 if c.get('flat') else np.int32)
        kw = dict(ids=dev(ids))
    else:
        ids = histogram(rng, n, c['C'])
        kw = dict(hist=dev(ids))
    nei, _ = ops.knn(dev(xyz), k_local, distances=False)
    s = ops.scene_structure(dev(xyz), nei, k_adj, id_mode=c['rule'], geof=dev(geof), rgb=dev(rgb), **kw)
    ref = R.structure(xyz, host(nei), k_adj, ids, c['rule'], geof)
    for k in ('edg_source', 'edg_target', 'is_transition', 'hard_ids', 'objects', 'elevation', 'xyn', 'geof'):
        same(s[k], ref[k], f'{name}/{k}')
    same(s['rgb'], rgb.astype(np.float32) / np.float32(255), f'{name}/rgb')
    if c.get('flat'):
        assert not host(s['xyn']).any()
    if c['rule'] != 'given':
        first = 1 if c['rule'] == 'objects' else 0
        zero = ~ids[:, first:].any(1)
        assert zero.any() and (host(s['hard_ids'])[zero] == first).all()


def test_scene_structure_refuses_nan_before_anything_else_is_launched(hip):
    from superpoint_graph_amd import ops
    rng = np.random.default_rng(5)
    xyz = rng.normal(size=(4099, 3)).astype(np.float32)
    nei, _ = ops.knn(dev(xyz), 20, distances=False)
    for bad in (np.nan, np.inf):
        x = xyz.copy()
        x[4098, 1] = bad                                                   # in the ragged tail of the last workgroup
        geof = torch.ones(4099, 4, device='cuda')
        with pytest.raises(ValueError, match='Input contains NaN or infinity.'):
            ops.scene_structure(dev(x), nei, 5, id_mode='given', ids=dev(np.zeros(4099, np.int32)), geof=geof)
        assert bool((geof == 1).all())                                     # the vertex pass (which doubles column 3) did not run
    with pytest.raises(IndexError, match='neighbour index'):
        wrong = nei.clone()
        wrong[7, 19] = 4099
        ops.scene_structure(dev(xyz), wrong, 5, id_mode='given', ids=dev(np.zeros(4099, np.int32)))
    with pytest.raises(ValueError, match='k_adj'):
        ops.scene_structure(dev(xyz), nei, 21, id_mode='given', ids=dev(np.zeros(4099, np.int32)))


# ----------------------------------------------------------------------------------------------------------------------
# 3. build_structure end to end
# ----------------------------------------------------------------------------------------------------------------------
def structure_args(rec, i):
    return NS(k_nn_local=int(rec['k_nn_local']), k_nn_adj=int(rec['k_nn_adj']), voxel_width=float(rec['voxel_width'][i]), compute_geof=1,
              plane_model=0, use_voronoi=0.0)


@pytest.fixture(scope='module')
def scenes(rec, hip):
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    return [GP.build_structure(rec[f'scene{i}/raw_xyz'], rec[f'scene{i}/raw_rgb'], rec[f'scene{i}/raw_labels'], rec[f'scene{i}/raw_objects'],
                               structure_args(rec, i), str(rec['datasets'][i]), int(rec['n_labels'])) for i in range(3)]


@pytest.mark.parametrize('i', [0, 1, 2])
def test_build_structure_against_the_record(rec, scenes, i):
    """voxel_width 0: field by field.  Pruned: integers equal, floats as exactly as tests/test_gpu_partition_edges.py asks of prune
    (equal), geof within its own bound."""
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    scene = scenes[i]
    assert isinstance(scene, GP.DeviceScene) and scene.n == len(rec[f'scene{i}/xyz'])
    arrays = GP.structure_arrays(scene)
    assert list(arrays) == ['xyz', 'rgb', 'elevation', 'xyn', 'edg_source', 'edg_target', 'is_transition', 'local_geometry', 'objects', 'geof',
                            'labels']
    dtypes = dict(xyz='float32', rgb='float32', elevation='float32', xyn='float32', edg_source='int64', edg_target='int64',
                  is_transition='uint8', local_geometry='uint32', objects='uint32', geof='float32',
                  labels='int32' if float(rec['voxel_width'][i]) > 0 else 'uint8')
    assert {k: str(v.dtype) for k, v in arrays.items()} == dtypes
    for mine, theirs in (('xyz', 'xyz'), ('edg_source', 'source'), ('edg_target', 'target'), ('is_transition', 'is_transition'),
                         ('local_geometry', 'nei'), ('objects', 'objects'), ('labels', 'labels'), ('elevation', 'elevation'), ('xyn', 'xyn')):
        same(arrays[mine], rec[f'scene{i}/{theirs}'], f'scene{i}/{theirs}')
    same(arrays['rgb'], rec[f'scene{i}/rgb'].astype(np.float32), f'scene{i}/rgb')
    same(scene.rgb, rec[f'scene{i}/rgb'].astype(np.float32) / np.float32(255), f'scene{i}/rgb / 255')
    geof_within_bound(arrays['geof'], rec[f'scene{i}/xyz'], rec[f'scene{i}/nei'], int(rec['k_nn_local']), f'scene{i}')


@pytest.mark.parametrize('i', [1, 2])
def test_build_structure_is_the_composition_of_the_ops(rec, scenes, i):
    from superpoint_graph_amd import ops
    vkitti = str(rec['datasets'][i]) == 'vkitti'
    n_labels, objects = int(rec['n_labels']), rec[f'scene{i}/raw_objects']
    xyz, rgb, labels, hist = ops.prune(dev(rec[f'scene{i}/raw_xyz']), float(np.float32(rec['voxel_width'][i])), dev(rec[f'scene{i}/raw_rgb']),
                                       dev(rec[f'scene{i}/raw_labels']), None if vkitti else dev(objects.astype(np.int32)), n_labels,
                                       0 if vkitti else int(objects.max()) + 1)
    nei, _ = ops.knn(xyz, int(rec['k_nn_local']), distances=False)
    geof = ops.compute_geof(xyz, nei.reshape(-1), int(rec['k_nn_local']))
    plain = geof.clone()
    s = ops.scene_structure(xyz, nei, int(rec['k_nn_adj']), id_mode='labels' if vkitti else 'objects', hist=labels if vkitti else hist,
                            geof=geof, rgb=rgb)
    assert s['geof'] is geof and torch.equal(geof[:, :3], plain[:, :3])
    assert torch.equal(geof[:, 3].view(torch.int32), (plain[:, 3] + plain[:, 3]).view(torch.int32))
    scene = scenes[i]
    for mine, theirs in ((scene.xyz, xyz), (scene.rgb, s['rgb']), (scene.nei, nei), (scene.edg_source, s['edg_source']),
                         (scene.edg_target, s['edg_target']), (scene.is_transition, s['is_transition']), (scene.labels, labels),
                         (scene.objects, s['objects']), (scene.elevation, s['elevation']), (scene.xyn, s['xyn']), (scene.geof, geof)):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape
        assert np.array_equal(host(mine).view(np.uint8), host(theirs).view(np.uint8))


def test_build_structure_refusals(rec, hip):
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    raw = [rec[f'scene0/raw_{k}'] for k in ('xyz', 'rgb', 'labels', 'objects')]
    with pytest.raises(ValueError, match='Expected n_neighbors <= n_samples, but n_samples = 20, n_neighbors = 21'):
        GP.build_structure(*[a[:20] for a in raw], NS(plane_model=0, voxel_width=0.0), 's3dis', 13)
    with pytest.raises(NotImplementedError, match='RANSAC'):
        GP.build_structure(*raw, NS(voxel_width=0.0), 's3dis', 13)
    # plane_model 1 with an elevation of the caller's: used as it is; sema3d with objects: the s3dis rule
    elevation = np.arange(len(raw[0]), dtype=np.float32)
    scene = GP.build_structure(*raw, NS(voxel_width=0.0, compute_geof=0), 'sema3d', 8, elevation=elevation)
    same(scene.elevation, elevation, 'elevation as given')
    same(scene.is_transition, rec['scene0/is_transition'], 'sema3d with objects')
    assert scene.geof is None and 'geof' not in GP.structure_arrays(scene)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the hand-crafted vertex values through graph_loader
# ----------------------------------------------------------------------------------------------------------------------
def loader_args(ver_value, **kw):
    a = dict(ver_value=ver_value, learned_embeddings=int('ptn' in ver_value), k_nn_local=20, use_rgb=1, global_feat='eXYrgb', max_ver_train=0,
             pc_augm_rot=0, pc_augm_jitter=0, cuda=1)
    a.update(kw)
    return NS(**a)


@pytest.mark.parametrize('as_arrays', [False, True], ids=['device_scene', 'host_arrays'])
@pytest.mark.parametrize('ver_value', ['geof', 'geofrgb'])
def test_graph_loader_hand_crafted_values(rec, scenes, ver_value, as_arrays):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    from superpoint_graph_amd.supervized_partition.supervized_partition import create_model
    scene, name = scenes[1], 'db/Area_1/room.h5'
    store = GP.MemorySceneStore({name: GP.structure_arrays(scene) if as_arrays else scene})
    sample = GP.graph_loader(name, False, loader_args(ver_value), 'db', store=store)
    tag = f'loader_{ver_value}'
    assert sample[0] == str(rec[f'{tag}/short_name'])
    for key, v in zip(('edg_source', 'edg_target', 'is_transition', 'labels', 'objects'), sample[1:6]):
        assert torch.is_tensor(v) and v.is_cuda, key
        same(v, rec[f'{tag}/{key}'], f'{tag}/{key}')
    clouds, clouds_global = sample[6], sample[7]
    assert clouds.is_cuda and clouds.dtype == torch.float32 and tuple(clouds.shape) == rec[f'{tag}/clouds'].shape
    geof = ops.compute_geof(scene.xyz, scene.nei.reshape(-1), 20)
    geof[:, 3] = geof[:, 3] + geof[:, 3]
    assert np.array_equal(host(clouds[:, :4]).view(np.uint32), host(geof).view(np.uint32))       # geof as ops.compute_geof makes it
    geof_within_bound(host(clouds[:, :4]), rec['scene1/xyz'], rec['scene1/nei'], 20, tag)       # ... which its restatement judges
    if ver_value == 'geofrgb':
        same(clouds[:, 4:].contiguous(), rec[f'{tag}/clouds'][:, 4:], f'{tag}/rgb')              # rgb / 255 bit for bit
    assert not clouds_global.is_cuda and clouds_global.dtype == torch.int64 and clouds_global.tolist() == [0]
    assert np.array_equal(sample[8], rec[f'{tag}/nei'])
    same(sample[9], rec[f'{tag}/xyz'], f'{tag}/xyz')
    model = create_model(loader_args(ver_value))
    assert [k for k, _ in model.named_parameters()] == ['placeholder'] and model.placeholder.is_cuda
    assert GP.spatialEmbedder(loader_args(ver_value)).run_batch(model, clouds, clouds_global) is clouds
    batch = GP.graph_collate([sample, sample])
    assert batch[6][0].shape == (2 * scene.n, clouds.shape[1]) and int(batch[1].max()) == 2 * scene.n - 1


def test_graph_loader_refuses_what_the_reference_leaves_undefined(scenes):
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    from superpoint_graph_amd.supervized_partition.supervized_partition import create_model
    name = 'db/Area_1/room.h5'
    store = GP.MemorySceneStore({name: scenes[1]})
    with pytest.raises(ValueError, match='does not select the rows of local_geometry'):
        GP.graph_loader(name, True, loader_args('geof', max_ver_train=100), 'db', store=store)
    for args in (loader_args('geof', learned_embeddings=1), loader_args('ptn', learned_embeddings=0)):
        with pytest.raises(NotImplementedError, match='learned_embeddings'):
            GP.graph_loader(name, False, args, 'db', store=store)
    with pytest.raises(NotImplementedError, match='geof'):
        create_model(loader_args('geofrgb', learned_embeddings=1))
    train = GP.graph_loader(name, True, loader_args('geofrgb', pc_augm_jitter=1), 'db', store=store, rng=np.random.RandomState(3))
    assert train[6].shape == (scenes[1].n, 7) and not torch.equal(train[9], scenes[1].xyz)       # train without subsampling: augmented
    no_geof = GP.build_structure(scenes[0].xyz, (scenes[0].rgb * 255).round().to(torch.uint8), scenes[0].labels, scenes[0].objects,
                                 NS(voxel_width=0.0, compute_geof=0, plane_model=0), 's3dis', 13)
    with pytest.raises(KeyError, match='geof'):
        GP.graph_loader(name, False, loader_args('geof'), 'db', store=GP.MemorySceneStore({name: no_geof}))


# ----------------------------------------------------------------------------------------------------------------------
# 5. the scene feeds what is there already: graph_loader ('ptn'), graph_collate, the contrastive loss
# ----------------------------------------------------------------------------------------------------------------------
def test_built_scene_feeds_the_learned_path(scenes):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    names = ['db/Area_1/a.h5', 'db/01/b.h5']
    store = GP.MemorySceneStore({names[0]: scenes[0], names[1]: scenes[2]})
    args = loader_args('ptn', max_ver_train=150, pc_augm_jitter=1)
    rng = np.random.RandomState(11)
    alone = GP.graph_loader(names[0], True, args, 'db', store=store, rng=rng)          # (label vectors and histograms do not collate)
    assert alone[6].shape == (len(alone[4]), 6, 20) and 150 <= len(alone[4]) <= 151 and bool(torch.isfinite(alone[6]).all())
    batch = GP.graph_collate([GP.graph_loader(names[1], True, args, 'db', store=store, rng=rng),
                              GP.graph_loader(names[1], False, args, 'db', store=store)])
    clouds, clouds_global, _ = batch[6]
    n = clouds.shape[0]
    assert clouds.shape == (n, 6, 20) and clouds_global.shape == (n, 7) and n == batch[7].shape[0] > scenes[2].n
    assert bool(torch.isfinite(clouds).all()) and bool(torch.isfinite(clouds_global).all())
    emb = torch.nn.functional.normalize(torch.randn(n, 4, device='cuda', generator=torch.Generator('cuda').manual_seed(1)))
    emb.requires_grad_(True)
    graph = ops.EdgeGraph(batch[1], batch[2], n)
    l1, l2, diff = ops.contrastive_edge_loss(emb, graph, batch[3], torch.ones(graph.E, device='cuda'))
    ((l1 + l2) / graph.E).backward()
    assert diff.shape == (graph.E,) and np.isfinite(float(l1.detach())) and np.isfinite(float(l2.detach())) and bool(torch.isfinite(emb.grad).all())
    assert 0 < int(batch[3].sum()) < graph.E


def test_frame_workspace_is_exactly_its_layout(hip):
    """the convention of csrc/spg_part.h: the reported size fits, one byte less is refused before anything is launched"""
    from superpoint_graph_amd import _lib
    n = 300000                                            # more workgroups than the first phase launches: grid-stride
    xyz = torch.randn(n, 3, device='cuda')
    xyz[n - 1] = torch.tensor([-9.0, 11.0, -13.0])
    frame, err = torch.full((5,), 7.0, device='cuda'), torch.ones(1, dtype=torch.int32, device='cuda')
    size = hip.spg_structure_frame_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device='cuda')
    args = (xyz.data_ptr(), n, frame.data_ptr(), err.data_ptr(), ws.data_ptr())
    assert hip.spg_structure_frame(*args, size - 1, torch.cuda.current_stream().cuda_stream) == -1
    assert b'workspace too small' in hip.spg_last_error() and frame.tolist() == [7.0] * 5 and err.item() == 1
    _lib.check(hip.spg_structure_frame(*args, size, torch.cuda.current_stream().cuda_stream), 'spg_structure_frame')
    x = xyz.cpu().numpy()
    want = [x[:, 2].min(), x[:, 0].min(), x[:, 1].min(), x[:, 0].max(), x[:, 1].max()]
    assert err.item() == 0 and frame.tolist() == [float(v) for v in want] and want[0] == -13.0 and want[4] == 11.0
