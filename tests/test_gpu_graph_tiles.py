"""Batches of the learned partition made on the device (csrc/spg_tiles.hip; ops.neighbourhood_tiles, ops.augment_whole,
ops.random_subgraph, ops.induced_subgraph; supervized_partition/graph_processing.py) against the reference's record
tests/golden/graph_tiles.npz and the numpy restatements of tests/graph_tiles_restatement.py (themselves checked against that
record on the CPU).  Floats bit for bit, integers equal; the rotation of augment_whole within the bound derived in
graph_tiles_restatement.augment_whole64."""
import os
import types

import numpy as np
import pytest
import torch

import graph_tiles_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SCENE_KEYS = ('xyz', 'rgb', 'edg_source', 'edg_target', 'is_transition', 'local_geometry', 'labels', 'objects', 'elevation', 'xyn')
TAGS = ('eval_rgb', 'eval_norgb', 'train_a', 'train_b', 'train_c', 'train_norgb')
COLLATED = ('train_a', 'train_b', 'train_c')
VPB = 32          # ops.TILES_VERTICES_PER_BLOCK


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(a, ref, what):
    a, ref = host(a) if torch.is_tensor(a) else np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if ref.dtype.kind == 'f':
        assert a.dtype == ref.dtype == np.float32, (what, a.dtype, ref.dtype)
        diff = a.view(np.uint32) != ref.view(np.uint32)
        assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} elements are not bit-equal, first at {np.argwhere(diff)[0].tolist()}'
    else:
        assert np.array_equal(a.astype(np.int64), ref.astype(np.int64)), what


# ----------------------------------------------------------------------------------------------------------------------
# 1. graph_loader / graph_collate against the reference's record
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'graph_tiles.npz'))


@pytest.fixture(scope='module')
def store(rec, hip):
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    return GP.MemorySceneStore({str(name): {k: rec[f'scene{i}/{k}'] for k in SCENE_KEYS} for i, name in enumerate(rec['names'])})


def load(rec, store, tag):
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    scene, train, use_rgb, max_ver, np_seed = (int(v) for v in rec[f'{tag}/meta'])
    assert int(rec['rotation']) == 0
    args = types.SimpleNamespace(ver_value='ptn', learned_embeddings=1, k_nn_local=int(rec['k_nn_local']), use_rgb=use_rgb,
                                 global_feat=str(rec['global_feat']), max_ver_train=max_ver, pc_augm_rot=0, pc_augm_jitter=1)
    seeds = rec[f'{tag}/seeds'] if f'{tag}/seeds' in rec.files and len(rec[f'{tag}/seeds']) else None
    return GP.graph_loader(str(rec['names'][scene]), bool(train), args, 'db', store=store, seeds=seeds, rng=np.random.RandomState(np_seed))


@pytest.mark.parametrize('tag', TAGS)
def test_graph_loader_against_the_record(rec, store, tag):
    sample = load(rec, store, tag)
    assert sample[0] == str(rec[f'{tag}/short_name'])
    for key, v in zip(('edg_source', 'edg_target', 'is_transition', 'labels', 'objects', 'clouds', 'clouds_global'), sample[1:8]):
        assert torch.is_tensor(v) and v.is_cuda, key
        same(v, rec[f'{tag}/{key}'], f'{tag}/{key}')
    assert isinstance(sample[8], np.ndarray) and np.array_equal(sample[8], rec[f'{tag}/nei'])
    same(sample[9], rec[f'{tag}/xyz'], f'{tag}/xyz')


def test_graph_collate_against_the_record_and_through_the_embedder(rec, store):
    from oracle import validate_against_reference as V
    from superpoint_graph_amd.learning import pointnet
    from superpoint_graph_amd.supervized_partition import graph_processing as GP
    from superpoint_graph_amd.supervized_partition import losses
    batch = GP.graph_collate([load(rec, store, tag) for tag in COLLATED])
    assert list(batch[0]) == [str(s) for s in rec['collate/short_name']]
    for key, v in zip(('edg_source', 'edg_target', 'is_transition', 'labels', 'objects'), batch[1:6]):
        same(v, rec[f'collate/{key}'], f'collate/{key}')
    clouds, clouds_global, nei = batch[6]
    same(clouds, rec['collate/clouds'], 'collate/clouds')
    same(clouds_global, rec['collate/clouds_global'], 'collate/clouds_global')
    assert np.array_equal(nei, rec['collate/nei'])
    same(batch[7], rec['collate/xyz'], 'collate/xyz')
    # the batch feeds the embedder and the loss unchanged
    gl = np.load(os.path.join(GOLDEN, 'local_embedder.npz'))
    model = V.make_local_model(pointnet)
    model.load_state_dict({k[7:]: torch.from_numpy(gl[k]) for k in gl.files if k.startswith('state0/')})
    model.cuda().train()
    emb = pointnet.LocalCloudEmbedder(types.SimpleNamespace(ptn_nfeat_stn=2, stn_as_global=1)).run_batch(model, clouds, clouds_global)
    assert emb.shape == (clouds.shape[0], 4)
    diff = losses.compute_dist(emb, batch[1], batch[2], 'euclidian')
    l1, l2 = losses.compute_loss(types.SimpleNamespace(loss='TVH_zhang', dist_type='euclidian'), diff, batch[3],
                                 torch.ones(diff.shape[0], device='cuda'))
    ((l1 + l2) / diff.shape[0]).backward()
    assert np.isfinite(float(l1.detach())) and np.isfinite(float(l2.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


# ----------------------------------------------------------------------------------------------------------------------
# 2. tiles against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def cloud(N, K, seed, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    xyz = (rng.normal(size=(N, 3)) * scale + offset).astype(np.float32)
    rgb = (rng.integers(0, 256, size=(N, 3)).astype(np.float32) / 255).astype(np.float32)
    nei = rng.integers(0, N, size=(N, K)).astype(np.int64)
    nei[:, 0] = np.arange(N)
    elevation = rng.normal(size=N).astype(np.float32)
    xyn = rng.uniform(size=(N, 2)).astype(np.float32)
    return xyz, rgb, nei, elevation, xyn


def check_tiles(xyz, rgb, nei, k, rows=None, global_feat='', elevation=None, xyn=None, cloud_rgb=True, nei_dtype=np.int64, stream=False):
    from superpoint_graph_amd import ops
    out = ops.neighbourhood_tiles(dev(xyz), dev(nei.astype(nei_dtype)), k, rows=None if rows is None else dev(np.asarray(rows, np.int64)),
                                  rgb=None if rgb is None else dev(rgb), global_feat=global_feat, elevation=None if elevation is None else dev(elevation),
                                  xyn=None if xyn is None else dev(xyn), cloud_rgb=cloud_rgb, stream_stores=stream)
    r = np.arange(len(xyz)) if rows is None else np.asarray(rows, np.int64)
    clouds, diam = R.tiles(xyz, nei, k, r, rgb, cloud_rgb)
    same(out[2], diam, 'diameters')
    same(out[0], clouds, 'clouds')
    same(out[1], R.tile_globals(diam, r, global_feat, xyz, rgb, elevation, xyn), 'clouds_global')
    return out


def test_tiles_single_vertex(hip):
    xyz, rgb, nei, _, _ = cloud(1, 2, 0)
    out = check_tiles(xyz, rgb, nei, 1)
    assert out[0].shape == (1, 6, 1) and float(out[2][0]) == 0.0 and not bool(torch.isnan(out[0]).any())


@pytest.mark.parametrize('k', [1, 2, 3, 20, 47, 64])
def test_tiles_neighbour_counts(hip, k):
    xyz, rgb, nei, e, xyn = cloud(300, k + 3, k)
    check_tiles(xyz, rgb, nei, k, global_feat='eXYrgb', elevation=e, xyn=xyn)


@pytest.mark.parametrize('m', [1, VPB - 1, VPB, VPB + 1, 63, 64, 65, 257, 1000])
def test_tiles_selected_vertex_counts(hip, m):
    xyz, rgb, nei, e, xyn = cloud(1000, 21, 7)
    rows = None if m == 1000 else np.sort(np.random.default_rng(m).choice(1000, m, replace=False))
    check_tiles(xyz, rgb, nei, 20, rows=rows, global_feat='eXYrgb', elevation=e, xyn=xyn, stream=(m % 2 == 1))


def test_tiles_rows_end_at_the_last_vertex(hip):
    xyz, rgb, nei, e, xyn = cloud(500, 20, 8)
    rows = np.concatenate([np.arange(3, 400, 7), [499]])
    check_tiles(xyz, rgb, nei, 20, rows=rows, global_feat='exy', elevation=e)


@pytest.mark.parametrize('nei_dtype', [np.int32, np.int64])
@pytest.mark.parametrize('with_rgb', [True, False])
def test_tiles_index_types_and_colours(hip, nei_dtype, with_rgb):
    xyz, rgb, nei, _, _ = cloud(333, 24, 9)
    out = check_tiles(xyz, rgb if with_rgb else None, nei, 20, nei_dtype=nei_dtype)
    assert out[0].shape == (333, 6 if with_rgb else 3, 20) and out[1].shape == (333, 1)
    if with_rgb:                                         # the reference's use_rgb = 0 with the 'rgb' global feature
        out = check_tiles(xyz, rgb, nei, 20, global_feat='rgb', cloud_rgb=False, nei_dtype=nei_dtype)
        assert out[0].shape == (333, 3, 20) and out[1].shape == (333, 4)


@pytest.mark.parametrize('global_feat,G', [('', 1), ('e', 2), ('rgb', 4), ('XY', 3), ('xy', 3), ('eXYrgb', 7), ('eXYxyrgb', 9)])
def test_tiles_global_features(hip, global_feat, G):
    xyz, rgb, nei, e, xyn = cloud(130, 20, 10)
    out = check_tiles(xyz, rgb, nei, 20, global_feat=global_feat, elevation=e, xyn=xyn)
    assert out[1].shape == (130, G)


def test_tiles_duplicate_neighbourhoods_are_exact_zeros(hip):
    xyz, rgb, nei, _, _ = cloud(100, 20, 11)
    xyz[:40] = np.float32([1.5, 2.25, 0.5])              # dyadic: every sum is exact, the diameter is exactly 0
    xyz[40:70] = np.float32([0.1, 0.7, -0.3])            # the mean of 20 equal values is not the value: a tiny diameter, zeros all the same
    nei[:40] = np.random.default_rng(0).integers(0, 40, size=(40, 20))
    nei[40:70] = np.random.default_rng(1).integers(40, 70, size=(30, 20))
    out = check_tiles(xyz, rgb, nei, 20)
    c, d = host(out[0]), host(out[2])
    assert not np.isnan(c).any() and (c[:70, :3] == 0).all() and (d[:40] == 0).all()


@pytest.mark.parametrize('scale,offset', [(1.0, 1e3), (1e-3, 0.0), (1e-3, 1e3), (30.0, 0.0)])
def test_tiles_scales_and_offsets(hip, scale, offset):
    xyz, rgb, nei, _, _ = cloud(400, 20, 12, scale, offset)
    out = check_tiles(xyz, rgb, nei, 20)
    if scale == 1e-3 and offset == 0.0:
        # the float32 `+ 1e-10` matters here: the float64 form of the denominator gives other bits
        c = xyz[nei]
        d = host(out[2])
        f64 = ((c - xyz[:, None, :]) / (d[:, None, None].astype(np.float64) + 1e-10)).astype(np.float32).transpose(0, 2, 1)
        assert (f64 != host(out[0])[:, :3]).any()


def test_tiles_out_of_range_index(hip):
    from superpoint_graph_amd import ops
    xyz, rgb, nei, _, _ = cloud(200, 20, 13)
    good = [host(t) for t in ops.neighbourhood_tiles(dev(xyz), dev(nei), 20, rgb=dev(rgb))]
    for bad_value in (200, -1):
        bad = nei.copy()
        bad[77, 5] = bad_value
        with pytest.raises(IndexError):
            ops.neighbourhood_tiles(dev(xyz), dev(bad), 20, rgb=dev(rgb))
        with pytest.raises(IndexError):
            ops.neighbourhood_tiles(dev(xyz), dev(bad.astype(np.int32)), 20, rgb=dev(rgb))
    with pytest.raises(IndexError):
        ops.neighbourhood_tiles(dev(xyz), dev(nei), 20, rows=dev(np.array([1, 5, 200])), rgb=dev(rgb))
    # the library call itself: the error word is set and every other row is what it was
    bad = nei.copy()
    bad[77, 5] = 10 ** 6
    x, c, nb = dev(xyz), dev(rgb), dev(bad)
    clouds = torch.full((200, 6, 20), 7.0, device='cuda')
    cg, diam = torch.empty(200, 1, device='cuda'), torch.empty(200, device='cuda')
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    rc = hip.spg_neighbourhood_tiles(x.data_ptr(), c.data_ptr(), 200, nb.data_ptr(), 1, 20, 20, None, 200, 1, None, None, 0, 0, 0, clouds.data_ptr(),
                                     cg.data_ptr(), diam.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and int(err.item()) == 1
    keep = np.arange(200) != 77
    same(clouds[torch.from_numpy(keep).cuda()], good[0][keep], 'clouds of the other rows')
    same(diam[torch.from_numpy(keep).cuda()], good[2][keep], 'diameters of the other rows')
    assert bool(torch.isfinite(clouds).all())
    with pytest.raises(ValueError):
        ops.neighbourhood_tiles(dev(xyz), dev(nei), 21)
    with pytest.raises(ValueError):
        ops.neighbourhood_tiles(dev(xyz), dev(nei), 0)


# ----------------------------------------------------------------------------------------------------------------------
# 3. whole-cloud augmentation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0.0, 1e3])
def test_augment_whole_rotation_within_the_bound(hip, offset):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition.graph_processing import axangle_z
    rng = np.random.default_rng(14)
    xyz = (rng.normal(size=(777, 3)) * 3 + offset).astype(np.float32)
    rgb = rng.uniform(size=(777, 3)).astype(np.float32)
    ref = xyz[123].copy()
    ref[2] = 0
    M = axangle_z(1.2345).astype('f4')
    exact, bound = R.augment_whole64(xyz, ref, M)
    reference = np.matmul(xyz[:, :3] - ref, M) + ref                      # numpy's own float32 result meets the bound
    assert reference.dtype == np.float32 and (np.abs(reference.astype(np.float64) - exact) <= bound).all()
    out, rgb_out = ops.augment_whole(dev(xyz), dev(rgb), ref, M)
    err = np.abs(host(out).astype(np.float64) - exact)
    print('rotation: worst error / bound', float((err / bound).max()), '; numpy', float((np.abs(reference.astype(np.float64) - exact) / bound).max()))
    assert (err <= bound).all()
    same(rgb_out, rgb, 'rgb is untouched')


def test_augment_whole_jitter_and_clip_are_bit_equal(hip):
    from superpoint_graph_amd import ops
    rng = np.random.default_rng(15)
    xyz = (rng.normal(size=(1001, 3)) * 5 + 100).astype(np.float32)
    rgb = rng.uniform(-1, 1, size=(1001, 3)).astype(np.float32)
    rgb[:60] = np.float32(1.0) - rng.uniform(-0.004, 0.004, size=(60, 3)).astype(np.float32)       # around both ends of the clip
    rgb[60:120] = np.float32(-1.0) + rng.uniform(-0.004, 0.004, size=(60, 3)).astype(np.float32)
    n1 = np.clip(0.002 * rng.standard_normal((1001, 3)), -0.005, 0.005).astype(np.float32)
    n2 = np.clip(0.002 * rng.standard_normal((1001, 3)), -0.005, 0.005).astype(np.float32)
    out, rgb_out = ops.augment_whole(dev(xyz), dev(rgb), noise_xyz=dev(n1), noise_rgb=dev(n2))
    same(out, xyz + n1, 'xyz + noise')
    want = np.clip(rgb + n2, -1, 1)
    assert (want == 1).any() and (want == -1).any()
    same(rgb_out, want, 'clip(rgb + noise, -1, 1)')
    out, rgb_out = ops.augment_whole(dev(xyz), None, noise_xyz=dev(n1))
    same(out, xyz + n1, 'xyz + noise')
    assert rgb_out is None
    x, c = dev(xyz), dev(rgb)
    out, rgb_out = ops.augment_whole(x, c)                                # every optional argument None: the inputs, bit for bit
    same(out, xyz, 'no augmentation')
    same(rgb_out, rgb, 'no augmentation')
    with pytest.raises(ValueError):
        ops.augment_whole(x, c, M=np.eye(3, dtype=np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# 4. random subgraph against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def path_graph(n):
    return n, np.arange(n - 1), np.arange(1, n)


def star_graph(leaves):
    return leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1)


def grid_graph(h, w):
    idx = np.arange(h * w).reshape(h, w)
    return h * w, np.concatenate([idx[:, :-1].ravel(), idx[:-1].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:].ravel()])


def two_components():
    n1, s1, t1 = grid_graph(5, 6)
    n2, s2, t2 = grid_graph(10, 10)
    return n1 + n2, np.concatenate([s1, s2 + n1]), np.concatenate([t1, t2 + n1])


def multigraph():
    rng = np.random.default_rng(16)
    src, tgt = rng.integers(0, 60, 240), rng.integers(0, 60, 240)
    src[::15] = tgt[::15]                                                  # self-loops
    return 60, np.concatenate([src, src[:40]]), np.concatenate([tgt, tgt[:40]])   # and parallel edges


def broom():
    """A centre, 1500 leaves, one child per leaf: the second frontier is wider than the workgroup."""
    leaves = np.arange(1, 1501)
    return 3001, np.concatenate([np.zeros(1500, np.int64), leaves]), np.concatenate([leaves, leaves + 1500])


SUBGRAPH_CASES = {
    'path from the middle': (path_graph(300), 100, [150]),
    'path from its end': (path_graph(300), 100, [0]),
    'star from the centre: cut in the middle of a list': (star_graph(200), 50, [0]),
    'star from a leaf': (star_graph(200), 50, [17]),
    'grid': (grid_graph(20, 20), 50, [210]),
    'grid from a corner': (grid_graph(20, 20), 50, [0]),
    'two components, a second seed': (two_components(), 60, [3, 40]),
    'a repeated seed is skipped and consumed': (two_components(), 60, [3, 3, 7, 40, 41]),
    'parallel edges and self-loops': (multigraph(), 25, [5, 6, 7, 8, 9, 10, 11, 12]),
    'size == n': (grid_graph(6, 7), 42, [20]),
    'size == n over two components': (two_components(), 130, [0, 129]),
    'size reached at the end of a list: overshoot through a queued vertex': (path_graph(5), 3, [2]),
    'size reached at the end of a list: no overshoot': (path_graph(5), 3, [0]),
    'size reached in the middle of a list: overshoot': ((6, np.array([1, 0, 0, 0, 2]), np.array([4, 1, 2, 3, 5])), 3, [0]),
    'size reached in the middle of a list: no overshoot': ((6, np.array([0, 0, 0, 1, 2]), np.array([1, 2, 3, 4, 5])), 3, [0]),
    'the seed completes the selection': (two_components(), 31, [0, 35]),
    'size 1': (grid_graph(4, 4), 1, [5]),
    'a vertex without edges as seed': ((5, np.array([1, 2]), np.array([2, 3])), 3, [0, 4, 1]),
    'a frontier wider than the workgroup, cut in its second part': (broom(), 2700, [0]),
    'a frontier wider than the workgroup, cut in its first part': (broom(), 1800, [0]),
}


@pytest.mark.parametrize('name', list(SUBGRAPH_CASES))
def test_random_subgraph_against_the_restatement(hip, name):
    from superpoint_graph_amd import ops
    (n, src, tgt), size, seeds = SUBGRAPH_CASES[name]
    se_r, sv_r, seen_r, used_r, _ = R.random_subgraph(n, src, tgt, size, seeds)
    g = ops.EdgeGraph(dev(src.astype(np.int64)), dev(tgt.astype(np.int64)), n)
    se, sv, seen, used, _ = ops.random_subgraph(g, size, torch.tensor(seeds))
    print(name, ': n_seen', seen, 'of size', size, '; seeds used', used)
    assert (seen, used) == (seen_r, used_r)
    assert se.dtype == torch.uint8 and sv.dtype == torch.uint8
    same(sv, sv_r, 'selected_ver')
    same(se, se_r, 'selected_edg')
    assert int(sv.sum()) == seen


def test_random_subgraph_overshoot_paths_are_covered(hip):
    """Properties of the cases above that the comparison relies on (they hold for the restatement, so for the kernel too)."""
    seen = {name: R.random_subgraph(*case[0], case[1], case[2])[2] - case[1] for name, case in SUBGRAPH_CASES.items()}
    assert seen['size reached at the end of a list: overshoot through a queued vertex'] == 1
    assert seen['size reached at the end of a list: no overshoot'] == 0
    assert seen['size reached in the middle of a list: overshoot'] == 1
    assert seen['size reached in the middle of a list: no overshoot'] == 0
    assert seen['star from the centre: cut in the middle of a list'] == 0 and seen['grid'] == 1 and seen['size == n'] == 0


def test_random_subgraph_exhaustion_and_continuation(hip):
    from superpoint_graph_amd import ops
    n, src, tgt = two_components()
    g = ops.EdgeGraph(dev(src), dev(tgt), n)
    a = ops.random_subgraph(g, 60, [3, 4])
    a_r = R.random_subgraph(n, src, tgt, 60, [3, 4])
    assert a[2] == a_r[2] == 30 and a[3] == a_r[3] == 2
    same(a[1], a_r[1], 'selected_ver after exhaustion')
    b = ops.random_subgraph(g, 60, [5, 77], state=a[4])
    b_r = R.random_subgraph(n, src, tgt, 60, [5, 77], state=a_r[4])
    assert b[2] == b_r[2] >= 60 and b[3] == b_r[3] == 2
    same(b[1], b_r[1], 'selected_ver after the continuation')
    same(b[0], b_r[0], 'selected_edg after the continuation')
    same(a[1], a_r[1], 'the first state is left as it was')
    c = ops.random_subgraph(g, 60, [1], state=b[4])                        # nothing left to do: no seed is consumed
    assert c[2] == b[2] and c[3] == 0
    with pytest.raises(ValueError):
        ops.random_subgraph(g, n + 1, [0])
    with pytest.raises(IndexError):
        ops.random_subgraph(g, 10, [n])
    with pytest.raises(IndexError):
        ops.random_subgraph(g, 10, [-1])


# ----------------------------------------------------------------------------------------------------------------------
# 5. induced subgraph
# ----------------------------------------------------------------------------------------------------------------------
def check_induced(n, src, tgt, sv, se):
    from superpoint_graph_amd import ops
    g = ops.EdgeGraph(dev(src.astype(np.int64)), dev(tgt.astype(np.int64)), n)
    out = ops.induced_subgraph(g, dev(sv.astype(np.uint8)), dev(se.astype(np.uint8)))
    for a, r, what in zip(out, R.induced_subgraph(n, src, tgt, sv, se), ('rows', 'new_ver_index', 'kept', 'edg_source', 'edg_target')):
        assert a.dtype == torch.int64
        same(a, r, what)


def test_induced_subgraph(hip):
    n, src, tgt = grid_graph(20, 20)
    E = len(src)
    check_induced(n, src, tgt, np.zeros(n), np.zeros(E))                                   # empty
    check_induced(n, src, tgt, np.ones(n), np.ones(E))                                     # full
    one = np.zeros(n)
    one[n - 1] = 1
    check_induced(n, src, tgt, one, np.zeros(E))                                           # a single vertex, the last one
    se, sv = R.random_subgraph(n, src, tgt, 50, [210])[:2]
    check_induced(n, src, tgt, sv, se)
    n, src, tgt = multigraph()
    se, sv = R.random_subgraph(n, src, tgt, 25, [5, 6, 7, 8])[:2]
    check_induced(n, src, tgt, sv, se)
    sv2 = np.zeros(n)
    sv2[7] = 1
    check_induced(n, src, tgt, sv2, (src == 7) & (tgt == 7))                               # a single vertex with its self-loops
