"""GPU: parsed superpoint clouds on the device (csrc/spg_parsed.hip, ops.parsed_points / ops.class_count,
learning/parsed.py: preprocess_scene, DevicePointCache.put) against the numpy restatement of the reference's
preprocess_pointclouds (tests/parsed_restatement.py, admitted against the recorded reference by tests/test_parsed_restatement.py)
on every scene of tests/parsed_cases.py.

Exact columns: every column but `dist` is bit-equal to float32(the reference's float64 value), NaNs by position; offsets, ids,
class_count and the trimmed selections are equal as integers.
`dist` and `centroid`: within ONE float32 ulp at max(|expected|, 1) of the float64 restatement (dist64 / centroid64), NaNs at its
positions.  Derived, not measured: the device rounds a float64 value once (half an ulp), and that value's own error -- sums of
float64 terms in another order than numpy's, at |coordinate| <= 1e5 about 1e-11 absolute on the centre -- is far below a float32 ulp
and can at most move the rounding to the neighbouring float.  On small_coords cases `dist` also lies within 1e-4 (the project's
fp32 parity) of the recorded float32 reference.
`python tests/test_gpu_parsed.py` prints the observed maxima (profiles/parsed_errors.txt)."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import parsed_cases as C
import parsed_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def device_inputs(case):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(xyz=t(case['xyz']), rgb=t(case['rgb']), geof=None if case['dataset'] == 'vkitti' else t(case['geof']),
                elevation=t(case['elevation']), labels=t(case['labels']))


def device_scene(case, components=None, inputs=None):
    from superpoint_graph_amd.learning import parsed
    d = inputs or device_inputs(case)
    random.seed(case['seed'])
    return parsed.preprocess_scene(case['dataset'], d['xyz'], d['rgb'], case['components'] if components is None else components,
                                   geof=d['geof'], elevation=d['elevation'], labels=d['labels'],
                                   supervized_partition=case['supervized_partition'], plane_model_elevation=case['plane_model_elevation'],
                                   max_points=case['max_points'])


def expected(case, plane_elevation=None):
    random.seed(case['seed'])
    return R.expected_rows(case, plane_elevation)


def plane_of(case):
    from superpoint_graph_amd import ops
    if 'plane' not in case['tags']:
        return None
    return ops.plane_elevation(torch.from_numpy(case['xyz']).to(DEV))['elevation'].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits_nan_by_position(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))


def ulp_error(got32, want64):
    """-> (NaN positions agree, max |got - want| / ulp_f32(max(|want|, 1)) over the others)"""
    got, want = np.asarray(got32, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False, np.inf, np.inf
    if wn.all():
        return True, 0.0, 0.0
    ulp = np.spacing(np.maximum(np.abs(want[~wn]), 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(got[~wn] - want[~wn])
    return True, float((err / ulp).max()), float(err.max())


def measure(name, rec):
    case = C.get(name)
    e_plane = plane_of(case)
    rows, off, s, d64 = expected(case, e_plane)
    p = device_scene(case)
    got = p.points.cpu().numpy()
    m = types.SimpleNamespace(case=case, parsed=p, got=got, rows=rows, off=off, s=s, e_plane=e_plane, dist_ulps=0.0, dist_abs=0.0,
                              dist_nan=True, dist_ref=0.0, cen_ulps=0.0, cen_nan=True)
    if case['dataset'] == 's3dis':
        m.dist_nan, m.dist_ulps, m.dist_abs = ulp_error(got[:, R.DIST_COLUMN], d64) if got.shape == rows.shape else (False, np.inf, np.inf)
        if {'small_coords', 'PARITY'} <= case['tags'] and 'UNPINNED' not in case['tags']:
            ref = rec[f'{name}/rows'][:, R.DIST_COLUMN].astype(np.float32)
            assert case['stride'] == 1 and ref.shape == got[:, R.DIST_COLUMN].shape
            d = np.abs(got[:, R.DIST_COLUMN].astype(np.float64) - ref)
            m.dist_ref = float(np.nanmax(d)) if not np.isnan(d).all() else 0.0
            m.dist_ref_nan = bool(np.array_equal(np.isnan(got[:, R.DIST_COLUMN]), np.isnan(ref)))
    if p.centroid is not None:
        m.cen_nan, m.cen_ulps, _ = ulp_error(p.centroid.cpu().numpy(), R.centroid64(case['xyz']))
    return m


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'parsed.npz'))


@pytest.mark.parametrize('name', C.names())
def test_against_the_restatement(hip, rec, name):
    m = measure(name, rec)
    case, p = m.case, m.parsed
    ncols = R.NCOLS[case['dataset']]
    assert p.points.dtype == torch.float32 and tuple(p.points.shape) == (int(m.off[-1]), ncols)
    assert p.offsets.dtype == np.int64 and np.array_equal(p.offsets, m.off) and p.ids == list(range(len(case['components'])))
    assert sorted(p.trimmed) == sorted(m.s['trimmed']) and all(np.array_equal(p.trimmed[c], m.s['trimmed'][c]) for c in p.trimmed)
    if case['dataset'] == 'custom':
        assert p.class_count is None and p.centroid is None
    else:
        assert p.class_count.dtype == np.int64 and np.array_equal(p.class_count, m.s['class_count'])
    exact = [c for c in range(ncols) if not (case['dataset'] == 's3dis' and c == R.DIST_COLUMN)]
    for c in exact:
        assert same_bits_nan_by_position(m.got[:, c], m.rows[:, c]), (name, 'column', c)
    if 'plane' in case['tags']:
        assert np.array_equal(bits(m.rows[:, 6]), bits(np.concatenate([m.e_plane[np.asarray(i, dtype=np.int64)] for i in case['components']])))
    print(f'{name}: dist {m.dist_ulps:.3f} ulp ({m.dist_abs:.3e}), |dist - float32 reference| {m.dist_ref:.3e}, centroid {m.cen_ulps:.3f} ulp')
    assert m.dist_nan and m.dist_ulps <= 1.0, (m.dist_ulps, m.dist_abs)
    assert m.cen_nan and m.cen_ulps <= 1.0, m.cen_ulps
    assert m.dist_ref <= 1e-4 and getattr(m, 'dist_ref_nan', True), m.dist_ref
    if 'exact_sums' in case['tags'] and p.centroid is not None:          # exact sums: the statistics are numpy's float64 ones, bit for bit
        assert np.array_equal(bits(p.centroid.cpu().numpy()), bits(R.centroid64(case['xyz']).astype(np.float32)))
    # to_store: the dict MemoryPointStore takes
    store = p.to_store()
    assert sorted(store) == p.ids and all(store[i].dtype == np.float32 and store[i].shape == (m.off[k + 1] - m.off[k], ncols) for k, i in enumerate(p.ids))


def test_component_forms_agree(hip):
    """a list of index arrays, a device CSR pair (int32 and int64 indices) and in_component give the same rows"""
    case = C.get('s3dis_n257')
    d = device_inputs(case)
    want = device_scene(case, inputs=d)
    off = np.zeros(len(case['components']) + 1, np.int64)
    np.cumsum([len(c) for c in case['components']], out=off[1:])
    flat = np.concatenate(case['components']).astype(np.int64)
    for idx in (torch.from_numpy(flat).to(DEV), torch.from_numpy(flat.astype(np.int32)).to(DEV)):
        for o in (off, torch.from_numpy(off).to(DEV)):
            got = device_scene(case, components=(o, idx), inputs=d)
            assert torch.equal(got.points.view(torch.int32), want.points.view(torch.int32)) and np.array_equal(got.offsets, want.offsets)
    in_component = np.empty(len(case['xyz']), np.int64)
    for c, idx in enumerate(case['components']):
        in_component[idx.astype(np.int64)] = c
    got = device_scene(case, components=torch.from_numpy(in_component).to(DEV), inputs=d)
    asc = device_scene(case, components=[np.sort(c) for c in case['components']], inputs=d)      # ascending members per component
    assert torch.equal(got.points.view(torch.int32), asc.points.view(torch.int32)) and np.array_equal(got.offsets, asc.offsets)


def test_class_count_dtypes(hip):
    from superpoint_graph_amd import ops
    for name in ('s3dis_n65', 's3dis_components', 's3dis_gridstride'):
        lab = C.get(name)['labels']
        want = np.bincount(np.argmax(lab[:, 1:], 1), minlength=lab.shape[1] - 1)
        got = ops.class_count(torch.from_numpy(lab).to(DEV), lab.shape[1] - 1)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    big = np.zeros((5, 3), np.uint32)
    big[:, 1], big[:, 2] = 0x7fffffff, 0x80000000                   # unsigned: column 2 wins; the same bits as int32: column 1
    assert ops.class_count(torch.from_numpy(big).to(DEV), 2).tolist() == [0, 5]
    assert ops.class_count(torch.from_numpy(big.view(np.int32)).to(DEV), 2).tolist() == [5, 0]
    assert ops.class_count(torch.zeros(0, 3, dtype=torch.int32, device=DEV), 2).tolist() == [0, 0]


@pytest.mark.parametrize('name', ['s3dis_n1025', 's3dis_gridstride'])
def test_two_runs_give_the_same_bits(hip, name):
    case = C.get(name)
    d = device_inputs(case)
    a, b = device_scene(case, inputs=d), device_scene(case, inputs=d)
    assert torch.equal(a.points.view(torch.int32), b.points.view(torch.int32))
    assert torch.equal(a.centroid.view(torch.int32), b.centroid.view(torch.int32))


def test_error_word(hip):
    from superpoint_graph_amd import ops
    case = C.get('s3dis_n257')
    d = device_inputs(case)
    n = len(case['xyz'])
    off = torch.tensor([0, 3, 3, 8], dtype=torch.int64)
    idx = torch.tensor([5, 6, 7, 0, 1, 2, 3, n - 1], dtype=torch.int32, device=DEV)
    args = ('s3dis', d['xyz'], d['rgb'], off)
    pts, cen, o = ops.parsed_points(*args, idx, geof=d['geof'], trim={2: [4, 0]})
    assert o.tolist() == [0, 3, 3, 5] and torch.equal(pts[3:, :3], d['xyz'][[n - 1, 0]])
    for bad in (float('nan'), float('inf'), float('-inf')):
        xyz = d['xyz'].clone()
        xyz[n // 2, 1] = bad
        with pytest.raises(ValueError, match='NaN or infinity'):
            ops.parsed_points('s3dis', xyz, d['rgb'], off, idx, geof=d['geof'])
    for v in (n, -1):
        bad_idx = idx.clone()
        bad_idx[6] = v
        with pytest.raises(IndexError, match='component index'):
            ops.parsed_points(*args, bad_idx, geof=d['geof'])
        with pytest.raises(IndexError, match='component index'):
            ops.parsed_points(*args, bad_idx.to(torch.int64), geof=d['geof'])
    for t in (5, -1):                                                 # component 2 has 5 members
        with pytest.raises(IndexError, match='trim position'):
            ops.parsed_points(*args, idx, geof=d['geof'], trim={2: [1, t]})
    with pytest.raises(ValueError):
        ops.parsed_points(*args, idx[:7], geof=d['geof'])              # comp_off runs past comp_idx: refused on the host


@pytest.mark.parametrize('n', [1, 257, C.REDUCE_BLOCK * C.REDUCE_MAX_BLOCKS + 1])
def test_workspace_query_is_what_the_layout_consumes(hip, n):
    """the pattern of tests/test_gpu_partition_workspace.py: exactly spg_parsed_workspace_bytes(n) bytes are enough and give the
    wrapper's bits; one byte less is refused before anything is written, and the error names the query"""
    from superpoint_graph_amd import ops
    from test_gpu_partition_workspace import P, exact_and_short, fresh, stream
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    xyz = torch.from_numpy(C.room(n, 0.0, 3)).to(DEV)
    s32, s64, cen = ops.scene_stats(xyz, True)
    exact_and_short(hip, 'spg_parsed_workspace_bytes', hip.spg_parsed_workspace_bytes(n), lambda: fresh((6, f32), (5, f64), (3, f32), (1, i32)),
                    lambda o, ws, b: hip.spg_parsed_stats(P(xyz), n, 1, P(o[0]), P(o[1]), P(o[2]), P(o[3]), ws, b, stream()),
                    [(0, s32, None), (1, s64, None), (2, cen, None), (3, torch.zeros(1, dtype=i32, device=DEV), None)])


def loader_args(attribs, minpts):
    return types.SimpleNamespace(ptn_minpts=minpts, ptn_npts=32, pc_xyznormalize=1, pc_attribs=attribs, pc_augm_scale=0, pc_augm_rot=0,
                                 pc_augm_mirror_prob=0, pc_augm_jitter=0, spg_augm_hardcutoff=0, spg_augm_nneigh=0, spg_augm_order=0)


@pytest.mark.parametrize('attribs', ['', 'xyzelpsv'])
def test_end_to_end_sema3d_through_the_loader(hip, attribs):
    """device-parsed rows -> DevicePointCache.put -> spg.loader: the clouds, diameters and flags of a DevicePointCache over
    MemoryPointStore(the restatement's rows), bit for bit (every column of the sema3d recipe is exact)"""
    from superpoint_graph_amd.learning import spg
    case = C.get('sema3d_n257')
    sizes = sorted(len(c) for c in case['components'])
    minpts = sizes[len(sizes) // 2]
    assert sizes[0] < minpts <= sizes[-1]                              # a superpoint below ptn_minpts, and one that is kept
    random.seed(case['seed'])
    rows = [a.astype(np.float32) for a in R.scene(case)['datasets']]
    n_sp = len(rows)
    G = spg.SuperpointGraph(n_sp, [(i, (i + 1) % n_sp) for i in range(n_sp)], True, {'f': [[0.5]] * n_sp},
                            {'v': list(range(n_sp)), 't': [[i % 8, 1] for i in range(n_sp)]})
    dev = torch.device('cuda', torch.cuda.current_device())
    want_cache = spg.DevicePointCache(spg.MemoryPointStore({'scene': dict(enumerate(rows))}), dev)
    cache = spg.DevicePointCache(None, dev)
    with pytest.raises(KeyError):
        cache.scene('scene')
    cache.put('scene', device_scene(case))
    args = loader_args(attribs, minpts)
    got = spg.loader((G, 'scene'), False, args, None, test_seed_offset=3, device_cache=cache)
    want = spg.loader((G, 'scene'), False, args, None, test_seed_offset=3, device_cache=want_cache)
    assert np.array_equal(got[0], want[0]) and got[2] == want[2]
    assert np.array_equal(np.asarray(got[3]), np.asarray(want[3])) and (np.asarray(got[3]) == -1).any() and (np.asarray(got[3]) == 0).any()
    assert got[4].shape[1] == (11 if attribs == '' else 8)
    assert torch.equal(got[4].view(torch.int32), want[4].view(torch.int32)) and torch.equal(got[5].view(torch.int32), want[5].view(torch.int32))


def test_end_to_end_s3dis_plane_model_elevation(hip):
    """plane_model_elevation=1: the e column is ops.plane_elevation(xyz) of the same cloud, bit for bit, through cache and loader"""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import spg
    case = C.get('s3dis_plane')
    p = device_scene(case)
    e = ops.plane_elevation(torch.from_numpy(case['xyz']).to(DEV))['elevation']
    flat = torch.from_numpy(np.concatenate(case['components']).astype(np.int64)).to(DEV)
    assert torch.equal(p.points[:, 6].view(torch.int32), e[flat].view(torch.int32))
    dev = torch.device('cuda', torch.cuda.current_device())
    cache = spg.DevicePointCache(None, dev)
    cache.put('room', p)
    pts, off, index = cache.scene('room')
    assert pts is p.points and np.array_equal(off, p.offsets) and index == {i: i for i in range(len(case['components']))}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec_ = np.load(os.path.join(GOLDEN, 'parsed.npz'))
    print('# python tests/test_gpu_parsed.py')
    print('# per case: rows and columns of the device buffer; max |device dist - dist64| in float32 ulps at max(|dist64|, 1) and absolute')
    print('# (bound: 1 ulp); max |device dist - the recorded float32 reference| (bound 1e-4 on small_coords cases; "-" where not compared);')
    print('# max |device centroid - centroid64| in ulps (bound: 1).  Every other column is compared bit for bit by the test.')
    print(f'{"case":<24}{"rows":>8}{"cols":>5}{"dist ulp":>10}{"dist abs":>11}{"vs f32 ref":>12}{"centroid ulp":>14}')
    worst = [0.0, 0.0, 0.0, 0.0]
    for name_ in C.names():
        m_ = measure(name_, rec_)
        s3 = m_.case['dataset'] == 's3dis'
        compared = s3 and {'small_coords', 'PARITY'} <= m_.case['tags'] and 'UNPINNED' not in m_.case['tags']
        print(f'{name_:<24}{m_.got.shape[0]:>8}{m_.got.shape[1]:>5}' + (f'{m_.dist_ulps:>10.3f}{m_.dist_abs:>11.3e}' if s3 else f'{"-":>10}{"-":>11}')
              + (f'{m_.dist_ref:>12.3e}' if compared else f'{"-":>12}') + (f'{m_.cen_ulps:>14.3f}' if m_.parsed.centroid is not None else f'{"-":>14}'))
        worst = [max(a, b) for a, b in zip(worst, (m_.dist_ulps, m_.dist_abs, m_.dist_ref, m_.cen_ulps))]
    print(f'# maxima: dist {worst[0]:.3f} ulp, {worst[1]:.3e} absolute; vs the float32 reference {worst[2]:.3e}; centroid {worst[3]:.3f} ulp')
