"""CPU: the numpy restatement of preprocess_pointclouds (tests/parsed_restatement.py) against the reference's own four functions,
recorded in tests/golden/parsed.npz by tools/gen_parsed_golden.py, and the admission of the cases of tests/parsed_cases.py.

1. On every PARITY case the restatement equals the record bit for bit after .astype(np.float32) -- every column, `dist` included,
   in float32 as the reference computed it (not on UNPINNED cases, whose `dist` is NaN in exact arithmetic); the sizes, the trimmed
   selections and class_count as integers; the centroid bit for bit.
2. Admission of every case: component indices in range; where a case is tagged exact_sums the float64 sums are exact; on
   small_coords cases the float32 reference's `dist` lies within 1e-4 (the project's fp32 parity; measured <= 8.4e-7) of dist64, with
   the same NaN positions; the degenerate scenes give what the issue names (extent 0 -> xyzn 0, vkitti e NaN, dist NaN)."""
import os
import random

import numpy as np
import pytest

import parsed_cases as C
import parsed_restatement as R
from conftest import GOLDEN


@pytest.fixture(scope='module')
def rec():
    return np.load(os.path.join(GOLDEN, 'parsed.npz'))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restated(case):
    assert 'plane' not in case['tags']
    random.seed(case['seed'])
    return R.scene(case)


def test_the_record_covers_the_parity_cases(rec):
    assert sorted({k.split('/')[0] for k in rec.files}) == sorted(C.names('PARITY'))
    assert len(C.names('PARITY')) >= 30 and any('trim' in k for k in rec.files)


@pytest.mark.parametrize('name', C.names('PARITY'))
def test_restatement_equals_the_reference(rec, name):
    case = C.get(name)
    s = restated(case)
    assert np.array_equal([len(d) for d in s['datasets']], rec[f'{name}/sizes'])
    got = np.concatenate([d[::case['stride']] for d in s['datasets']], 0)
    want = rec[f'{name}/rows']
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape and got.shape[1] == R.NCOLS[case['dataset']]
    cols = list(range(got.shape[1]))
    if case['dataset'] == 's3dis' and 'UNPINNED' in case['tags']:
        cols.remove(R.DIST_COLUMN)
    assert np.array_equal(bits(got[:, cols]), bits(want[:, cols]))
    trims = sorted(int(k.split('/trim')[1]) for k in rec.files if k.startswith(f'{name}/trim'))
    assert trims == sorted(s['trimmed'])
    for c in trims:
        assert np.array_equal(s['trimmed'][c], rec[f'{name}/trim{c}'])
    if case['dataset'] == 'custom':
        assert s['centroid'] is None and s['class_count'] is None and f'{name}/centroid' not in rec.files
    else:
        assert np.array_equal(s['class_count'], rec[f'{name}/class_count'])
        assert s['centroid'].dtype == rec[f'{name}/centroid'].dtype == np.float32
        assert np.array_equal(bits(s['centroid']), bits(rec[f'{name}/centroid']))


def test_trimming_is_exercised(rec):
    case = C.get('sema3d_trim10001')
    sizes = [len(c) for c in case['components']]
    assert sizes[:2] == [10000, 10001] and list(rec['sema3d_trim10001/sizes'][:2]) == [10000, 10000]
    assert [k for k in rec.files if k.startswith('sema3d_trim10001/trim')] == ['sema3d_trim10001/trim1']
    for name in ('s3dis_max7', 'sema3d_max7'):
        case = C.get(name)
        s = restated(case)
        assert len(s['trimmed']) >= 3 and all(len(d) <= 7 for d in s['datasets'])
        # the selections are Python's stream consumed in component order
        random.seed(case['seed'])
        for c in sorted(s['trimmed']):
            assert np.array_equal(s['trimmed'][c], random.sample(range(len(case['components'][c])), k=7))


@pytest.mark.parametrize('name', C.names())
def test_admission(name):
    case = C.get(name)
    n, xyz = len(case['xyz']), case['xyz']
    assert xyz.dtype == np.float32 and case['geof'].dtype == np.float32 and case['rgb'].dtype in (np.uint8, np.float32)
    assert case['labels'].dtype in (np.uint32, np.int32) and case['labels'].shape == (n, C.N_CLASSES[case['dataset']] + 1)
    assert np.isfinite(xyz).all()
    for idx in case['components']:
        idx = np.asarray(idx)
        assert idx.size == 0 or (idx.dtype.kind in 'iu' and idx.min() >= 0 and idx.max() < n)
    for k in range(3):                      # no zeros of mixed sign at an extreme (parsed_cases.py)
        for ext in (xyz[:, k].min(), xyz[:, k].max()):
            if ext == 0:
                assert len(set(np.signbit(xyz[xyz[:, k] == 0, k]))) == 1
    if 'small_coords' in case['tags']:
        assert np.abs(xyz).max() < 10
    if 'exact_sums' in case['tags']:
        # the float64 sums are exact in any order: every partial sum of the coordinates fits 53 bits, the centre is a float64 number
        # from which both (all) points are equally far, so d - mean(d) is exactly 0
        x64 = xyz.astype(np.float64)
        assert n <= 2 or (x64 == x64[0]).all()
        assert np.array_equal(R.centroid64(xyz), x64.sum(0) / n) and np.array_equal(x64.mean(0) * n, x64.sum(0))
        assert np.isnan(R.dist64(xyz)).all()
    if case['dataset'] == 's3dis' and 'plane' not in case['tags']:
        d32, d64 = R.features(case)[:, R.DIST_COLUMN], R.dist64(xyz)
        if 'UNPINNED' not in case['tags']:
            assert np.array_equal(np.isnan(d32), np.isnan(d64))
            if 'small_coords' in case['tags']:
                err = np.nanmax(np.abs(d32 - d64)) if not np.isnan(d64).all() else 0.0
                assert err <= 1e-4, err


def test_degenerate_scenes():
    for name in ('s3dis_identical', 's3dis_flat_z', 's3dis_negzero_axis'):
        case = C.get(name)
        P = R.features(case)
        flat_axes = [k for k in range(3) if case['xyz'][:, k].min() == case['xyz'][:, k].max()]
        assert flat_axes and all((bits(P[:, 11 + k]) == 0).all() for k in flat_axes)            # extent 0: xyzn = +0.0
    assert np.isnan(R.dist64(C.get('s3dis_identical')['xyz'])).all() and np.isnan(R.dist64(C.get('s3dis_n1')['xyz'])).all()
    assert np.isnan(R.dist64(C.get('s3dis_n2')['xyz'])).all()
    for name in ('vkitti_identical', 'vkitti_flat_z'):
        assert np.isnan(R.features(C.get(name))[:, 6]).all()                                    # 0 / 0
    neg = C.get('s3dis_negzero')['xyz']
    assert (np.signbit(neg) & (neg == 0)).any() and ((neg == 0) & ~np.signbit(neg)).any()


def test_class_count_cases():
    for name in ('s3dis_n65', 's3dis_components'):
        lab = C.get(name)['labels'][:, 1:]
        top = lab.max(1)
        assert (top == 0).any() and ((lab == top[:, None]).sum(1) > 1)[top > 0].any()
    assert C.get('s3dis_components')['labels'].dtype == np.int32 and C.get('s3dis_n65')['labels'].dtype == np.uint32
