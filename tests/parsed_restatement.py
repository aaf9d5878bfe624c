"""Numpy restatement, over arrays, of the per-scene bodies of the reference's four preprocess_pointclouds (learning/s3dis_dataset.py:
111-158, sema3d_dataset.py:102-132, vkitti_dataset.py:97-127, custom_dataset.py:81-107): the feature matrix P in the reference's
dtypes (Python scalars do not widen float32 arrays; rgb is float64; the vkitti position is float64 because it is divided by an
integer array), the gather per component with random.sample's trimming, the centroid, the class count.  Admitted against the
recorded reference by tests/test_parsed_restatement.py; the judge of csrc/spg_parsed.hip in tests/test_gpu_parsed.py.

dist64 / centroid64 are the two statistics outputs in float64: the reference takes them with numpy's float32 pairwise sums, whose
result depends on numpy's blocking and drifts as coordinates grow; the device computes them in float64 and rounds once."""
import random

import numpy as np

NCOLS = {'s3dis': 15, 'sema3d': 11, 'custom': 11, 'vkitti': 14}
DIST_COLUMN = 14              # s3dis only


def features(case, plane_elevation=None):
    """-> P [n, ncols] as the reference concatenates it (float64).  plane_elevation: the elevation of the plane model (float32 [n]) for
    plane_model_elevation without supervized_partition."""
    dataset, xyz = case['dataset'], case['xyz']
    with np.errstate(invalid='ignore', divide='ignore'):
        rgb = case['rgb'].astype(float)
        rgb = rgb / 255.0 - 0.5
        if dataset == 's3dis':
            lpsv = case['geof'].copy()
            if not case['supervized_partition']:
                lpsv -= 0.5
            if case['plane_model_elevation']:
                e = case['elevation'] if case['supervized_partition'] else plane_elevation
            else:
                e = xyz[:, 2] / 4 - 0.5
            room_center = xyz[:, [0, 1]].mean(0)
            d = np.sqrt(((xyz[:, [0, 1]] - room_center) ** 2).sum(1))
            d = (d - d.mean()) / d.std()
            ma, mi = np.max(xyz, axis=0, keepdims=True), np.min(xyz, axis=0, keepdims=True)
            xyzn = (xyz - mi) / (ma - mi + 1e-8)
            assert lpsv.dtype == e.dtype == d.dtype == xyzn.dtype == np.float32
            return np.concatenate([xyz, rgb, e[:, None], lpsv, xyzn, d[:, None]], axis=1)
        if dataset in ('sema3d', 'custom'):
            elpsv = np.concatenate((xyz[:, 2][:, None], case['geof']), axis=1)
            elpsv[:, 0] /= 100
            elpsv[:, 1:] -= 0.5
            assert elpsv.dtype == np.float32
            return np.concatenate([xyz, rgb, elpsv], axis=1)
        z = xyz[:, 2]
        e = (z - np.min(z)) / (np.max(z) - np.min(z)) - 0.5
        xyzn = (xyz - np.array([30, 0, 0])) / np.array([30, 5, 3])
        assert e.dtype == np.float32 and xyzn.dtype == np.float64
        return np.concatenate([xyz, rgb, e[:, None], np.zeros((len(z), 4)), xyzn], axis=1)


def scene(case, plane_elevation=None, rng=random):
    """-> dict: datasets (one float64 array per component, in order), trimmed {component: the positions rng.sample chose}, centroid
    (float32 [3], the reference's; None for custom), class_count (int64 [n_classes]; None for custom).  The caller seeds rng."""
    P = features(case, plane_elevation)
    datasets, trimmed = [], {}
    for c, idx in enumerate(case['components']):
        idx = np.asarray(idx).flatten()
        if idx.size > case['max_points']:
            ii = rng.sample(range(idx.size), k=case['max_points'])
            trimmed[c] = np.asarray(ii, dtype=np.int64)
            idx = idx[ii]
        datasets.append(P[idx, ...])
    custom = case['dataset'] == 'custom'
    count = None if custom else np.bincount(np.argmax(case['labels'][:, 1:], 1), minlength=case['labels'].shape[1] - 1).astype(np.int64)
    return dict(datasets=datasets, trimmed=trimmed, centroid=None if custom else case['xyz'].mean(0), class_count=count)


def dist64(xyz):
    """the standardised distance to the room centre, every step in float64"""
    xy = xyz[:, :2].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.sqrt(((xy - xy.mean(0)) ** 2).sum(1))
        return (d - d.mean()) / d.std()


def centroid64(xyz):
    return xyz.astype(np.float64).mean(0)


def expected_rows(case, plane_elevation=None, rng=random):
    """What the device must hold: (rows float32 [Ntot, ncols] = float32(reference float64 value) with the dist column replaced by
    float32(dist64), offsets int64 [C + 1], the scene() dict, dist64 gathered like the rows (float64 [Ntot]; None off s3dis))."""
    s = scene(case, plane_elevation, rng)
    ncols = NCOLS[case['dataset']]
    sizes = [len(d) for d in s['datasets']]
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    rows = np.concatenate(s['datasets'] + [np.zeros((0, ncols))], 0).astype(np.float32)
    d64 = None
    if case['dataset'] == 's3dis':
        full = dist64(case['xyz'])
        parts = []
        for c, idx in enumerate(case['components']):
            idx = np.asarray(idx).flatten().astype(np.int64)
            parts.append(full[idx[s['trimmed'][c]] if c in s['trimmed'] else idx])
        d64 = np.concatenate(parts + [np.zeros(0)])
        rows[:, DIST_COLUMN] = d64.astype(np.float32)
    return rows, off, s, d64
