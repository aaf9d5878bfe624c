"""Writes tests/golden/plane.npz: sklearn's own RANSACRegressor(random_state=0) on the clouds of tests/plane_cases.py, as the
reference's supervized_partition/graph_processing.py:181-186 runs it, so that no test needs sklearn.  Only recorded arrays:

  <case>/elevation f32 [n]     xyz[:, 2] - reg.predict(xyz[:, :2]) as the reference computes it (parity cases only)
  <case>/inlier_mask u8 [n_low], <case>/coef f64 [2], <case>/intercept f64, <case>/n_trials, <case>/best_trial (the first k for
      which max_trials = k + 1 gives the final consensus set: the stream of triples is a prefix of the same stream)
  <case>/subsets i64 [100, 3]  sample_without_replacement(n_low, 3) from RandomState(0), 100 draws
  <case>/dist                  max |elevation - float64 restatement's elevation|
  sampler/<n> i64 [100, 3]     the same stream at the sizes of plane_cases.SAMPLER_SIZES
  sklearn_seconds/<case>       wall time of the fit and the prediction (median of 3)

Run from the repository root: python tools/gen_plane_golden.py"""
import os
import sys
import time
import warnings

import numpy as np
from sklearn.linear_model import RANSACRegressor
from sklearn.utils.random import sample_without_replacement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import plane_cases as C          # noqa: E402
import plane_restatement as R    # noqa: E402


def stream(n, trials=100, seed=0):
    rs = np.random.RandomState(seed)
    return np.stack([sample_without_replacement(n, 3, random_state=rs) for _ in range(trials)]).astype(np.int64)


def fit(xyz, max_trials=100):
    low = xyz[:, 2] - xyz[:, 2].min() < 0.5
    reg = RANSACRegressor(random_state=0, max_trials=max_trials).fit(xyz[low, :2], xyz[low, 2])
    return reg, xyz[:, 2] - reg.predict(xyz[:, :2])


def main():
    out = {}
    for n in C.SAMPLER_SIZES:
        out[f'sampler/{n}'] = stream(n)
    for name, make in {**C.PARITY, **C.UNPINNED}.items():
        xyz = make()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            reg, elevation = fit(xyz)
            times.append(time.perf_counter() - t0)
        mask = reg.inlier_mask_
        best = -1
        for k in range(1, reg.n_trials_ + 1):
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    r_k, _ = fit(xyz, k)
            except ValueError:
                continue
            if np.array_equal(r_k.inlier_mask_, mask) and np.array_equal(r_k.estimator_.coef_, reg.estimator_.coef_):
                best = k - 1
                break
        rest = R.plane_elevation(xyz)
        if name in C.PARITY:
            out[f'{name}/elevation'] = elevation.astype(np.float32)
        out[f'{name}/inlier_mask'] = mask.astype(np.uint8)
        out[f'{name}/coef'] = np.asarray(reg.estimator_.coef_, np.float64)
        out[f'{name}/intercept'] = np.float64(reg.estimator_.intercept_)
        out[f'{name}/n_trials'] = np.int64(reg.n_trials_)
        out[f'{name}/best_trial'] = np.int64(best)
        out[f'{name}/subsets'] = stream(int(mask.size))
        out[f'{name}/dist'] = np.float64(np.abs(elevation.astype(np.float64) - rest['elevation']).max())
        out[f'sklearn_seconds/{name}'] = np.float64(np.median(times))
        print(f'{name}: n {len(xyz)} n_low {mask.size} trials {reg.n_trials_} best {best} inliers {int(mask.sum())} | restatement trials '
              f"{rest['n_trials']} best {rest['best_trial']} masks equal {np.array_equal(rest['inlier_mask'], mask.astype(np.uint8))} margin "
              f"{rest['margin']:.3g} tie {rest['tie']} | dist {out[f'{name}/dist']:.3g} | sklearn {np.median(times) * 1e3:.1f} ms")
    path = os.path.join(ROOT, 'tests', 'golden', 'plane.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
