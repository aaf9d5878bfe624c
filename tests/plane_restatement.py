"""Float64 numpy restatement of ops.plane_elevation (csrc/spg_plane.hip): the ground-plane elevation of the reference's
supervized_partition/graph_processing.py:181-186 -- RANSACRegressor(random_state=0) of sklearn 1.7 with its defaults, fitted to
the points less than 0.5 above the lowest one.  The six steps:

  1. low        low = z - min(z) < low_height in float32, ascending index order; X = xy[low], y = z[low]
  2. threshold  median(|y - median(y)|) in float32 with numpy's even-count rule (np.median itself)
  3. subsets    sklearn's sample_without_replacement(n_low, 3) stream of np.random.RandomState(seed): `subsets`
  4. trials     the least-squares plane through each triple (`triple_plane`), residual |y - y^| <= threshold, the inlier count and
                the R^2 of the plane on its inliers (`r2`) -- in float64 from the float32 inputs, every trial evaluated
  5. replay     sklearn's acceptance loop over the counts and scores (`replay`)
  6. final fit  the same least squares on the best trial's inliers; elevation = z - (a x + b y + c)

The least squares (`solve_centred`) restates LinearRegression.fit: centre, then scipy's lstsq with cond = max(rows, 2) *
eps_float32 (the input is float32): singular values s <= cond * s_max are dropped, the minimum-norm solution is taken.  It works
from the centred second moments (2 x 2), whose eigenvalues are the squared singular values.

Every expression is written out operation by operation in the order the kernels use, so that the plane of a triple is the same
float64 number on both sides; the sums over points are numpy's pairwise sums here (`seq`) and block-wise there, which is what the
tolerance of tests/test_gpu_plane.py measures (`order`: the final fit's sums over the inliers in another order)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.spacing(1))            # sklearn's _EPSILON


def subsets(n_low, trials, seed=0):
    """the first `trials` triples sklearn's RANSAC draws: sample_without_replacement(n_low, 3, random_state=RandomState(seed))"""
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    rs = np.random.RandomState(seed)
    out = np.empty((trials, 3), np.int64)
    for t in range(trials):
        if n_low == 3:                      # ratio 1: reservoir sampling with nothing to replace
            out[t] = (0, 1, 2)
        elif n_low < 300:                   # 0.01 < 3 / n_low < 0.99
            out[t] = rs.permutation(n_low)[:3]
        else:                               # tracking selection
            sel = []
            for _ in range(3):
                j = rs.randint(n_low)
                while j in sel:
                    j = rs.randint(n_low)
                sel.append(j)
            out[t] = sel
    return out


def seq(v):
    """the sum of v in float64: numpy's pairwise np.sum.  (Not a left-to-right sum: the summands come from float32 coordinates and
    carry few significant bits, so a running sum meets exact rounding ties again and again and round-to-even pulls it one way.  On
    the 200 000-point room 1000 m from the origin the left-to-right sums of the final fit moved the elevation by 2.2e-13 from the one
    of exactly rounded sums (math.fsum) -- in the same direction for the reversed and a shuffled order, which differ from each other
    by only 1e-14 -- where the pairwise sums stay within 3.6e-15 of it.)"""
    v = np.asarray(v, F64)
    return float(np.sum(v)) if v.size else 0.0


def solve_centred(Sxx, Sxy, Syy, Sxz, Syz, rows):
    """minimum-norm least squares of the centred system from its second moments -> (a, b)"""
    cond = max(rows, 2) * EPS32
    tr = Sxx + Syy
    if not (tr > 0.0) or cond >= 1.0:
        return 0.0, 0.0
    det = Sxx * Syy - Sxy * Sxy
    disc = tr * tr - 4.0 * det
    l1 = (tr + math.sqrt(disc if disc > 0.0 else 0.0)) / 2.0
    if det > (cond * cond) * (l1 * l1):
        return (Sxz * Syy - Syz * Sxy) / det, (Syz * Sxx - Sxz * Sxy) / det
    vx, vy = Sxy, l1 - Sxx                  # the eigenvector of l1, from the better conditioned row
    if abs(l1 - Syy) > abs(l1 - Sxx):
        vx, vy = l1 - Syy, Sxy
    vv = vx * vx + vy * vy
    if not (vv > 0.0):
        return 0.0, 0.0
    s = (vx * Sxz + vy * Syz) / (vv * l1)
    return vx * s, vy * s


def triple_plane(P):
    """P float64 [3, 3] (x, y, z) -> (a, b, xr, yr, zr): y^ = (zr + a * (x - xr)) + b * (y - yr), (xr, yr, zr) the centroid"""
    xr, yr, zr = ((P[0] + P[1]) + P[2]) / 3.0
    d = P - np.array([xr, yr, zr])
    Sxx = (d[0, 0] * d[0, 0] + d[1, 0] * d[1, 0]) + d[2, 0] * d[2, 0]
    Sxy = (d[0, 0] * d[0, 1] + d[1, 0] * d[1, 1]) + d[2, 0] * d[2, 1]
    Syy = (d[0, 1] * d[0, 1] + d[1, 1] * d[1, 1]) + d[2, 1] * d[2, 1]
    Sxz = (d[0, 0] * d[0, 2] + d[1, 0] * d[1, 2]) + d[2, 0] * d[2, 2]
    Syz = (d[0, 1] * d[0, 2] + d[1, 1] * d[1, 2]) + d[2, 1] * d[2, 2]
    a, b = solve_centred(float(Sxx), float(Sxy), float(Syy), float(Sxz), float(Syz), 3)
    return a, b, float(xr), float(yr), float(zr)


def residuals(plane, X, y):
    a, b, xr, yr, zr = plane
    return np.abs(y - ((zr + a * (X[:, 0] - xr)) + b * (X[:, 1] - yr)))


def r2(count, S_rr, S_q, S_qq):
    """sklearn's r2_score from the sums over the inliers of r^2, q = y - median and q^2"""
    if count < 2:
        return float('nan')
    ss_tot = S_qq - S_q * S_q / count
    if not (ss_tot > 0.0):
        return 1.0 if S_rr == 0.0 else 0.0
    return 1.0 - S_rr / ss_tot


def dynamic_max_trials(n_inliers, n_samples):
    ratio = n_inliers / float(n_samples)
    denom = max(EPS64, 1 - ratio ** 3)
    if denom == 1:
        return float('inf')
    return abs(float(np.ceil(np.log(max(EPS64, 1 - 0.99)) / np.log(denom))))


def replay(counts, scores, n_low, max_trials):
    """-> (n_trials, best_trial or -1, tie): sklearn's loop over trials whose counts and scores are known"""
    n_best, score_best, best, t, tie = 1, -np.inf, -1, 0, False
    while t < max_trials:
        c, s = int(counts[t]), float(scores[t])
        t += 1
        if c < n_best:
            continue
        if c == n_best and best >= 0:
            tie = True
        if c == n_best and s < score_best:
            continue
        n_best, score_best, best = c, s, t - 1
        max_trials = min(max_trials, dynamic_max_trials(n_best, n_low))
    return t, best, tie


def final_sums(dx, dy, dz, order=None):
    if order is not None:
        dx, dy, dz = dx[order], dy[order], dz[order]
    return [seq(v) for v in (dx, dy, dz, dx * dx, dx * dy, dy * dy, dx * dz, dy * dz)]


def final_model(sums, n_in, ref):
    Sx, Sy, Sz, Sxx, Sxy, Syy, Sxz, Syz = sums
    a, b = solve_centred(Sxx - Sx * Sx / n_in, Sxy - Sx * Sy / n_in, Syy - Sy * Sy / n_in, Sxz - Sx * Sz / n_in, Syz - Sy * Sz / n_in, n_in)
    xm, ym, zm = ref[0] + Sx / n_in, ref[1] + Sy / n_in, ref[2] + Sz / n_in
    return a, b, (zm - a * xm) - b * ym


def elevation_of(xyz64, a, b, c):
    return xyz64[:, 2] - ((a * xyz64[:, 0] + b * xyz64[:, 1]) + c)


def plane_elevation(xyz, subsets_=None, seed=0, max_trials=100, low_height=0.5, orders=()):
    """xyz float32 [n, 3] -> dict: elevation (float64), coef, intercept, threshold (float32), low_index, inlier_mask, n_low,
    n_trials, best_trial, margin (the smallest |residual - threshold| / threshold over the evaluated trials; nan when the
    threshold is 0), tie (a trial met the best count of an accepted one), subsets; and `reordered`: the elevation with the final
    fit's sums taken in each of `orders` ('reversed' or a seed of a shuffle)."""
    xyz = np.ascontiguousarray(xyz, F32)
    if not np.isfinite(xyz).all():
        raise ValueError('Input contains NaN or infinity.')
    z = xyz[:, 2]
    low_index = np.flatnonzero((z - z.min()) < F32(low_height)).astype(np.int32)
    n_low = int(low_index.size)
    y32 = z[low_index]
    threshold = np.median(np.abs(y32 - np.median(y32)))
    assert threshold.dtype == F32
    sub = subsets(n_low, max_trials, seed) if subsets_ is None else np.asarray(subsets_, np.int64).reshape(-1, 3)
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    T = len(sub)
    X, y = xyz[low_index, :2].astype(F64), y32.astype(F64)
    med, thr = float(np.median(y32)), float(threshold)
    q = y - med
    pts = np.concatenate([X, y[:, None]], 1)
    planes, counts, scores, res = [], np.zeros(T, np.int64), np.zeros(T), []
    for t in range(T):
        planes.append(triple_plane(pts[sub[t]]))
        r = residuals(planes[t], X, y)
        m = r <= thr
        counts[t] = int(m.sum())
        scores[t] = r2(counts[t], seq((r * r)[m]), seq(q[m]), seq((q * q)[m]))
        res.append(r)
    n_trials, best, tie = replay(counts, scores, n_low, T)
    if best < 0:
        raise ValueError('RANSAC could not find a valid consensus set.')
    margin = float('nan')
    if thr > 0:
        margin = min(float(np.abs(res[t] - thr).min()) / thr for t in range(n_trials))
    mask = res[best] <= thr
    ref = planes[best][2:]
    dx, dy, dz = X[mask, 0] - ref[0], X[mask, 1] - ref[1], y[mask] - ref[2]
    n_in = int(mask.sum())
    a, b, c = final_model(final_sums(dx, dy, dz), n_in, ref)
    xyz64 = xyz.astype(F64)
    reordered = []
    for o in orders:
        perm = np.arange(n_in)[::-1] if o == 'reversed' else np.random.RandomState(o).permutation(n_in)
        reordered.append(elevation_of(xyz64, *final_model(final_sums(dx, dy, dz, perm), n_in, ref)))
    return dict(elevation=elevation_of(xyz64, a, b, c), coef=np.array([a, b]), intercept=c, threshold=threshold, low_index=low_index,
                inlier_mask=mask.astype(np.uint8), n_low=n_low, n_trials=n_trials, best_trial=best, margin=margin, tie=tie, subsets=sub,
                counts=counts, scores=scores, reordered=reordered)
