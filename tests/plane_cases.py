"""The clouds of the ground-plane tests (tests/test_plane_restatement.py, tests/test_gpu_plane.py, tools/gen_plane_golden.py):
seeded synthetic rooms, all float32 [n, 3].

room(n, offset, seed):      60 % of the points on a tilted noisy floor, the rest clutter up to 3 m above it; x and y moved by `offset`.
low_count(k, n_high, seed): exactly k low points (a tilted noisy floor and clutter within 0.45 of the lowest point, which is pinned at
                            z = 0) and n_high points at 0.6 or more: the branches of the sampler (3, 4, 299, 300, 301) and the
                            block edges of the trial pass (1023, 1024, 1025 and several blocks).
flat_floor(n, seed):        70 % of the points at exactly z = 0, so the threshold (a median of absolute deviations) is 0.

PARITY cases are admitted by tests/test_plane_restatement.py against the sklearn record tests/golden/plane.npz; UNPINNED ones are
recorded too but judged by the restatement alone (sklearn fits in float32 and classifies a point next to the threshold the
other way there)."""
import numpy as np

F32 = np.float32
BLOCK_POINTS = 1024          # low points per workgroup of the trial pass (csrc/spg_plane.hip: PL_BLOCK * PL_PER_LANE)


def room(n, offset=0.0, seed=0):
    rng = np.random.RandomState(seed)
    n_floor = int(0.6 * n)
    xy = rng.uniform(0, (8.0, 5.0), size=(n, 2))
    z = np.empty(n)
    z[:n_floor] = 0.02 * xy[:n_floor, 0] - 0.015 * xy[:n_floor, 1] + 0.2 + rng.normal(0, 0.01, n_floor)
    z[n_floor:] = rng.uniform(0.0, 3.0, n - n_floor)
    p = rng.permutation(n)
    return np.concatenate([xy + offset, z[:, None]], 1)[p].astype(F32)


def low_count(k, n_high=50, seed=0, clutter=0.4):
    rng = np.random.RandomState(seed)
    n_clutter = int(clutter * k) if k >= 8 else 0
    xy = rng.uniform(0, (6.0, 4.0), size=(k + n_high, 2))
    z = np.empty(k + n_high)
    nf = k - n_clutter
    z[:nf] = 0.03 * xy[:nf, 0] + 0.02 * xy[:nf, 1] + 0.05 + rng.normal(0, 0.002, nf)
    z[nf:k] = rng.uniform(0.0, 0.45, n_clutter)
    z[k:] = rng.uniform(0.6, 2.5, n_high)
    xy[0], z[0] = (0.0, 0.0), 0.0            # the lowest point: every other low one is below 0.45
    p = rng.permutation(k + n_high)
    out = np.concatenate([xy, z[:, None]], 1)[p].astype(F32)
    assert int(((out[:, 2] - out[:, 2].min()) < F32(0.5)).sum()) == k
    return out


def flat_floor(n=600, seed=0):
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, (6.0, 4.0), size=(n, 2))
    z = np.where(np.arange(n) < int(0.7 * n), 0.0, rng.uniform(0.01, 2.0, n))
    p = rng.permutation(n)
    return np.concatenate([xy, z[:, None]], 1)[p].astype(F32)


PARITY = {
    'room2000': lambda: room(2000, 0.0, 1),
    'room20000': lambda: room(20000, 0.0, 2),
    'room20000_100m': lambda: room(20000, 100.0, 3),
    'low3': lambda: low_count(3, 40, 4),
    'low4': lambda: low_count(4, 40, 5),
    'low299': lambda: low_count(299, 50, 6),
    'low300': lambda: low_count(300, 50, 7),
    'low301': lambda: low_count(301, 50, 8),
    'block_minus': lambda: low_count(BLOCK_POINTS - 1, 100, 9),
    'block_exact': lambda: low_count(BLOCK_POINTS, 100, 10),
    'block_plus': lambda: low_count(BLOCK_POINTS + 1, 100, 11),
    'blocks': lambda: low_count(3 * BLOCK_POINTS + 77, 300, 12),
    'all_low': lambda: low_count(500, 0, 17),
}
UNPINNED = {
    'room200000_1000m': lambda: room(200000, 1000.0, 14),
    'flat_floor': lambda: flat_floor(600, 15),
}


def degenerate_floor(seed=16):
    """flat_floor and, at the end, three low points on the line x = 1 whose heights are not collinear: the threshold is 0 and the
    minimum-norm plane of that triple meets no point exactly -> (xyz, the triple's indices among the low points)"""
    xyz = np.concatenate([flat_floor(600, seed), np.array([[1, 0, 0.1], [1, 1, 0.2], [1, 3, 0.45]], F32)])
    k = int(((xyz[:, 2] - xyz[:, 2].min()) < F32(0.5)).sum())
    return xyz, [k - 3, k - 2, k - 1]


def floor_triple(xyz):
    """the first three low points at z = 0 of a flat floor, as indices among the low points"""
    low = np.flatnonzero((xyz[:, 2] - xyz[:, 2].min()) < F32(0.5))
    return np.flatnonzero(xyz[low, 2] == 0)[:3].tolist()


def _explicit():
    base = PARITY['low299']()
    low = np.flatnonzero((base[:, 2] - base[:, 2].min()) < F32(0.5))
    draws = np.random.RandomState(21).randint(0, 299, size=(6, 3)).tolist()
    lined = base.copy()
    lined[low[5:8], 0] = F32(2.5)                        # low points 5, 6, 7 share their x
    degenerate, special = degenerate_floor()
    return {
        'x_collinear': (lined, [[5, 6, 7]] + draws),
        'coincident': (base, [[9, 9, 9]] + draws),
        'same_twice': (base, [draws[0], draws[0]]),          # a tie: the later trial wins, with the same result
        'zero_first': (degenerate, [special, floor_triple(degenerate)]),
    }


EXPLICIT = _explicit
SAMPLER_SIZES = (3, 4, 7, 255, 299, 300, 301, 302, 1000, 70000, 5000000)
