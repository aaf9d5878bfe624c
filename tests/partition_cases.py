"""Case builders and float64 references for the partition kernels of csrc/spg_spgraph.hip (compute_geof, compute_sp_graph,
prune) at their degenerate and scale edges.  Plain module (no test in it): tests/test_partition_cases.py checks on the CPU that
every builder reaches the branch it claims, tests/test_gpu_partition_edges.py runs the device against the references.

Every case is generated from a seed or written out by hand.  The constructed ("exact") cases use coordinates that are small
integer multiples of a power of two: the float32 inputs, their float64 sums and their means are then exact, so a degenerate
neighbourhood is degenerate in both implementations (all neighbours on the point: 0/0, NaN on both sides).

Every bound below is derived from the float64 / float32 formats and first-order perturbation of the reference, never from what
the device returns."""
import functools

import numpy as np

from oracle import spg_partition_oracle as P

EPS64 = float(np.finfo(np.float64).eps)      # 2^-52
EPS32 = float(np.finfo(np.float32).eps)      # 2^-23 (one ulp of a value in [1, 2))


def ulp32(v):
    """One float32 ulp at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# =====================================================================================================================
# compute_geof
# =====================================================================================================================
GEOF_ATOL = 2e-5      # the project's existing tolerance (tests/test_gpu_spgraph.py::test_compute_geof_vs_restatement)

# Conditioning mask of the verticality.  Verticality is sum_i lambda_i |v_i| (normalised): it depends on the eigenVECTORS, and
# the eigenvectors of a pair (i, j) turn by about ||dC|| / |lambda_i - lambda_j| when the covariance is perturbed by dC
# (Davis-Kahan, first order).  The device forms the covariance in one pass, E[d d^T] - E[d] E[d]^T on offsets d from the point:
# with the point inside its own neighbourhood E|d|^2 <= (k + 1) tr C <= 3 (k + 1) lambda_0 at worst and ~ a few lambda_0
# typically, so ||dC|| is a small multiple of eps64 k r^2: ~1e-16 * 150 * 10 lambda_0 ~ 1.5e-13 lambda_0 typically and
# 3 k (k + 1) eps64 lambda_0 ~ 7.5e-12 lambda_0 in the worst case (k = 150); the reference's two-pass form is no worse.  A turn
# of ||dC|| / gap moves the verticality by at most about that much (weights lambda_i / lambda_0 <= 1), so with a relative gap
# of at least g the two sides differ by <= 7.5e-12 / g: far below the absolute tolerance 2e-5 for every g >= ~1e-9 (and still
# 7.5e-6 < 2e-5 at g = 1e-6 under the worst-case bound).  From above, g is limited by how many points may be masked: in a random
# cloud the share of points with a relative eigenvalue gap below g is of the order of g, and at most 0.1 % may be masked:
# g <= ~1e-4.  Any g in [1e-9, 1e-4] serves; 1e-6 sits in the middle.  A pair of eigenvalues that are BOTH below g lambda_0
# carries no weight in sum lambda |v| (<= 2 g of the result) and does not mask the point.
GEOF_GAP = 1e-6


def geof_reference_eigenvalues(xyz, target, k_nn):
    """Descending float64 eigenvalues [n,3] of the (k_nn + 1)-neighbourhood covariance, formed exactly as
    oracle.spg_partition_oracle.geof forms it (the mask is a condition on the INPUTS: reference values only)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = xyz.shape[0]
    nb = np.concatenate((np.arange(n)[:, None], np.asarray(target, dtype=np.int64).reshape(n, k_nn)), axis=1)
    cen = xyz[nb] - xyz[nb].mean(1, keepdims=True)
    cov = np.einsum('nki,nkj->nij', cen, cen) / (k_nn + 1)
    return np.maximum(np.linalg.eigvalsh(cov)[:, ::-1], 0.0)


def verticality_mask(lam, g=GEOF_GAP):
    """True where the verticality is compared: no pair i < j with |lam_i - lam_j| < g lam_0 while max(lam_i, lam_j) >= g lam_0."""
    lam = np.asarray(lam, dtype=np.float64)
    floor = g * lam[:, 0]
    ok = np.ones(len(lam), dtype=bool)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        close = np.abs(lam[:, i] - lam[:, j]) < floor
        weighty = np.maximum(lam[:, i], lam[:, j]) >= floor
        ok &= ~(close & weighty)
    return ok & (lam[:, 0] > 0)


def _knn_target(xyz, k):
    from scipy.spatial import cKDTree
    if k == 0:
        return np.zeros(0, dtype=np.uint32)
    _, nb = cKDTree(xyz).query(xyz, k + 1)
    nb = nb.reshape(len(xyz), k + 1)
    own = nb == np.arange(len(xyz))[:, None]                  # drop the point itself (a duplicate may sort in front of it)
    own[~own.any(1), 0] = True
    keep = ~(own & (np.cumsum(own, 1) == 1))
    return nb[keep].reshape(len(xyz), k).astype(np.uint32).reshape(-1)


def _random_cloud(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * rng.uniform(0.3, 3.0, 3)).astype(np.float32)


def _two_slabs(seed, n):
    rng = np.random.default_rng(seed)
    return np.concatenate((rng.normal(size=(n // 2, 3)) * [4, 4, 0.05],
                           rng.normal(size=(n - n // 2, 3)) * [0.05, 3, 3] + [8, 0, 0])).astype(np.float32)


def _window_targets(shape, half):
    """Neighbour lists on a regular index grid: all offsets within `half` per axis (the point itself left out), indices clamped
    at the border -- so border points get REPEATED neighbours and, clamped onto themselves, THEMSELVES as neighbours."""
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, len(shape))
    offs = np.stack(np.meshgrid(*[np.arange(-h, h + 1) for h in half], indexing='ij'), -1).reshape(-1, len(shape))
    offs = offs[np.any(offs != 0, 1)]
    nb = np.clip(grids[:, None, :] + offs[None, :, :], 0, np.asarray(shape) - 1)
    flat = np.ravel_multi_index(tuple(nb[..., d] for d in range(len(shape))), shape)
    return grids, flat.astype(np.uint32).reshape(-1), len(offs)


@functools.lru_cache(maxsize=None)
def geof_cases():
    """-> list of dicts {name, xyz f32 [n,3], target u32 [n k], k_nn, kind} in the order they are to be run: every case with
    k_nn < 64 (dynamic LDS below 64 KB) before the first with k_nn >= 64.
    kind: 'random' (mask share <= 0.1 %), 'exact' (constructed, well defined: nothing masked), 'isotropic' (all eigenvalues
    equal: exists for linearity / planarity / scattering), 'nan' (no spread at all: every feature 0/0)."""
    cases = []

    def add(name, xyz, target, k, kind):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        target = np.ascontiguousarray(target, dtype=np.uint32).reshape(-1)
        assert target.size == len(xyz) * k and (target.size == 0 or target.max() < len(xyz)), name
        cases.append({'name': name, 'xyz': xyz, 'target': target, 'k_nn': k, 'kind': kind})

    # ---- no neighbour at all / a single point: covariance exactly zero ----
    add('n1_k0', [[1.5, -2.25, 3.0]], [], 0, 'nan')
    add('n1_k2_self', [[1.5, -2.25, 3.0]], [0, 0], 2, 'nan')                       # its own neighbour, twice
    add('n256_k0', _random_cloud(20, 256), [], 0, 'nan')
    # ---- random clouds around the workgroup size (256) and the small k_nn ----
    for seed, (n, k) in enumerate(((255, 1), (256, 2), (257, 2), (255, 45), (256, 45), (257, 45), (255, 63), (257, 63))):
        xyz = _random_cloud(100 + seed, n)
        add(f'random_n{n}_k{k}', xyz, _knn_target(xyz, k), k, 'random')
    xyz = _two_slabs(3, 50_000)
    add('slabs_n50000_k45', xyz, _knn_target(xyz, 45), 45, 'random')
    # ---- a large common offset: float32 spacing 2^-7 at 1e5; the spread (std 5) keeps the points distinct ----
    rng = np.random.default_rng(31)
    xyz = (rng.normal(size=(5000, 3)) * [5, 4, 2] + [1e5, -2e5, 5e4]).astype(np.float32)
    add('shifted_1e5_n5000_k45', xyz, _knn_target(xyz, 45), 45, 'random')
    # ---- neighbour lists with repeats and with the point itself ----
    xyz = _random_cloud(41, 1000)
    tgt = _knn_target(xyz, 45).reshape(1000, 45).copy()
    tgt[:, 5:12] = tgt[:, 4:5]                                                     # one neighbour eight times
    tgt[::2, 20] = np.arange(0, 1000, 2)                                           # the point itself
    tgt[::3, 30:33] = np.arange(0, 1000, 3)[:, None]                               # ... three times
    add('repeats_and_self_n1000_k45', xyz, tgt, 45, 'random')
    # ---- all neighbours coincident with the point (0/0): 100 copies of one point inside an ordinary cloud ----
    xyz = _random_cloud(42, 300)
    xyz[:100] = [2.5, -1.25, 0.75]
    tgt = _knn_target(xyz[100:], 12).reshape(200, 12) + 100
    tgt = np.concatenate((np.random.default_rng(43).integers(0, 100, (100, 12)), tgt))
    add('coincident_block_n300_k12', xyz, tgt, 12, 'random')
    xyz = np.tile(np.array([[-3.5, 0.125, 1024.0]], np.float32), (257, 1))
    add('all_coincident_n257_k45', xyz, np.random.default_rng(44).integers(0, 257, 257 * 45), 45, 'nan')
    # ---- exactly collinear: i * (1, 2, -1) / 4, window of +-4 along the line (clamped: repeats and self at the ends) ----
    grid, tgt, k = _window_targets((300,), (4,))
    add('collinear_n300_k8', grid[:, :1] * np.array([[0.25, 0.5, -0.25]]) + [1.0, -2.0, 0.5], tgt, k, 'exact')
    # ---- exactly coplanar: a * (1, 0, 1) / 4 + b * (0, 1, 2) / 4, window 7 x 3 (two distinct in-plane eigenvalues) ----
    grid, tgt, k = _window_targets((24, 16), (3, 1))
    add('coplanar_n384_k20', grid[:, :1] * np.array([[0.25, 0.0, 0.25]]) + grid[:, 1:] * np.array([[0.0, 0.25, 0.5]]) - [2.0, 1.0, 0.0],
        tgt, k, 'exact')
    # ---- exactly isotropic: cubic lattice, the six axis neighbours (interior points: covariance (2 h^2 / 7) I) ----
    grid = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing='ij'), -1).reshape(-1, 3)
    offs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    nb = np.clip(grid[:, None, :] + offs[None], 0, 6)
    add('isotropic_lattice_n343_k6', grid * 0.5 - 1.5, np.ravel_multi_index((nb[..., 0], nb[..., 1], nb[..., 2]), (7, 7, 7)), 6, 'isotropic')
    # ---- k_nn >= 64: more than 64 KB of dynamic LDS (256 x (k_nn + 1) words); 150 is the library's limit ----
    for seed, (n, k) in enumerate(((257, 64), (256, 100), (255, 150), (257, 150))):
        xyz = _random_cloud(200 + seed, n)
        add(f'random_n{n}_k{k}', xyz, _knn_target(xyz, k), k, 'random')
    xyz = _two_slabs(5, 50_000)
    add('slabs_n50000_k64', xyz, _knn_target(xyz, 64), 64, 'random')
    xyz = _two_slabs(6, 50_000)
    add('slabs_n50000_k150', xyz, _knn_target(xyz, 150), 150, 'random')
    first_big = min(i for i, c in enumerate(cases) if c['k_nn'] >= 64)
    assert all(c['k_nn'] >= 64 for c in cases[first_big:])
    return cases


def geof_reference(case):
    """-> (ref f32 [n,4] from the project's restatement, compare bool [n,4]).  Linearity / planarity / scattering are compared
    wherever s0 > 0, verticality where verticality_mask allows; where the reference is NaN the device must be NaN too."""
    ref = P.geof(case['xyz'], case['target'], case['k_nn'])
    lam = geof_reference_eigenvalues(case['xyz'], case['target'], case['k_nn'])
    cmp = np.zeros(ref.shape, dtype=bool)
    cmp[:, :3] = (lam[:, 0] > 0)[:, None]
    cmp[:, 3] = verticality_mask(lam)
    cmp &= ~np.isnan(ref)
    return ref, cmp


def geof_measure(dev, case):
    """Figures of one device result against the reference: dict with the NaN-pattern agreement, the worst absolute error per
    feature on the comparable entries and the share of points masked from the verticality."""
    ref, cmp = geof_reference(case)
    err = np.where(cmp, np.abs(dev.astype(np.float64) - ref.astype(np.float64)), 0.0)
    n = len(ref)
    return {'nan_equal': bool(np.array_equal(np.isnan(dev), np.isnan(ref))), 'worst': err.max(0) if n else np.zeros(4),
            'masked': float(1.0 - cmp[:, 3].mean()) if n else 0.0, 'nan_rows': int(np.isnan(ref).any(1).sum())}


# =====================================================================================================================
# compute_sp_graph: superpoints
# =====================================================================================================================
# Perturbation of the eigenvalues between two correct float64 implementations (the device: two-pass moments summed over 64 lanes
# and a butterfly, cyclic Jacobi; the reference: np.cov + eigvalsh).  A sum of m terms in blocks (64 lanes / numpy's pairwise
# blocks) carries at most (m / 64 + 6) eps64 of sum |terms| <= ev0 (m - 1) per covariance entry -- <= 70 eps64 ev0 for the
# m <= 4096 of these tests --, for each of the two implementations; a symmetric 3 x 3 perturbation moves an eigenvalue by at most
# its 2-norm <= 3 max |entry| (Weyl); both eigen-solvers are backward stable to ~20 eps64 ||C||.  3 (70 + 70) + 40 < 512.
C_EIG = 512
SP_MAX_UNIQUE = 4096


def superpoint_features_f64(xyz, comp, n_com):
    """float64 restatement of the superpoint features of graphs.py:141-172 from the published expressions:
    -> dict {centroid [n_com,3], length, surface, volume [n_com], ev [n_com,3] (descending, zeros outside the general branch),
    n_unique [n_com], count [n_com], scale [n_com] (max |coordinate| of the component)}.
    0 points: zeros (what the kernel documents); 1 unique point: the point, zeros; 2 unique points: mean, sqrt(sum var);
    otherwise np.cov of the unique points (divisor m - 1), eigvalsh, sqrt(ev0 ev1 + 1e-10), sqrt(ev0 ev1 ev2 + 1e-10)."""
    xyz = np.asarray(xyz)
    comp = np.asarray(comp).astype(np.int64)
    order = np.argsort(comp, kind='stable')
    bounds = np.searchsorted(comp[order], np.arange(n_com + 1))
    out = {'centroid': np.zeros((n_com, 3)), 'length': np.zeros(n_com), 'surface': np.zeros(n_com), 'volume': np.zeros(n_com),
           'ev': np.zeros((n_com, 3)), 'n_unique': np.zeros(n_com, dtype=np.int64), 'count': np.diff(bounds),
           'scale': np.zeros(n_com)}
    for c in range(n_com):
        rows = xyz[order[bounds[c]:bounds[c + 1]]]
        if len(rows) == 0:
            continue
        pts = np.unique(rows, axis=0).astype(np.float64)                 # (== on the float32 rows: -0.0 and +0.0 are one value)
        out['n_unique'][c] = len(pts)
        out['scale'][c] = np.abs(pts).max()
        out['centroid'][c] = pts.mean(0)
        if len(pts) == 2:
            out['length'][c] = np.sqrt(np.sum(np.var(pts, axis=0)))
        elif len(pts) > 2:
            ev = np.maximum(np.linalg.eigvalsh(np.cov(pts.T))[::-1], 0.0)
            out['ev'][c] = ev
            out['length'][c] = ev[0]
            out['surface'][c] = np.sqrt(ev[0] * ev[1] + 1e-10)
            out['volume'][c] = np.sqrt(ev[0] * ev[1] * ev[2] + 1e-10)
    return out


def superpoint_bounds(f):
    """Per-component bounds on |device - superpoint_features_f64| -> dict {centroid, length, surface, volume} [n_com].
    General branch: every eigenvalue is known to d = C_EIG eps64 ev0; first order through the published expressions,
      length = ev0:                          d
      surface = sqrt(ev0 ev1 + 1e-10):       d (ev0 + ev1) / (2 surface)
      volume = sqrt(ev0 ev1 ev2 + 1e-10):    d (ev1 ev2 + ev0 ev2 + ev0 ev1) / (2 volume)
    plus two float32 ulps of the value (one rounding to float32 on each side, and the two may straddle a rounding boundary).
    Two unique points: the kernel (like the reference) evaluates mean and variance in float32: the mean (u + v) / 2 is rounded
    to eps32 / 2 of max |coordinate| per axis and enters u - mean, v - mean absolutely; three axes in quadrature and the rounding
    of the squares, sums and root give  length: 2 eps32 scale + 4 eps32 length.  The centroid is one float32 rounding of the
    float64 mean (general branch) or of (u + v) / 2: two ulps at the component's largest coordinate.  0 / 1 unique points: exact."""
    assert f['n_unique'].max() <= SP_MAX_UNIQUE
    ev = f['ev']
    d = C_EIG * EPS64 * ev[:, 0]
    b = {'centroid': np.where(f['n_unique'] > 1, 2 * ulp32(f['scale']), 0.0)}
    b['length'] = d + 2 * ulp32(f['length'])
    b['surface'] = d * (ev[:, 0] + ev[:, 1]) / (2 * np.maximum(f['surface'], 1e-5)) + 2 * ulp32(f['surface'])
    b['volume'] = d * (ev[:, 1] * ev[:, 2] + ev[:, 0] * ev[:, 2] + ev[:, 0] * ev[:, 1]) / (2 * np.maximum(f['volume'], 1e-5)) + 2 * ulp32(f['volume'])
    two = f['n_unique'] == 2
    b['length'] = np.where(two, 2 * EPS32 * f['scale'] + 4 * EPS32 * f['length'], b['length'])
    few = f['n_unique'] < 2
    for k in ('length', 'surface', 'volume'):
        b[k] = np.where(few | (two & (k != 'length')), 0.0, b[k])
    return b


def superpoint_measure(g, xyz, comp, n_com):
    """Per-element figures of a device (or oracle) result dict against superpoint_features_f64:
    -> {feature: (worst absolute error, worst error / bound, index of the worst component)}; error / bound is 0 where both are 0
    and inf where the bound is 0 and the error is not."""
    f = superpoint_features_f64(xyz, comp, n_com)
    b = superpoint_bounds(f)
    out = {}
    for key, name in (('sp_centroids', 'centroid'), ('sp_length', 'length'), ('sp_surface', 'surface'), ('sp_volume', 'volume')):
        a = np.asarray(g[key], dtype=np.float64)
        ref = f[name]
        if name != 'centroid':
            a = a.reshape(-1)
            if name in ('surface', 'volume'):      # 0 / 1 / 2 unique points and empty components: exactly 0, as graphs.py leaves them
                ref = np.where(f['n_unique'] > 2, ref, 0.0)
        err = np.abs(a - ref)
        bound = b[name] if name != 'centroid' else b[name][:, None]
        err, bound = np.broadcast_arrays(err, bound)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isnan(a) if a.shape == ratio.shape else False, np.inf, ratio)
        worst = int(np.argmax(ratio.reshape(len(ratio), -1).max(1))) if ratio.size else -1
        out[name] = (float(err.max()) if err.size else 0.0, float(ratio.max()) if ratio.size else 0.0, worst)
    return out


def _explicit_edges(pairs):
    """Tetrahedra that produce exactly the given vertex pairs: (a, b, b, b) -- its six pairs are (a, b) three times and (b, b)
    three times (never an interface pair)."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return np.stack((pairs[:, 0], pairs[:, 1], pairs[:, 1], pairs[:, 1]), 1)


@functools.lru_cache(maxsize=None)
def superpoint_cases():
    """-> list of dicts {name, xyz, comp (int64), n_com, labels (1-D int64), n_labels, tets (int32 [T,4]), d_max, claims}.
    `claims`: component id -> what it is built to be (checked by tests/test_partition_cases.py)."""
    rng = np.random.default_rng(2024)
    parts, claims = [], {}

    def comp_add(cid, pts, what):
        parts.append((cid, np.asarray(pts, dtype=np.float32).reshape(-1, 3)))
        claims[cid] = what

    one = np.array([[4.0, -3.5, 2.25]])
    comp_add(0, np.repeat(one, 40, 0), 'copies_of_one_point')
    comp_add(1, np.concatenate((np.repeat([[6.0, 1.5, -2.0]], 5, 0), np.repeat([[6.5, 1.25, -2.0]], 7, 0))), 'two_points_with_copies')
    comp_add(2, [[-6.0, 2.0, 1.0], [-5.5, 2.5, 1.0], [-6.0, 2.25, 1.75]], 'three_points')
    comp_add(3, np.arange(20)[:, None] * np.array([[0.5, 0.25, -0.75]]) + [10.0, 10.0, 0.0], 'collinear')
    a, b = np.meshgrid(np.arange(6), np.arange(5), indexing='ij')
    comp_add(4, a.reshape(-1, 1) * np.array([[0.5, 0.0, 0.25]]) + b.reshape(-1, 1) * np.array([[0.0, 0.25, 0.5]]) + [-10.0, 8.0, 1.0], 'coplanar')
    comp_add(5, [[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [3.0, 1.0, 2.0], [3.0, 1.0, 2.0]], 'signed_zero_two_unique')
    comp_add(6, [[1.0, -0.0, 7.0], [1.0, 0.0, 5.0], [1.0, 0.0, 7.0], [2.0, 0.5, -0.0], [2.0, 0.5, 0.0], [0.5, 3.0, 6.0], [-1.0, 2.0, 4.0]],
             'signed_zero_five_unique')
    for cid, m in ((7, 65), (8, 128), (9, 129)):                                   # straddling the 64-lane stride; two duplicates each
        pts = (rng.normal(size=(m, 3)) * [1.0, 0.6, 0.3] + rng.uniform(-8, 8, 3)).astype(np.float32)
        comp_add(cid, np.concatenate((pts, pts[:2])), f'unique_{m}')
    # id 10 stays unused: an empty segment inside the id range
    thin = rng.normal(size=(30, 3)) * [5e-3, 3e-3, 1e-3] + [1.0, 1.0, 1.0]          # volume and surface far below everyone else's
    comp_add(11, thin, 'thin_small')
    comp_add(12, rng.normal(size=(600, 3)) * [6.0, 5.0, 4.0], 'large_blob')         # sets max |ref| of every array
    comp_add(13, [[20.0, 20.0, 20.0]], 'single_point')
    comp_add(14, np.repeat(rng.normal(size=(64, 3)), 2, 0) * [0.5, 0.5, 0.5] + [-4.0, -4.0, 3.0], 'unique_64_each_twice')
    # id 15 stays unused as well: a trailing empty component, n_com = max(comp) + 2
    xyz = np.concatenate([p for _, p in parts])
    comp = np.concatenate([np.full(len(p), cid) for cid, p in parts]).astype(np.int64)
    perm = rng.permutation(len(xyz))
    xyz, comp = np.ascontiguousarray(xyz[perm]), comp[perm]
    n = len(xyz)
    n_com = 16
    # tetrahedra given explicitly: random quadruples (most of them join two to four components) and one explicit edge from every
    # small component to the large blob, so that every non-empty component has a superedge
    tets = rng.integers(0, n, (1500, 4)).astype(np.int32)
    blob = np.flatnonzero(comp == 12)
    link = [(int(np.flatnonzero(comp == c)[0]), int(blob[i])) for i, c in enumerate(sorted(claims)) if c != 12]
    tets = np.concatenate((tets, _explicit_edges(link)))
    n_labels = 5
    labels = rng.integers(0, n_labels + 1, n).astype(np.int64)                     # 1-D labels; outside [0, n_labels]: dropped
    labels[rng.choice(n, 60, replace=False)] = np.tile([n_labels + 1, 200, -1], 20)
    base = {'xyz': xyz, 'comp': comp, 'n_com': n_com, 'labels': labels, 'n_labels': n_labels, 'tets': tets, 'claims': claims}
    cases = [dict(base, name='branches_gaps_dmax0', d_max=0.0), dict(base, name='branches_gaps_dmax6', d_max=6.0)]
    # the same cloud without the id gaps and without labels, through the reference's own signature
    _, dense = np.unique(comp, return_inverse=True)
    cases.append(dict(base, name='branches_dense_nolabels', comp=dense.astype(np.int64), n_com=int(dense.max()) + 1, labels=np.zeros(0, np.int64),
                      n_labels=0, d_max=0.0, claims={i: claims[c] for i, c in enumerate(sorted(claims))}))
    return cases


# =====================================================================================================================
# compute_sp_graph: superedges
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def superedge_cases():
    """-> list of dicts like superpoint_cases() plus `expect`: {(source, target): number of Delaunay edges} for the hand-built
    ones (checked on the CPU against the oracle's own grouping)."""
    cases = []
    # ---- hand-built: exact coordinates (multiples of 1/4), components A = 0, B = 1, C = 2, D = 3 ----
    rng = np.random.default_rng(77)
    A = np.array([10.5, -2.25, 7.0]) + rng.integers(-8, 9, (40, 3)) * 0.25
    B = np.array([30.0, 4.0, -5.0]) + rng.integers(-8, 9, (40, 3)) * 0.25
    C = np.array([-20.0, 0.5, 12.0]) + rng.integers(-8, 9, (150, 3)) * 0.25
    D = np.array([0.0, 40.0, 0.0]) + rng.integers(-8, 9, (150, 3)) * 0.25
    xyz = np.concatenate((A, B, C, D)).astype(np.float32)
    comp = np.repeat(np.arange(4), (40, 40, 150, 150)).astype(np.int64)
    iA, iB, iC, iD = 0, 40, 80, 230
    pairs = [(iA, iB)]                                                             # A-B: exactly ONE edge (std = 0 branch)
    pairs += [(iA + i, iC + i) for i in range(40)] + [(iA + i, iC + 40 + i) for i in range(24)]       # A-C: exactly 64
    pairs += [(iB + i, iC + i) for i in range(40)] + [(iB + i, iC + 60 + i) for i in range(25)]       # B-C: exactly 65
    pairs += [(iC + i, iD + i) for i in range(129)]                                                   # C-D: exactly 129
    tets = np.concatenate((_explicit_edges(pairs),
                           np.array([[iA + 1, iA + 2, iD + 140, iD + 141], [iB + 3, iB + 4, iD + 142, iD + 143]], np.int32)))   # real tetrahedra: 4 edges each
    expect = {(0, 1): 1, (0, 2): 64, (1, 2): 65, (2, 3): 129, (0, 3): 4, (1, 3): 4}
    expect.update({(t, s): c for (s, t), c in list(expect.items())})
    base = {'xyz': xyz, 'comp': comp, 'n_com': 4, 'labels': np.zeros(0, np.int64), 'n_labels': 0, 'tets': tets}
    for d_max in (0.0, -1.0):
        cases.append(dict(base, name=f'handbuilt_counts_dmax{d_max:g}', d_max=d_max, expect=expect))
    # ---- an edge whose float32 length equals d_max exactly: 3-4-5 offsets on exact coordinates ----
    p = np.array([10.5, -2.25, 7.0])
    xyz = np.array([p, p + [3, 4, 0], p + [0, -3, 4], p + [4, 0, 3],               # 0 | 1, 2, 3: three edges of length exactly 5
                    p + [1.5, 2.0, 0], p + [0, 6, 8], p + [3, 4, 0.25]], np.float32)   # 4: length 2.5; 5: length 10; 6: just above 5
    comp = np.array([0, 1, 1, 2, 2, 1, 2], dtype=np.int64)
    tets = np.array([[0, 1, 2, 3], [0, 4, 5, 6]], np.int32)
    # forty more points in each of the components 1 and 2, in no tetrahedron: full-rank components (three points alone have a
    # third eigenvalue of pure round-off, and sp_volume = sqrt(ev0 ev1 ev2 + 1e-10) of nothing but such components is ill-conditioned)
    more = np.concatenate((p + [2.0, 3.0, 4.0] + rng.integers(-16, 17, (40, 3)) * 0.25, p + [3.0, 1.0, 2.0] + rng.integers(-16, 17, (40, 3)) * 0.25))
    xyz = np.concatenate((xyz, more.astype(np.float32)))
    comp = np.concatenate((comp, np.repeat([1, 2], 40)))
    base = {'xyz': xyz, 'comp': comp, 'n_com': 3, 'labels': np.zeros(0, np.int64), 'n_labels': 0, 'tets': tets}
    five_up = float(np.nextafter(np.float32(5.0), np.float32(np.inf)))
    cases.append(dict(base, name='length_equals_dmax_5', d_max=5.0, expect_edges_from_0={4}))                  # strict <: the 5s go
    cases.append(dict(base, name='length_equals_dmax_next', d_max=five_up, expect_edges_from_0={1, 2, 3, 4}))  # one ulp more: they stay
    cases.append(dict(base, name='length_equals_dmax_0', d_max=0.0, expect_edges_from_0={1, 2, 3, 4, 5, 6}))
    cases.append(dict(base, name='length_equals_dmax_neg', d_max=-1.0, expect_edges_from_0={1, 2, 3, 4, 5, 6}))
    # ---- scipy's triangulation of a labelled synthetic cloud next to them ----
    from scipy.spatial import Delaunay
    xyz, comp, components, labels = P.synthetic_cloud(21, n=4000, n_blobs=30, duplicates=40)
    tets = Delaunay(xyz).simplices.astype(np.int32)
    base = {'xyz': xyz, 'comp': comp, 'n_com': int(comp.max()) + 1, 'labels': labels.astype(np.int64), 'n_labels': 5, 'tets': tets}
    for d_max in (0.9, 0.0, -1.0):
        cases.append(dict(base, name=f'delaunay_n{len(xyz)}_dmax{d_max:g}', d_max=d_max))
    return cases


def sp_graph_reference(case):
    """The pinned CPU oracle P.sp_graph_after_triangulation on a case.  The oracle (like the reference) cannot walk an EMPTY
    component, so component ids are compacted for it and its rows scattered back: empty components have zero features, no
    superedge, and the order of the superedges (by source * n_com + target) does not change under a monotone renumbering."""
    comp, n_com = case['comp'], case['n_com']
    used, dense = np.unique(comp, return_inverse=True)
    components = [np.flatnonzero(dense == c) for c in range(len(used))]
    g = P.sp_graph_after_triangulation(case['xyz'], case['d_max'], dense, components, case['labels'], case['n_labels'], case['tets'])
    if len(used) == n_com:
        return g
    out = dict(g)
    for k, v in g.items():
        if k.startswith('sp_') and isinstance(v, np.ndarray):
            full = np.zeros((n_com,) + v.shape[1:], dtype=v.dtype)
            full[used] = v
            out[k] = full
    out['source'] = used[g['source'].astype(np.int64)].astype(np.uint32)
    out['target'] = used[g['target'].astype(np.int64)].astype(np.uint32)
    return out


def superedge_stats_f64(case):
    """float64 offset statistics of every superedge, grouped as the oracle groups them -> dict {source, target, count,
    mean [S,3], std [S,3], norm [S], dmax [S] (largest |offset component| of the group)}.  The offsets themselves are the float32
    differences of graphs.py:193 (delta is a float32 array in the reference; the kernel subtracts in float32 too)."""
    xyz, comp, n_com = case['xyz'], case['comp'], case['n_com']
    edges = P.interface_edges(case['tets'], comp, xyz, case['d_max'])
    ec = comp[edges]
    index = n_com * ec[0].astype(np.int64) + ec[1]
    order = np.argsort(index, kind='stable')
    edges, index = edges[:, order], index[order]
    starts = np.flatnonzero(np.r_[True, index[1:] != index[:-1]]) if index.size else np.zeros(0, dtype=np.int64)
    bounds = np.r_[starts, index.size]
    S = len(starts)
    out = {'source': index[starts] // n_com, 'target': index[starts] % n_com, 'count': np.diff(bounds), 'mean': np.zeros((S, 3)),
           'std': np.zeros((S, 3)), 'norm': np.zeros(S), 'dmax': np.zeros(S)}
    delta = (xyz[edges[0]] - xyz[edges[1]]).astype(np.float32)
    norm32 = np.sqrt((delta ** 2).sum(1, dtype=np.float32))                       # one float32 norm per edge (:197), averaged in float64
    for s in range(S):
        d = delta[bounds[s]:bounds[s + 1]].astype(np.float64)
        out['mean'][s] = d.mean(0)
        out['std'][s] = d.std(0) if len(d) > 1 else 0.0
        out['norm'][s] = norm32[bounds[s]:bounds[s + 1]].astype(np.float64).mean()
        out['dmax'][s] = np.abs(d).max()
    return out


def superedge_bounds(st):
    """Per-superedge bounds on |device - superedge_stats_f64|.  Both sides sum the same float32 offsets in float64: a sum of c
    terms carries at most c eps64 of c max|d|, the mean c eps64 max|d| =: e.  The variance of the two-pass form is then known to
    dv = 4 e max|d| (first order in e, |d - mean| <= 2 max|d|), and |sqrt(a) - sqrt(b)| <= min(|a - b| / (2 sqrt(a)), sqrt|a - b|).
    Plus two float32 ulps of the value for the final rounding on each side.  One edge: the offset itself, std exactly 0."""
    c = st['count'].astype(np.float64)
    e = (c + 8) * EPS64 * st['dmax']
    dv = 4 * e * st['dmax']
    with np.errstate(divide='ignore', invalid='ignore'):
        dstd = np.minimum(np.where(st['std'] > 0, dv[:, None] / (2 * st['std']), np.inf), np.sqrt(dv)[:, None])
    single = (st['count'] == 1)
    return {'mean': np.where(single, 0.0, e)[:, None] + np.where(single[:, None], 0.0, 2 * ulp32(st['mean'])),
            'std': np.where(single[:, None], 0.0, dstd + 2 * ulp32(st['std'])),
            'norm': np.where(single, 0.0, np.sqrt(3) * e + 2 * ulp32(st['norm']))}


def superedge_measure(g, case):
    """-> {feature: (worst absolute error, worst error / bound)} of se_delta_mean / std / norm against the float64 statistics."""
    st = superedge_stats_f64(case)
    assert np.array_equal(np.asarray(g['source']).reshape(-1), st['source']) and np.array_equal(np.asarray(g['target']).reshape(-1), st['target'])
    b = superedge_bounds(st)
    out = {}
    for key, name in (('se_delta_mean', 'mean'), ('se_delta_std', 'std'), ('se_delta_norm', 'norm')):
        a = np.asarray(g[key], dtype=np.float64).reshape(st[name].shape)
        err = np.abs(a - st[name])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(err == 0, 0.0, err / b[name])
        ratio = np.where(np.isnan(a), np.inf, ratio)
        out[name] = (float(err.max()) if err.size else 0.0, float(ratio.max()) if ratio.size else 0.0)
    return out


def ratio_rows_from_own_features(g):
    """se_*_ratio and se_delta_centroid recomputed from the result's OWN superpoint features with the float32 / float64
    expressions of graphs.py:186-190 -> dict of arrays that must be bit-equal to the result's rows."""
    s, t = np.asarray(g['source']).reshape(-1).astype(np.int64), np.asarray(g['target']).reshape(-1).astype(np.int64)
    one = np.float32(1e-6)
    out = {'se_delta_centroid': g['sp_centroids'][s] - g['sp_centroids'][t]}
    for k in ('length', 'surface', 'volume'):
        v = np.asarray(g[f'sp_{k}'], dtype=np.float32)
        out[f'se_{k}_ratio'] = v[s] / (v[t] + one)
    pc = np.asarray(g['sp_point_count']).astype(np.float64)
    out['se_point_count_ratio'] = (pc[s] / (pc[t] + 1e-6)).astype(np.float32)
    return out


# =====================================================================================================================
# prune
# =====================================================================================================================
PRUNE_VOXEL = 0.25


@functools.lru_cache(maxsize=None)
def prune_cases():
    """-> list of dicts {name, xyz, voxel, rgb, labels (uint8), objects (uint32), n_labels, n_objects}.  Coordinates are integer
    multiples of voxel / 2 (voxel = 0.25): half of them lie exactly ON a voxel face, and every division is exact."""
    cases = []

    def add(name, xyz, rgb, labels, objects, n_labels, n_objects):
        cases.append({'name': name, 'xyz': np.ascontiguousarray(xyz, dtype=np.float32), 'voxel': PRUNE_VOXEL,
                      'rgb': np.ascontiguousarray(rgb, dtype=np.uint8), 'labels': np.ascontiguousarray(labels, dtype=np.uint8),
                      'objects': np.ascontiguousarray(objects, dtype=np.uint32), 'n_labels': n_labels, 'n_objects': n_objects})

    add('n1', [[3.125, -7.5, 0.25]], [[255, 255, 255]], [8], [40], 8, 40)
    # the known answer of tests/test_partition_cases.py: points on faces, a -0.0 minimum along x, saturated colours, upper-bound ids
    add('on_face_known_answer', [[0.0, 0.5, -1.0], [-0.0, 0.5, -1.0], [0.25, 0.5, -1.0], [0.125, 0.625, -0.875], [0.375, 0.5, -0.75],
                                 [0.5, 0.75, -1.0], [0.25, 0.5, -0.875]],
        np.full((7, 3), 255), [2, 2, 0, 2, 1, 2, 2], [3, 0, 3, 3, 3, 1, 3], 2, 3)
    for name, n, span, seed in (('n262143', 262_143, 128, 1), ('n262144', 262_144, 128, 2), ('n1000000', 1_000_000, 80, 3)):
        rng = np.random.default_rng(seed)
        xyz = (rng.integers(0, span, (n, 3)) * (PRUNE_VOXEL / 2)).astype(np.float32)
        xyz[:, 0] = np.where(xyz[:, 0] == 0, np.float32(-0.0), xyz[:, 0])         # the minimum along x is -0.0 (and only -0.0)
        xyz[:, 1] -= np.float32(5.0)                                               # an ordinary negative minimum along y
        xyz[rng.integers(0, n, 50), 2] = np.float32(-0.0)                          # both zeros along z
        rgb = rng.integers(0, 256, (n, 3))
        rgb[rng.random(n) < 0.5] = 255
        labels = rng.integers(0, 9, n)
        labels[rng.random(n) < 0.3] = 8                                            # == n_labels
        objects = rng.integers(0, 41, n)
        objects[rng.random(n) < 0.3] = 40                                          # == n_objects
        add(name, xyz, rgb, labels, objects, 8, 40)
    # 262 144 points in eight voxels, every colour saturated: 32 768 points per voxel, colour sums 255 * 32 768 < 2^24 (exact)
    rng = np.random.default_rng(4)
    xyz = (rng.integers(0, 4, (262_144, 3)) * (PRUNE_VOXEL / 2)).astype(np.float32)
    add('n262144_eight_voxels_saturated', xyz, np.full((262_144, 3), 255), np.full(262_144, 8), np.full(262_144, 40), 8, 40)
    return cases
