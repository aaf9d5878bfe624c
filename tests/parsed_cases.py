"""The scenes of the parsed-superpoint tests (tests/test_parsed_restatement.py, tests/test_gpu_parsed.py,
tools/gen_parsed_golden.py): seeded and small -- the smallest shapes at which csrc/spg_parsed.hip can go wrong, not the workload's.

A case is a dict: name, dataset ('s3dis' | 'sema3d' | 'vkitti' | 'custom'), xyz f32 [n, 3], rgb u8 | f32 [n, 3], geof f32 [n, 4],
labels u32 | i32 [n, n_classes + 1], components (list of integer arrays: the reference's form), supervized_partition,
plane_model_elevation, elevation (f32 [n]: what features_supervision would hold; read only with both switches), max_points, seed
(random.seed before the scene: the reference's random.seed(area) of s3dis and vkitti, random.seed(0) of sema3d and custom), tags.

Tags
  PARITY        run through the reference by tools/gen_parsed_golden.py and recorded in tests/golden/parsed.npz.  (The reference
                hard-codes the trim limit 10000, so a lowered max_points cannot be PARITY; 'plane' -- elevation from RANSAC -- is
                not either: sklearn fits in float32, the device restates the fit in float64, and tests/golden/plane.npz records
                their distance.)
  UNPINNED      `dist` is NaN in exact arithmetic (n = 2: both points are equally far from their midpoint; identical points) and the
                float32 reference may print noise instead: its recorded `dist` is not compared.
  small_coords  |coordinate| < 10: the float32 reference's `dist` lies within 1e-4 of the float64 one (measured <= 8.4e-7).
  exact_sums    every float64 sum of the scene statistics is exact whatever its order, so the device's statistics must equal
                numpy's float64 ones bit for bit (k copies of one point; two points).
  stride=k      the record keeps every k-th row of each dataset (the 21 000-point scene would not fit a committed file).

Zeros of mixed sign are kept away from the extremes of an axis: np.min of {-0.0, +0.0} depends on the order numpy's SIMD reduction
happens to take, and (x - min) then differs in the sign of a zero.  An axis whose every value is -0.0 is unambiguous and is a case."""
import numpy as np

F32 = np.float32
N_CLASSES = {'s3dis': 13, 'sema3d': 8, 'vkitti': 13, 'custom': 8}
REDUCE_BLOCK = 256            # csrc/spg_parsed.hip: PR_BLOCK (threads of a reduction workgroup, rows of a gather workgroup)
REDUCE_MAX_BLOCKS = 1024      # csrc/spg_part.h: PART_MAX_BLOCKS: beyond, a workgroup strides over the scene


def room(n, offset=0.0, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.uniform(0, (6.0, 5.0, 3.0), size=(n, 3)) + [offset, offset, 0.0]).astype(F32)


def labels_of(n, n_classes, seed, dtype=np.uint32):
    """label histograms with tied rows (every 3rd: the two largest equal, the first must win) and all-zero rows (every 5th)"""
    rng = np.random.RandomState(seed + 1000)
    lab = rng.randint(0, 9, size=(n, n_classes + 1)).astype(dtype)
    rows = np.arange(0, n, 3)
    a = rng.randint(1, n_classes + 1, size=len(rows))
    b = (a - 1 + rng.randint(1, n_classes, size=len(rows))) % n_classes + 1        # another column
    lab[rows, a] = lab[rows, b] = 20
    lab[::5, 1:] = 0               # (column 0, the unlabelled count, stays: it is not part of the arg-max)
    return lab


def partition(n, n_comp, seed):
    """every vertex in exactly one of n_comp components, members in random order"""
    rng = np.random.RandomState(seed + 2000)
    comp = rng.randint(0, n_comp, size=n)
    perm = rng.permutation(n)
    order = perm[np.argsort(comp[perm], kind='stable')].astype(np.uint32)
    return np.split(order, np.cumsum(np.bincount(comp, minlength=n_comp))[:-1])


def make(name, dataset, xyz, seed, *, rgb_f32=False, components=None, tags=(), labels_dtype=np.uint32, **kw):
    n = len(xyz)
    rng = np.random.RandomState(seed + 3000)
    rgb = rng.randint(0, 256, size=(n, 3)).astype(np.uint8)
    if rgb_f32:                     # (what a file with float colours holds: not only integers)
        rgb = (rgb.astype(F32) + rng.uniform(0, 1, size=(n, 3)).astype(F32)).astype(F32)
    case = dict(name=name, dataset=dataset, xyz=np.ascontiguousarray(xyz, dtype=F32), rgb=rgb,
                geof=rng.uniform(0, 1, size=(n, 4)).astype(F32), elevation=rng.uniform(-0.1, 3, size=n).astype(F32),
                labels=labels_of(n, N_CLASSES[dataset], seed, labels_dtype),
                components=components if components is not None else partition(n, max(1, n // 24), seed),
                supervized_partition=0, plane_model_elevation=0, max_points=10000,
                seed=1 + seed % 6 if dataset in ('s3dis', 'vkitti') else 0, tags=set(tags), stride=1)
    case.update(kw)
    return case


def _cases():
    out = []
    # ---- sizes: the wave, the workgroup, several workgroups plus one point; every recipe at the workgroup edge ----
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 4 * REDUCE_BLOCK + 1):
        tags = {'PARITY', 'small_coords'} | ({'UNPINNED', 'exact_sums'} if n <= 2 else set())
        out.append(make(f's3dis_n{n}', 's3dis', room(n, 0.0, n), n, tags=tags))
    for dataset in ('sema3d', 'vkitti', 'custom'):
        for n in (1, 65, 257):
            out.append(make(f'{dataset}_n{n}', dataset, room(n, 0.0, n + 7), n + 7, tags={'PARITY', 'small_coords'}, rgb_f32=(n == 65)))
    # the grid-stride path of the reductions: more than REDUCE_MAX_BLOCKS workgroups' worth, plus one point
    n = REDUCE_BLOCK * REDUCE_MAX_BLOCKS + 1
    out.append(make('s3dis_gridstride', 's3dis', room(n, 0.0, 5), 5, tags={'small_coords'}, components=partition(n, 300, 5)))
    # ---- degenerate extents ----
    same = np.tile(F32([1.25, -2.5, 0.75]), (37, 1))
    flat = room(100, 0.0, 21)
    flat[:, 2] = F32(1.5)
    negzero = room(65, 0.0, 22) - F32([3, 2.5, 1.5])          # extremes well away from zero on both sides
    negzero[::4, 0] = F32(-0.0); negzero[1::4, 1] = F32(-0.0); negzero[2::4, 2] = F32(-0.0); negzero[3::8] = F32(0.0)
    allneg = room(65, 0.0, 23)
    allneg[:, 1] = F32(-0.0)                                  # an axis of -0.0 alone: min = max = -0.0
    for dataset in ('s3dis', 'vkitti'):
        out.append(make(f'{dataset}_identical', dataset, same, 31, tags={'PARITY', 'UNPINNED', 'small_coords', 'exact_sums'}))
        out.append(make(f'{dataset}_flat_z', dataset, flat, 32, tags={'PARITY', 'small_coords'}))
        out.append(make(f'{dataset}_negzero', dataset, negzero, 33, tags={'PARITY', 'small_coords'}))
        out.append(make(f'{dataset}_negzero_axis', dataset, allneg, 34, tags={'PARITY', 'small_coords'}))
    out.append(make('sema3d_negzero', 'sema3d', negzero, 35, tags={'PARITY', 'small_coords'}))
    # ---- the project's scale edge ----
    for off in (1e3, 1e5):
        out.append(make(f's3dis_offset{off:g}', 's3dis', room(257, off, 41), 41, tags={'PARITY'}))
        out.append(make(f'vkitti_offset{off:g}', 'vkitti', room(257, off, 42), 42, tags={'PARITY'}))
    # ---- components: an empty one (first, middle, last), a vertex in none (0 and 64), a vertex in two (7), one member ----
    comps = [np.zeros(0, np.uint32), np.arange(1, 20, dtype=np.uint32), np.zeros(0, np.uint32), np.array([7], np.uint32),
             np.arange(63, 19, -1).astype(np.uint32), np.array([7, 30, 7], np.uint32), np.zeros(0, np.uint32)]
    for dataset in ('s3dis', 'sema3d', 'vkitti', 'custom'):
        out.append(make(f'{dataset}_components', dataset, room(65, 0.0, 51), 51, components=comps, tags={'PARITY', 'small_coords'},
                        labels_dtype=np.int32))
    # ---- trimming: 10 000 stays, 10 001 is trimmed (one scene of 21 000 points); a lowered limit over several components ----
    n = 21000
    big = [np.arange(0, 10000, dtype=np.uint32), np.arange(20000, 9999, -1).astype(np.uint32), np.arange(20001, n, dtype=np.uint32)]
    out.append(make('sema3d_trim10001', 'sema3d', room(n, 0.0, 61), 61, components=big, tags={'PARITY', 'small_coords'}, stride=64))
    for dataset in ('s3dis', 'sema3d'):
        out.append(make(f'{dataset}_max7', dataset, room(65, 0.0, 62), 62, components=partition(65, 6, 62), max_points=7,
                        tags={'small_coords'}))
    # ---- s3dis: the other elevation sources ----
    out.append(make('s3dis_supervized', 's3dis', room(257, 0.0, 71), 71, supervized_partition=1, plane_model_elevation=1,
                    tags={'PARITY', 'small_coords'}))
    out.append(make('s3dis_supervized_z4', 's3dis', room(65, 0.0, 72), 72, supervized_partition=1, tags={'PARITY', 'small_coords'},
                    rgb_f32=True))
    from plane_cases import room as plane_room
    out.append(make('s3dis_plane', 's3dis', plane_room(600, 0.0, 1), 73, plane_model_elevation=1, tags={'small_coords', 'plane'}))
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    return out


_CACHE = []


def cases():
    if not _CACHE:
        _CACHE.extend(_cases())
    return _CACHE


def names(tag=None):
    return [c['name'] for c in cases() if tag is None or tag in c['tags']]


def get(name):
    return next(c for c in cases() if c['name'] == name)
