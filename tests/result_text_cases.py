"""The inputs of the result-text tests (csrc/spg_format.hip, ops.text.format_table / error_colours and the writers of
partition/provider.py), shared by the CPU restatement test, the GPU test and tools/gen_result_text_golden.py.  numpy only.

A table is a list of column specs over host arrays, so that the GPU test can rebuild the same views on device copies:
    ('vec', a)         a contiguous [n]
    ('col', a, j)      column j of a contiguous [n, k]
    ('step', a, s)     every s-th element of a contiguous vector
    ('mat', a)         a contiguous [n, k], standing for its k columns
"""
import numpy as np

ROW_COUNTS = (0, 1, 63, 64, 65, 257)
BLOCK_ROWS = 100                      # the writers' block size in the tests; 257 rows cross it twice
TIE_M = (1, 3, 5, 7, 9, 11, 13, 15, 8388609, 12345677, 16777215)
TIE_K = range(10, 41)


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def special_f32():
    """zeros, infinities, NaNs of both signs and several payloads, the subnormal range's ends, FLT_MAX, the two switches between
    fixed and scientific notation with their float32 neighbours, and a few plain values, each with both signs"""
    bits = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffabcdef,
            0x7fa00000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff]
    values = list(np.array(bits, dtype=np.uint32).view(np.float32))
    for v in (1e18, 1e-4, 1e17, 1e-5):
        values += _neighbours(v)
    values += [np.float32(v) for v in (1, 255, 0.5, 16777216, 2.0 ** -20, 0.1, 123.456, 1e10, 3e38, 1e-38, 1e-40)]
    out = np.array(values, dtype=np.float32)
    return np.concatenate((out, -out))


def tie_f32():
    """every m * 2^-k of TIE_M x TIE_K whose exact decimal expansion has 19 significant digits: m is odd, so m * 5^k are the
    digits, the last of them is 5 and the 18-digit rounding is a tie"""
    ties = [(m, k) for m in TIE_M for k in TIE_K if len(str(m * 5 ** k)) == 19]
    assert len(ties) >= 15 and all(str(m * 5 ** k)[-1] == '5' for m, k in ties), ties
    out = np.array([m * 2.0 ** -k for m, k in ties], dtype=np.float32)
    assert all(float(v) == m * 2.0 ** -k for v, (m, k) in zip(out, ties))              # representable
    return out


def random_f32(n=200000, seed=20240521):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def all_f32():
    return np.concatenate((special_f32(), tie_f32(), random_f32()))


def _powers(lo, hi, signed):
    vals = {0, lo, hi, lo + 1, hi - 1}
    k = 1
    while k <= hi:
        vals |= {k - 1, k, k + 1}
        if signed:
            vals |= {-k - 1, -k, -k + 1}
        k *= 10
    return sorted(v for v in vals if lo <= v <= hi)


def int_cases():
    """{dtype name: values}: every uint8; int32, uint32 and int64 at their extremes, at 0 and around +-10^k"""
    return {'uint8': np.arange(256, dtype=np.uint8),
            'int32': np.array(_powers(-2 ** 31, 2 ** 31 - 1, True), dtype=np.int32),
            'uint32': np.array(_powers(0, 2 ** 32 - 1, False), dtype=np.uint32),
            'int64': np.array(_powers(-2 ** 63, 2 ** 63 - 1, True), dtype=np.int64)}


def resolve(spec):
    """the host view a column spec stands for: [n], or [n, k] for 'mat'"""
    kind, a = spec[0], spec[1]
    return a if kind in ('vec', 'mat') else a[:, spec[2]] if kind == 'col' else a[::spec[2]]


def columns_of(specs):
    """the 1-D host columns of a table"""
    out = []
    for spec in specs:
        v = resolve(spec)
        out += [v[:, j] for j in range(v.shape[1])] if v.ndim == 2 else [v]
    return out


def _mixed(n, rng):
    """n values of every kind, drawn over each kind's whole range"""
    f = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return {'f32': f, 'u8': rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8),
            'i32': rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32),
            'u32': rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
            'i64': rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)}


def table_cases():
    """[(name, column specs)]: the value cases as one-column tables, and tables of 1, 7 and 16 columns with mixed kinds and strided
    columns at every row count of ROW_COUNTS"""
    cases = [('f32_all', [('vec', all_f32())])]
    cases += [(f'int_{name}', [('vec', v)]) for name, v in int_cases().items()]
    rng = np.random.default_rng(7)
    for n in ROW_COUNTS:
        xyz = (rng.standard_normal((n, 3)) * 50).astype(np.float32)
        rgb = rng.integers(0, 256, (n, 3), dtype=np.uint64).astype(np.uint8)
        m = _mixed(3 * n, rng)
        wide = _mixed(4 * n, rng)
        cases.append((f'labels_{n}', [('vec', m['u8'][:n].copy())]))
        cases.append((f'xyzrgbl_{n}', [('mat', xyz), ('mat', rgb), ('vec', m['i64'][:n].copy())]))
        cases.append((f'strided7_{n}', [('col', xyz, 2), ('step', m['i32'], 3), ('col', rgb, 1), ('step', m['u32'], 3), ('col', xyz, 0),
                                        ('step', m['i64'], 3), ('step', m['f32'], 3)]))
        cases.append((f'wide16_{n}', [('mat', wide['f32'].reshape(n, 4)), ('mat', wide['i64'].reshape(n, 4)), ('col', wide['u8'].reshape(n, 4), 3),
                                      ('col', wide['i32'].reshape(n, 4), 1), ('mat', wide['u32'].reshape(n, 4)), ('step', wide['f32'], 4),
                                      ('step', wide['u8'], 4)]))
    return cases


# ---- the cloud the reference's writers run on (tools/gen_result_text_golden.py) ----
N_VER, N_LABEL, DATASET, SEED = 300, 8, 'sema3d', 7
DATASETS = {'s3dis': 14, 'sema3d': 9, 'vkitti': 14, 'custom_dataset': 3}          # labels with a colour


def cloud_case():
    rng = np.random.default_rng(11)
    n = N_VER
    xyz = (rng.standard_normal((n, 3)) * np.array([30.0, 30.0, 3.0])).astype(np.float32)
    xyz[:4] = [[0, -0.0, 1], [1e-5, 123456.789, -2.5e-4], [16777216, 0.1, -1e18], [3.0e38, 1e-40, 0.5]]
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint64).astype(np.uint8)
    labels = (np.arange(n) % (N_LABEL + 1)).astype(np.int64)
    rng.shuffle(labels)
    labels[17] = N_LABEL + 3                                                       # out of range: stays black in prediction2ply
    histograms = rng.random((n, N_LABEL + 1)).astype(np.float32)
    perm = rng.permutation(n)
    cuts = [0, 40, 41, 90, 150, 151, 230, 270]                                     # 7 components; 30 vertices in none
    components = [np.sort(perm[a:b]).astype(np.int64) for a, b in zip(cuts[:-1], cuts[1:])]
    geof = rng.random((n, 4)).astype(np.float32)
    geof[:6, 0] = [0.0, 1.0, 1.0 / 255, 2.0 / 255, 0.999999, 0.5]
    geof[100:140, 1] += 1.0                                                        # up to 2: 255 * v above 255
    geof[200:210, 3] = 2.0
    return dict(xyz=xyz, rgb=rgb, labels=labels, histograms=histograms, components=components, geof=geof,
                scalar=(rng.standard_normal(n) * 1e3).astype(np.float32), object_indices=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                sp_centroids=(rng.standard_normal((7, 3)) * 10).astype(np.float32), source=rng.integers(0, 7, (12, 1)).astype(np.int64),
                target=rng.integers(0, 7, (12, 1)).astype(np.int64))


def error_case():
    """2000 vertices for error2ply's colours: every grey level, saturated primaries and their mixtures, black, white, random
    colours; labels with zeros, predictions right and wrong"""
    rng = np.random.default_rng(13)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.uint8)
    near = np.array([[255, 254, 255], [1, 0, 0], [0, 1, 0], [0, 0, 1], [254, 255, 255], [128, 127, 128], [178, 178, 179]], dtype=np.uint8)
    rgb = np.concatenate((grey, grey, corners, corners, near, near))
    rgb = np.concatenate((rgb, rng.integers(0, 256, (2000 - len(rgb), 3), dtype=np.uint64).astype(np.uint8)))
    labels = rng.integers(0, 5, 2000).astype(np.int64)
    prediction = np.where(rng.random(2000) < 0.5, labels, rng.integers(0, 5, 2000)).astype(np.int64)
    labels[:256], prediction[:256] = 1, 1                                          # every grey level right ...
    labels[256:512], prediction[256:512] = 1, 2                                    # ... and wrong
    labels[512:520], prediction[512:520] = 0, 3                                    # label 0 counts as right
    return dict(rgb=rgb, labels=labels, prediction=prediction)


def label_cloud_case(n=1000, n_ref=200, seed=17):
    """a text cloud of n `x y z i r g b` lines, the pruned cloud xyz [n_ref, 3] and its labels, for write_semantic3d_labels"""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3)) * 20 - 10
    lines = [f'{p[0]:.3f} {p[1]:.3f} {p[2]:.3f} {int(rng.integers(0, 2000))} {int(rng.integers(0, 256))} {int(rng.integers(0, 256))} '
             f'{int(rng.integers(0, 256))}' for p in pts]
    xyz = (rng.random((n_ref, 3)) * 20 - 10).astype(np.float32)
    return dict(data=('\n'.join(lines) + '\n').encode(), xyz=xyz, labels=rng.integers(0, 9, n_ref).astype(np.uint8),
                histograms=rng.random((n_ref, 9)).astype(np.float32))
