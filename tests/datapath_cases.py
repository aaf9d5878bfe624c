"""Case tables, references, bounds and a numpy stand-in for the units that feed and drain the training step: the device loader
(spg_load_superpoints, spg_loader_random), batch construction (spg_set_batch, spg_gather_rows, spg_batch_graph_build[_dev],
spg_edge_features) and the evaluation accounting (spg_eval_accumulate).  No test in here: tests/test_datapath_cases.py admits the
tables on the CPU (stand-in, planted faults), tests/test_gpu_datapath_edges.py runs them on the device.  Nothing below is derived
from what the device returns.

A "device" is any object with the methods of `StandIn` (numpy in, numpy out); every check_*(case, dev, report) drives one entry
point over the runs of one case and appends (case, entry, check, element, ratio) to `report`, where ratio = error / bound (0 or inf
for the bit-exact checks).  A failure names the case, the entry point, the check, the element and the ratio.

References
  loader      oracle.spg_loader_oracle.normalise_and_select on the rows the oracle's resampling picks (numpy's float32 axis-0
              add.reduce is row-sequential, hence the kernel's mean is numpy's bit for bit), then the column map.
  streams     oracle.philox_oracle.loader_random.
  batch       np.argsort(kind='stable') on the targets, np.bincount / np.cumsum for CSR and reverse CSR.
  features    the numpy expressions of learning/spg.py spg_edge_features on the same operands; the logarithms in float64.
  evaluation  oracle.spg_metrics_oracle.aggregate (np.mean over the stacked samples, np.argmax, the confusion update).

Bounds (u32 = 2^-24, u64 = 2^-53; ulp32(v) = the float32 spacing of the binade of |v|, 2^-149 at least)
  bit-exact   loader clouds and diameters without M, the non-rotated columns with M; the sampling indices; every integer buffer of
              the batch builders and of the evaluation; gathered rows; edge-feature kinds copy / d / r / const in both storage
              types (IEEE element-wise operations in the storage type's arithmetic, one final rounding for float64); the scaler,
              restated as float32(float64(float32(float64(u) - mean)) / scale) on the device's OWN unscaled output u.  NaN
              positions must agree, NaN payloads are not compared (the host and the device have different default NaNs).
  loader, M   the kernel rounds a float64 product once: out = fl32(d), d the device's float64 value of a m0 + b m1 + c m2.  For a
              length-3 dot product in float64, with or without fused multiply-adds, |fl(x.y) - x.y| <= g3 sum|x_i y_i| with
              g3 = 3 u64 / (1 - 3 u64) (Higham, Accuracy and Stability, 3.1); the same holds for the reference's own float64
              sum, so |d - ref| <= 2 g3 sum|terms|, and |out - ref| <= ulp32(max(|out|, |ref|)) / 2 + 2 g3 sum|terms|.
              The second term is what a cancelling row needs: there the result is far below its terms.
  + noise     out = fl32(fl32(d) + z): the rounding of d is no longer seen at the output, so it is taken at the largest |d| the above
              allows, ulp32(|ref| + 2 g3 sum|terms|) / 2; the one float32 addition on top gives ulp32(max(|out|, |ref + z|)) / 2, the
              reference's own float64 addition u64 |ref + z|.
  ld, f32     device: fl32(logf(x') - logf(y')), x' = fl32(x + 1e-10f).  With logf within 1 ulp (what test_gpu_batch.py assumes
              of it) |out - ref| <= ulp32(log x') + ulp32(log y') + ulp32(max(|out|, |ref|)) / 2; the reference's own two float64
              logarithms (1 ulp each) and subtraction add 2 u64 (|log x'| + |log y'|) + u64 |ref|.
  ld, f64     device: fl32(log(x + 1e-10) - log(y + 1e-10)) in float64; device and reference logarithms within 1 ulp of float64
              each: 4 u64 (|log x| + |log y|) + 2 u64 |ref| + ulp32(max(|out|, |ref|)) / 2.
  M (RNG)     1e-14 absolute, jitter 2e-7 absolute: the figures of tests/test_gpu_loader.py (float64 cos / sin, float32 logf /
              cosf / sinf of the device against numpy's on values below 1 resp. 0.05)."""
import os
import re

import numpy as np

from oracle import philox_oracle as P
from oracle import spg_loader_oracle as L
from oracle import spg_metrics_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
U64 = 2.0 ** -53
G3 = 3 * U64 / (1 - 3 * U64)
M_RNG_ATOL, JITTER_ATOL = 1e-14, 2e-7


def _define(name):
    text = open(os.path.join(ROOT, 'include', 'spg_hip.h')).read()
    return int(re.search(r'#define\s+' + name + r'\s+(\d+)', text).group(1))


MAX_FEATS = _define('SPG_LOADER_MAX_FEATS')
EF_MAX_COLS = _define('SPG_EF_MAX_COLS')
LOADER_MAX_NPTS = 4096                              # spg_load_superpoints: npts in [1, 4096]
BG_MAX_NODES, BG_MAX_EDGES = 4096, 32768            # spg_batch.hip: kBgMaxNodes, kBgMaxEdges


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    v = np.abs(np.asarray(v, dtype=F64))
    _, e = np.frexp(np.where(np.isfinite(v), v, 1.0))
    return np.where(v == 0, 2.0 ** -149, np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same_bits(a, b):
    """shape, dtype, NaN positions and every other bit"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def _where(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def exact(report, case, entry, check, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f'{case}: {entry}: {check}: {got.dtype}{got.shape} for {want.dtype}{want.shape}'
    if same_bits(got, want):
        report.append((case, entry, check, None, 0.0))
        return
    if got.dtype.kind == 'f':
        bad = (np.isnan(got) != np.isnan(want)) | (~np.isnan(got) & ~np.isnan(want) & (_bits(got) != _bits(want)))
    else:
        bad = got != want
    w = _where(bad)
    report.append((case, entry, check, w, float('inf')))
    raise AssertionError(f'{case}: {entry}: {check}: element {w} is {got[w]!r}, not {want[w]!r} (bit-exact check, ratio inf); {int(bad.sum())} of {bad.size} differ')


def bounded(report, case, entry, check, got, ref, bound):
    got, ref, bound = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64), np.broadcast_to(np.asarray(bound, dtype=F64), np.shape(ref))
    assert got.shape == ref.shape, f'{case}: {entry}: {check}: shape {got.shape} for {ref.shape}'
    if got.size == 0:
        report.append((case, entry, check, None, 0.0))
        return
    with np.errstate(all='ignore'):
        settled = (np.isnan(got) & np.isnan(ref)) | (got == ref)            # NaN on both sides, equal infinities
        ratio = np.where(settled, 0.0, np.abs(got - ref) / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    w = _where(ratio == ratio.max())
    report.append((case, entry, check, w, float(ratio[w])))
    assert ratio[w] <= 1.0, f'{case}: {entry}: {check}: element {w} is {got[w]!r} for {ref[w]!r}: {float(ratio[w]):.3f} of its bound {bound[w]:.3e}'


class Twice:
    """A device whose every call runs twice; the two results must agree bit for bit."""

    def __init__(self, dev):
        self.dev = dev

    def __getattr__(self, name):
        f = getattr(self.dev, name)

        def call(*a, **k):
            first, second = f(*a, **k), f(*a, **k)
            items = lambda r: list(r.items()) if isinstance(r, dict) else list(enumerate(r if isinstance(r, tuple) else (r,)))
            for (key, x), (_, y) in zip(items(first), items(second)):
                assert (x is None and y is None) or same_bits(x, y), f'{name}: result {key} of the second run differs from the first'
            return first
        return call


# ---------------------------------------------------------------------------------------------------------------------
# the numpy stand-in for the device (with the planted faults)
# ---------------------------------------------------------------------------------------------------------------------
class StandIn:
    """The kernels restated in numpy the way they compute; a knob plants one plausible mistake."""

    def __init__(self, **knobs):
        self.k = knobs

    # ---- loader
    def load(self, points, offsets, slot, sidx, colmap, norm, n_valid, M=None, noise=None):
        npts, nf = sidx.shape[1], len(colmap)
        clouds, diam = np.zeros((n_valid, nf, npts), F32), np.zeros(n_valid, F32)
        for s in range(len(slot)):
            if slot[s] < 0:
                continue
            raw = points[offsets[s]:offsets[s + 1]]
            rows = raw[sidx[s]]
            xyz = rows[:, :3]
            if self.k.get('pairwise_mean'):
                mean = np.array([np.add.reduce(np.ascontiguousarray(xyz[:, j])) for j in range(3)], F32) / F32(npts)
            else:
                mean = np.cumsum(xyz, axis=0, dtype=F32)[-1] / F32(npts)
            ext = raw[:, :3] if self.k.get('raw_diameter') else xyz
            d = F32(np.max(ext.max(0) - ext.min(0)))
            den = d if self.k.get('no_epsilon') else F32(d + F32(1e-10))
            with np.errstate(all='ignore'):
                c = (xyz - mean) / den if norm else xyz - mean
            full = rows.copy()
            full[:, :3] = c
            f = full[:, list(colmap)]
            if M is not None and nf >= 3:
                m = M[s].astype(F32) if self.k.get('f32_product') else M[s]
                a = f[:, :3].astype(m.dtype)
                f[:, :3] = (a[:, 0:1] * m[:, 0] + a[:, 1:2] * m[:, 1] + a[:, 2:3] * m[:, 2]).astype(F32)
            if noise is not None:
                f = f + noise[slot[s]]
            clouds[slot[s]], diam[slot[s]] = f.T, d if norm else F32(0)
        return clouds, diam

    def random(self, counts, ids, slot, npts, nfeat, n_valid, seed, step, augment, scale=0.0, rot=False, mirror_prob=0.0, jitter=False):
        return P.loader_random(counts, ids, slot, npts, nfeat, n_valid, seed, step, augment, scale, rot, mirror_prob, jitter)

    # ---- batch
    def _order(self, edges, n):
        """counting sort by target; inside a segment ascending edge index (or the planted reversed order)"""
        e = len(edges)
        bad = e > 0 and bool(((edges < 0) | (edges >= n)).any())
        if bad:
            return None
        buckets = [[] for _ in range(n)]
        for i in range(e):
            buckets[int(edges[i, 1])].append(i)
        if self.k.get('unstable_segment'):
            buckets = [b[::-1] for b in buckets]
        return np.array([i for b in buckets for i in b], dtype=np.int64)

    def set_batch(self, edges, n):
        perm = self._order(edges, n)
        if perm is None:
            return None, None, None, 1
        return edges[perm, 0], np.bincount(edges[:, 1], minlength=n).astype(np.int64), perm, 0

    def gather(self, src, perm, cols=None):
        cols = src.shape[1] if cols is None else cols
        out = np.zeros((len(perm), cols), F32)
        for r, s in enumerate(perm):
            if s >= 0:
                out[r] = src[s, :cols]
        return out

    def build(self, edges, feats, n, on_device):
        e = len(edges)
        perm = self._order(edges, n)
        if perm is None:
            return dict(err=1)
        src, dst = edges[perm, 0], edges[perm, 1]
        rev = np.array(sorted(range(e), key=lambda p: (src[p], p)), dtype=np.int32).reshape(e)
        ptr = lambda v: np.concatenate([[0], np.cumsum(np.bincount(v, minlength=n))]).astype(np.int32)
        return dict(err=0, hdr=np.array([n, n, e, 0], np.int32), idxn=src.astype(np.int64), degs=np.bincount(dst, minlength=n).astype(np.int64),
                    feats=None if feats is None else feats[perm], rowptr=ptr(dst), src=src.astype(np.int32), dst=dst.astype(np.int32),
                    rev_rowptr=ptr(src), rev=rev)

    def edge_features(self, columns, edges, mean=None, scale=None):
        e = len(edges)
        out = np.zeros((e, len(columns)), F32)
        a, b = edges[:, 0], edges[:, 1]
        with np.errstate(all='ignore'):
            for c, (kind, t, col) in enumerate(columns):
                if kind == 'const':
                    out[:, c] = 1
                elif kind == 'copy':
                    out[:, c] = t[:, col].astype(F32)
                else:
                    if t.dtype == F64 and self.k.get('f32_on_f64'):
                        t = t.astype(F32)
                    x, y, eps = t[a, col], t[b, col], t.dtype.type(1e-10)
                    out[:, c] = (x - y if kind == 'd' else np.log(x + eps) - np.log(y + eps) if kind == 'ld' else x / (y + eps)).astype(F32)
            if mean is not None:
                if self.k.get('one_rounding'):
                    out = ((out.astype(F64) - mean) / scale).astype(F32)
                else:
                    out = ((out.astype(F64) - mean).astype(F32).astype(F64) / scale).astype(F32)
        return out

    # ---- evaluation
    def evaluate(self, logits, label_mode, label_vec, confusion, counters):
        lg = logits if logits.ndim == 3 else logits[None]
        s, n, c = lg.shape
        with np.errstate(all='ignore'):
            if s > 1 and self.k.get('divide_first'):
                v = np.cumsum(lg / F32(s), axis=0, dtype=F32)[-1]
            else:
                v = np.cumsum(lg, axis=0, dtype=F32)[-1]
                v = v / F32(s) if s > 1 else v
        best, bv = np.zeros(n, np.int64), v[:, 0].copy() if c else None
        for k in range(1, c):
            with np.errstate(all='ignore'):
                take = (v[:, k] >= bv) if self.k.get('last_maximum') else (v[:, k] > bv)
            take |= np.isnan(v[:, k]) & ~np.isnan(bv)
            best[take], bv[take] = k, v[take, k]
        cm, cnt = confusion.copy(), counters.copy()
        for i in np.nonzero(label_mode != -100)[0]:
            if self.k.get('transposed_confusion'):
                cm[best[i], :] += label_vec[i]
            else:
                cm[:, best[i]] += label_vec[i]
            cnt[1] += 1
            cnt[0] += int(best[i] == label_mode[i])
        return best, cm, cnt


# ---------------------------------------------------------------------------------------------------------------------
# loader
# ---------------------------------------------------------------------------------------------------------------------
LOADER_NPTS = (1, 3, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 1000, 4096)
LOADER_NCOLS = (3, 14, 15)
VALUE_EDGES = ('identical', 'flat2', 'far', 'tiny')
M_KINDS = ('identity', 'mirror', 'rotscale', 'cancel')
THETA = 0.7


def column_maps(ncols):
    """name -> column map; ncols = 3 has no non-xyz column: its 'single' and 'front' maps stay inside xyz"""
    return {'identity': list(range(ncols)),
            'xyz': [0, 1, 2],
            'single': [min(3, ncols - 1)],
            'max repeats': [(7 * i + ncols - 1) % ncols for i in range(MAX_FEATS)],
            'permuted': [2, 0, 1] + list(range(3, ncols)),
            'front': [5, 4, 3, 0, 1, 2] if ncols >= 6 else [2, 2, 1]}


def _counts(npts):
    return [3, 1, max(1, npts - 1), npts, 2, npts + 1, 5 * npts, 4]


VALID = [False, True, True, True, False, True, True, False]      # slot -1 on the first, an inner and the last superpoint


def _m_of(kind):
    c, s = np.cos(THETA), np.sin(THETA)
    return {'identity': np.eye(3), 'mirror': np.diag([-1.0, 1.0, 1.0]), 'rotscale': 1.1 * L.rot_z(THETA),
            'cancel': 1.1 * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])}[kind]


def _superpoint(rng, n, ncols, kind):
    p = rng.standard_normal((n, ncols)).astype(F32)
    if kind == 'plain':
        p[:, :3] = p[:, :3] * 2 + rng.standard_normal(3).astype(F32) * 20
    elif kind == 'identical':      # every row the same point near 1e3: diameter 0, xyz - mean is pure summation round-off
        p[:, :3] = np.array([1000.123, -999.877, 1003.3], F32)
    elif kind == 'flat2':          # extent in x only
        p[:, 1:3] = np.array([7.25, -3.1], F32)
    elif kind == 'far':            # near 1e4, extent 1e-2
        p[:, :3] = (np.array([1e4, -1e4, 9e3]) + rng.uniform(0, 1e-2, (n, 3))).astype(F32)
    elif kind == 'tiny':           # diameter ~1e-7: float32(d + 1e-10) != d
        p[:, :3] = rng.uniform(0, 1e-7, (n, 3)).astype(F32)
    elif kind == 'cancel':         # xy on the line through the centre along (sin, cos): a cos(t) - b sin(t) cancels after centring
        t = rng.standard_normal(n)
        p[:, 0], p[:, 1] = (3.0 + np.sin(THETA) * t).astype(F32), (-2.0 + np.cos(THETA) * t).astype(F32)
    return p


def _loader_buffers(seed, npts, ncols, kinds):
    """S = 8 superpoints whose counts straddle npts, slots of -1 interleaved, the indices from the oracle's resampling"""
    rng = np.random.default_rng(seed)
    counts = _counts(npts)
    points = np.concatenate([_superpoint(rng, n, ncols, kinds[s % len(kinds)]) for s, n in enumerate(counts)])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    slot = np.full(len(counts), -1, np.int32)
    slot[VALID] = np.arange(sum(VALID), dtype=np.int32)
    sidx = np.zeros((len(counts), npts), np.int32)
    for s, n in enumerate(counts):
        if VALID[s]:
            sidx[s] = L.sample_indices(n, npts, L.test_rng(seed + s))
    return dict(points=points, offsets=offsets, slot=slot, sidx=sidx, n_valid=sum(VALID))


def loader_cases():
    out = [dict(name=f'npts{n}', kind='shape', npts=n) for n in LOADER_NPTS]
    out += [dict(name=f'values npts{n}', kind='values', npts=n) for n in (3, 64, 100, 257, 1000)]
    out += [dict(name=f'M npts{n}', kind='M', npts=n) for n in (3, 100, 257)]
    out += [dict(name='no superpoint', kind='empty', npts=128)]
    return out


def loader_runs(case):
    """-> dicts(tag, points, offsets, slot, sidx, n_valid, colmap, norm, M, noise)"""
    npts = case['npts']
    if case['kind'] == 'shape':
        for ncols in LOADER_NCOLS:
            buf = _loader_buffers(1000 * ncols + npts, npts, ncols, ['plain'])
            for name, cm in column_maps(ncols).items():
                for norm in (0, 1):
                    yield dict(buf, tag=f'ncols{ncols} {name} norm{norm}', colmap=cm, norm=norm, M=None, noise=None)
    elif case['kind'] == 'values':
        for edge in VALUE_EDGES:
            buf = _loader_buffers(77 + npts, npts, 14, [edge])
            for norm in (0, 1):
                yield dict(buf, tag=f'{edge} norm{norm}', colmap=list(range(14)), norm=norm, M=None, noise=None)
    elif case['kind'] == 'M':
        kinds = ['plain'] * 5 + ['cancel'] + ['plain'] * 2      # the valid superpoints 1, 2, 3, 5, 6 take M_KINDS in turn: 5 gets 'cancel'
        buf = _loader_buffers(5 + npts, npts, 14, kinds)
        M = np.stack([_m_of(M_KINDS[max(k, 0) % 4]) for k in buf['slot']])
        for name, cm in (('identity', list(range(14))), ('front', [5, 4, 3, 0, 1, 2])):
            nz = L.jitter_noise((buf['n_valid'], npts, len(cm)), np.random.RandomState(9))
            for noise in (None, nz):
                yield dict(buf, tag=f"{name}{' noise' if noise is not None else ''}", colmap=cm, norm=1, M=M, noise=noise)
    else:
        z = dict(points=np.zeros((0, 14), F32), offsets=np.zeros(1, np.int64), slot=np.zeros(0, np.int32), sidx=np.zeros((0, npts), np.int32), n_valid=0)
        yield dict(z, tag='S = 0', colmap=list(range(14)), norm=1, M=None, noise=None)
        buf = _loader_buffers(3, npts, 14, ['plain'])
        buf.update(slot=np.full(8, -1, np.int32), n_valid=0)
        yield dict(buf, tag='all slots -1', colmap=list(range(14)), norm=1, M=None, noise=None)


def loader_reference(run):
    """-> (clouds f32 [Nv, F, npts] (exact where `rotated` is False), diam, ref64 / bound for the rotated part or None)"""
    npts, nf = run['sidx'].shape[1], len(run['colmap'])
    nv = run['n_valid']
    clouds, diam = np.zeros((nv, nf, npts), F32), np.zeros(nv, F32)
    rot = run['M'] is not None and nf >= 3
    ref64, bound = (np.zeros((nv, 3, npts)), np.zeros((nv, 3, npts))) if rot else (None, None)
    for s in range(len(run['slot'])):
        k = run['slot'][s]
        if k < 0:
            continue
        rows = run['points'][run['offsets'][s]:run['offsets'][s + 1]][run['sidx'][s]]
        with np.errstate(all='ignore'):
            p, d = L.normalise_and_select(rows, run['norm'], '')
        p = p[:, run['colmap']]
        nz = run['noise'][k] if run['noise'] is not None else None
        clouds[k], diam[k] = (p if nz is None else p + nz).T, d[0]
        if rot:
            terms = p[:, :3].astype(F64)[:, None, :] * run['M'][s][None, :, :]              # [npts, 3 (out), 3 (k)]
            r = terms[:, :, 0] + terms[:, :, 1] + terms[:, :, 2]
            slack = 2 * G3 * np.abs(terms).sum(2)
            if nz is not None:                       # the first rounding, at the largest value the device's float64 product may have
                r1, r = r, r + nz[:, :3].astype(F64)
                slack = slack + 0.5 * ulp32(np.abs(r1) + slack) + U64 * np.abs(r)
            ref64[k], bound[k] = r.T, slack.T
    return clouds, diam, ref64, bound


def check_loader(case, dev, report):
    for run in loader_runs(case):
        name = f"{case['name']} {run['tag']}"
        clouds, diam = dev.load(run['points'], run['offsets'], run['slot'], run['sidx'], run['colmap'], run['norm'], run['n_valid'], run['M'], run['noise'])
        want, wdiam, ref64, slack = loader_reference(run)
        exact(report, name, 'load_superpoints', 'diam', diam, wdiam)
        if ref64 is None:
            exact(report, name, 'load_superpoints', 'cloud', clouds, want)
        else:
            exact(report, name, 'load_superpoints', 'cloud', clouds[:, 3:], want[:, 3:])
            got = clouds[:, :3].astype(F64)
            bound = 0.5 * ulp32(np.maximum(np.abs(got), np.abs(ref64))) + slack
            bounded(report, name, 'load_superpoints', 'cloud.M+noise' if run['noise'] is not None else 'cloud.M', got, ref64, bound)


# ---------------------------------------------------------------------------------------------------------------------
# loader random streams
# ---------------------------------------------------------------------------------------------------------------------
RANDOM_NPTS = (1, 2, 3, 5, 127, 128, 130)
RANDOM_NFEAT = (1, 2, 3, 4)
RANDOM_IDS = np.array([0, 2 ** 32 - 1, 2 ** 32, -1, -2 ** 40 + 3, 12345], np.int64)
RANDOM_SLOT = np.array([0, -1, 1, 2, -1, 3], np.int32)
RANDOM_STEPS = (0, 2 ** 32 - 1)


def random_cases():
    return [dict(name=f'npts{n}', npts=n) for n in RANDOM_NPTS]


def random_runs(case):
    npts = case['npts']
    counts = np.array([0, 1, max(0, npts - 1), npts, npts + 1, 2 ** 31 - 1], np.int64)
    i = 0
    for nfeat in RANDOM_NFEAT:
        flags = [(False, 0.0, False, 0.0, False)] + [(True, 1.1 * sc, bool(ro), 0.6 * mi, bool(ji)) for sc in (0, 1) for ro in (0, 1) for mi in (0, 1) for ji in (0, 1)]
        for augment, scale, rot, mirror, jitter in flags:
            i += 1
            yield dict(tag=f'nfeat{nfeat} augment{int(augment)} scale{scale:g} rot{int(rot)} mirror{mirror:g} jitter{int(jitter)} step{RANDOM_STEPS[i % 2]}',
                       args=(counts, RANDOM_IDS, RANDOM_SLOT, npts, nfeat, 4, 0x1234567890ABCDEF + i, RANDOM_STEPS[i % 2], augment, scale, rot, mirror, jitter))


def check_random(case, dev, report):
    for run in random_runs(case):
        name = f"{case['name']} {run['tag']}"
        sidx, M, noise = dev.random(*run['args'])
        o_sidx, o_M, o_noise = P.loader_random(*run['args'])
        counts, npts = run['args'][0], run['args'][3]
        assert np.all((o_sidx >= 0) & (o_sidx < np.maximum(counts, 1)[:, None])), name      # what the loader may index with
        exact(report, name, 'loader_random', 'sidx', sidx, o_sidx)
        assert (M is None) == (o_M is None) and (noise is None) == (o_noise is None), f'{name}: loader_random: which streams are returned'
        if o_M is not None:
            bounded(report, name, 'loader_random', 'M', M, o_M, M_RNG_ATOL)
        if o_noise is not None:
            bounded(report, name, 'loader_random', 'jitter', noise, o_noise, JITTER_ATOL)


# ---------------------------------------------------------------------------------------------------------------------
# batch construction
# ---------------------------------------------------------------------------------------------------------------------
BATCH_N = (1, 2, 1023, 1024, 1025, 2047, 2049, 4096)


def _hub_edges(rng, n, e):
    """random edges among nodes [3, n - 1) (the last node stays isolated) + targets 0 / 1 / 2 of in-degree exactly 64 / 65 / 129, a
    source of out-degree >= 65, duplicate edges, self loops; shuffled"""
    lo, hi = 3, n - 1
    edges = np.stack([rng.integers(0, hi, e), rng.integers(lo, hi, e)], 1).astype(np.int64)
    edges[0:64, 1], edges[64:129, 1], edges[129:258, 1] = 0, 1, 2
    edges[258:323, 0] = 5
    edges[330:340] = edges[320:330]
    edges[340:345] = np.arange(lo, lo + 5)[:, None]
    return edges[rng.permutation(e)]


def batch_cases():
    out = []
    for n in BATCH_N:
        for e in sorted({0, 1, 3 * n}):
            out.append(dict(name=f'N{n} E{e}', kind='graph', N=n, E=e, F=13 if (n + e) % 2 else 1))
    out += [dict(name='hubs N12', kind='graph', N=12, E=400, F=1), dict(name='hubs N70', kind='graph', N=70, E=500, F=13)]
    out += [dict(name=f'malformed {m}', kind='malformed', N=40, E=150, F=13, bad=m) for m in ('target', 'source', 'negative', 'equal N')]
    out += [dict(name='gather', kind='gather')]
    return out


def batch_edges(case):
    n, e = case['N'], case['E']
    rng = np.random.default_rng(1000 * n + e)
    if e >= 345 and n >= 12:
        edges = _hub_edges(rng, n, e)
    else:                      # a small graph: everything among the nodes in front of the isolated last one
        hi = max(1, n - 1)
        edges = np.stack([rng.integers(0, hi, e), rng.integers(0, hi, e)], 1).astype(np.int64)
    feats = rng.standard_normal((e, case['F'])).astype(F32)
    return edges, feats


def malformed(case, edges):
    """The same list with three entries spoilt.  spg_set_batch re-derived: count_targets skips an edge with a bad end and raises
    the flag; fill_buckets skips only a bad target, so an edge with a good target t and a bad source takes slot rowptr[t] + deg[t] + j
    (j < k_t, the number of such edges into t), at most G + k_t - 1 <= E - 1 with G = rowptr[N] the counted edges: inside bucket[0..E),
    in front of the flag word.  Every slot below G is written (the cursors hand out 0 .. deg[t] + k_t - 1 without a gap) with an edge
    index < E, so sort_buckets reads written slots only, ranks below deg[t], and stores inside idxn / perm[0..G).  The single-launch
    builder returns after the count phase."""
    n, bad = case['N'], edges.copy()
    rows = [7, len(edges) // 2, len(edges) - 1]
    for r in rows:
        if case['bad'] == 'target':
            bad[r, 1] = n + 5
        elif case['bad'] == 'source':
            bad[r, 0] = n + 5
        elif case['bad'] == 'negative':
            bad[r, r % 2] = -1
        else:
            bad[r, r % 2] = n
    return bad


def batch_reference(edges, feats, n):
    e = len(edges)
    stable = np.argsort(edges[:, 1], kind='stable')
    src, dst = edges[stable, 0], edges[stable, 1]
    degs = np.bincount(dst, minlength=n).astype(np.int64)
    out_deg = np.bincount(src, minlength=n)
    return dict(err=0, hdr=np.array([n, n, e, 0], np.int32), idxn=src.astype(np.int64), degs=degs, perm=stable.astype(np.int64),
                feats=feats[stable] if feats is not None else None,
                rowptr=np.concatenate([[0], np.cumsum(degs)]).astype(np.int32), src=src.astype(np.int32), dst=dst.astype(np.int32),
                rev_rowptr=np.concatenate([[0], np.cumsum(out_deg)]).astype(np.int32), rev=np.argsort(src, kind='stable').astype(np.int32))


GATHER_RUNS = (('negative indices', 9, 40, 7, 7), ('ld_src > cols', 50, 33, 13, 5), ('one element', 3, 1, 1, 1), ('rows*cols 255', 20, 51, 5, 5),
               ('rows*cols 257', 300, 257, 1, 1), ('rows*cols 771', 300, 257, 4, 3))


def check_batch(case, dev, report):
    name = case['name']
    if case['kind'] == 'gather':
        for tag, nsrc, rows, ld, cols in GATHER_RUNS:
            rng = np.random.default_rng(rows)
            src = rng.standard_normal((nsrc, ld)).astype(F32)
            perm = rng.integers(0, nsrc, rows).astype(np.int64)
            if tag == 'negative indices':
                perm[::3] = -1 - np.arange(len(perm[::3]))
            want = np.where((perm >= 0)[:, None], src[np.maximum(perm, 0), :cols], F32(0))
            exact(report, f'{name} {tag}', 'gather_rows', 'rows', dev.gather(src, perm, cols), want)
        return
    edges, feats = batch_edges(case)
    n = case['N']
    if case['kind'] == 'malformed':
        bad = malformed(case, edges)
        assert dev.set_batch(bad, n)[3] == 1, f'{name}: set_batch: flag not raised'
        for on_device in (False, True):
            assert dev.build(bad, feats, n, on_device)['err'] == 1, f'{name}: batch_graph_build: flag not raised'
    want = batch_reference(edges, feats, n)          # (the repaired list after a malformed one)
    idxn, degs, perm, err = dev.set_batch(edges, n)
    assert err == 0, f'{name}: set_batch: flag raised on a well-formed list'
    for key, got in (('idxn', idxn), ('degs', degs), ('perm', perm)):
        exact(report, name, 'set_batch', key, got, want[key])
    exact(report, name, 'gather_rows', 'rows', dev.gather(feats, perm), want['feats'])
    if n <= BG_MAX_NODES and len(edges) <= BG_MAX_EDGES:
        for on_device in (False, True):
            got = dev.build(edges, feats, n, on_device)
            assert got['err'] == 0, f'{name}: batch_graph_build: flag raised on a well-formed list'
            for key in ('hdr', 'idxn', 'degs', 'feats', 'rowptr', 'src', 'dst', 'rev_rowptr', 'rev'):
                exact(report, name, 'batch_graph_build' + ('_dev' if on_device else ''), key, got[key], want[key])


# ---------------------------------------------------------------------------------------------------------------------
# edge features
# ---------------------------------------------------------------------------------------------------------------------
EF_E = (0, 1, 255, 257)
EF_KINDS = ('copy', 'd', 'ld', 'r', 'const')


def ef_cases():
    out = [dict(name=f'E{e}', E=e, edge='plain') for e in EF_E]
    out += [dict(name='zeros', E=257, edge='zeros'), dict(name='negative', E=257, edge='negative'), dict(name='counts', E=257, edge='counts'),
            dict(name='max cols', E=33, edge='max cols'), dict(name='scale 1e-12', E=255, edge='scale')]
    return out


def ef_build(case):
    """-> (columns [(kind, array or None, column)], edges, mean, scale)"""
    e, edge = case['E'], case['edge']
    rng = np.random.default_rng(31 + e + len(edge))
    n = 50
    edges = rng.integers(0, n, (e, 2)).astype(np.int64)
    node32 = rng.uniform(0.01, 9, (n, 3)).astype(F32)
    node64 = rng.integers(1, 10000, (n, 2)).astype(np.uint64).astype(F64)
    if edge == 'counts':           # the uint64 point count above 2^24, up to 1e12: neighbours that float32 cannot tell apart
        node64[:, 0] = 2.0 ** 24 + rng.integers(0, 64, n)
        node64[:, 1] = np.floor(10.0 ** rng.uniform(7.3, 12, n))
        node64[0, 1] = 1e12
    if edge == 'zeros':
        node32[::3, 0], node32[1::4, 1], node64[::3, 0] = 0, 0, 0
        edges[:5] = [[0, 0], [0, 1], [1, 0], [3, 3], [4, 8]]      # 0 / 0, 0 / y, x / 0
    if edge == 'negative':
        node32[::2, 0], node64[1::3, 0] = -node32[::2, 0], -node64[1::3, 0]
    edge32 = rng.standard_normal((e, 4)).astype(F32)
    edge64 = rng.standard_normal((e, 2)) * 1e3
    columns = [(k, t, c) for t, c in ((node32, 0), (node32, 2), (node64, 0), (node64, 1)) for k in ('d', 'ld', 'r')]
    columns += [('copy', edge32, 1), ('copy', edge32, 3), ('copy', edge64, 1), ('const', None, 0)]
    if edge == 'max cols':
        columns = (columns * 3)[:EF_MAX_COLS]
    nc = len(columns)
    mean, scale = rng.standard_normal(nc), rng.uniform(0.5, 3, nc)
    if edge == 'scale':
        scale[::2] = 1e-12
    return columns, edges, mean, scale


def ef_reference(columns, edges):
    """-> (exact f32 [E, ncols], is_ld [ncols], ref64 [E, ncols], bound [E, ncols] without the final half ulp)"""
    e, nc = len(edges), len(columns)
    want, ref64, bound = np.zeros((e, nc), F32), np.zeros((e, nc)), np.zeros((e, nc))
    a, b = edges[:, 0], edges[:, 1]
    is_ld = np.array([k == 'ld' for k, _, _ in columns])
    with np.errstate(all='ignore'):
        for c, (kind, t, col) in enumerate(columns):
            if kind == 'const':
                want[:, c] = 1
            elif kind == 'copy':
                want[:, c] = t[:, col].astype(F32)
            elif kind == 'ld':
                xs, ys = t[:, col][a] + t.dtype.type(1e-10), t[:, col][b] + t.dtype.type(1e-10)      # the operands in the storage type
                lx, ly = np.log(xs.astype(F64)), np.log(ys.astype(F64))
                ref64[:, c] = lx - ly
                if t.dtype == F32:
                    bound[:, c] = ulp32(lx) + ulp32(ly) + 2 * U64 * (np.abs(lx) + np.abs(ly)) + U64 * np.abs(lx - ly)
                else:
                    bound[:, c] = 4 * U64 * (np.abs(lx) + np.abs(ly)) + 2 * U64 * np.abs(lx - ly)
            else:
                v = t[:, col]
                want[:, c] = (v[a] - v[b] if kind == 'd' else v[a] / (v[b] + t.dtype.type(1e-10))).astype(F32)
    return want, is_ld, ref64, bound


def check_ef(case, dev, report):
    name = case['name']
    columns, edges, mean, scale = ef_build(case)
    out = dev.edge_features(columns, edges)
    want, is_ld, ref64, slack = ef_reference(columns, edges)
    exact(report, name, 'edge_features', 'copy d r const', out[:, ~is_ld], want[:, ~is_ld])
    got = out[:, is_ld].astype(F64)
    with np.errstate(all='ignore'):
        bound = slack[:, is_ld] + 0.5 * ulp32(np.maximum(np.abs(got), np.abs(ref64[:, is_ld])))
    bounded(report, name, 'edge_features', 'ld', got, ref64[:, is_ld], bound)
    scaled = dev.edge_features(columns, edges, mean, scale)
    with np.errstate(all='ignore'):
        restated = ((out.astype(F64) - mean).astype(F32).astype(F64) / scale).astype(F32)
    exact(report, name, 'edge_features', 'scaler', scaled, restated)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------------
EVAL_S, EVAL_N, EVAL_C = (1, 2, 33), (0, 1, 255, 256, 257), (1, 2, 13, 40)


def eval_cases():
    out = [dict(name=f'S{s} C{c}', kind='ties', S=s, C=c) for s in EVAL_S for c in EVAL_C]
    out += [dict(name=k, kind=k, S=33, C=13) for k in ('division tie', 'summation order')]
    out += [dict(name=k, kind=k, S=2, C=13) for k in ('all -100', 'labels 2^40', 'two calls')]
    return out


def _labels(rng, n, c, big=False):
    lv = (rng.integers(0, 10000, (n, c)) * (rng.random((n, c)) < 0.4)).astype(np.int64)
    if big:
        lv[lv > 0] = 2 ** 40
    lm = np.where((lv.sum(1) == 0) | (rng.random(n) < 0.2), -100, lv.argmax(1) if c else 0).astype(np.int64)
    return lm, lv


def _tie_logits(rng, s, n, c):
    """integer-valued logits in [-2, 2] (exact sums, many ties); the first rows hold the named edges"""
    lg = rng.integers(-2, 3, (s, n, c)).astype(F32)
    special = [('first and last tied', lambda r: (r.fill(-1), r.__setitem__((slice(None), [0, -1]), 2))),
               ('all equal', lambda r: r.fill(1)),
               ('signed zeros', lambda r: (r.fill(0), r.__setitem__((slice(None), slice(0, None, 2)), F32(-0.0)))),
               ('-inf row', lambda r: r.fill(-np.inf)),
               ('NaN inside', lambda r: r.__setitem__((0, c // 2), np.nan)),
               ('NaN in class 0', lambda r: r.__setitem__((0, 0), np.nan)),
               ('two NaN', lambda r: (r.__setitem__((0, c // 2), np.nan), r.__setitem__((s - 1, c - 1), np.nan))),
               ('inf - inf', lambda r: (r.__setitem__((0, c - 1), np.inf), r.__setitem__((s - 1, c - 1), -np.inf if s > 1 else np.inf)))]
    for i, (_, f) in enumerate(special):
        for row in range(i, n, 64):          # in every block of the launch
            f(lg[:, row, :])
    return lg


def division_tie():
    """Sums a < b (adjacent float32 values above 33) whose quotients by 33 round to the same float32: found by search, not measured"""
    a = F32(33.0)
    for _ in range(4096):
        b = np.nextafter(a, F32(64))
        if F32(a / F32(33)) == F32(b / F32(33)):
            return a, b
        a = b
    raise AssertionError('no tie')


def eval_runs(case):
    """-> dicts(tag, logits [S, N, C] or [N, C], lm, lv)"""
    s, c, kind = case['S'], case['C'], case['kind']
    rng = np.random.default_rng(100 * s + c + len(kind))
    if kind == 'ties':
        for n in EVAL_N:
            lg = _tie_logits(rng, s, n, c)
            lm, lv = _labels(rng, n, c)
            yield dict(tag=f'N{n}', logits=lg if s > 1 else lg[0], lm=lm, lv=lv)
        return
    n = 257
    lm, lv = _labels(rng, n, c, big=kind == 'labels 2^40')
    if kind == 'division tie':
        a, b = division_tie()
        lg = np.zeros((s, n, c), F32)
        lg[0] = a - 1
        lg[0, ::2, 3], lg[0, ::2, 9] = a, b            # the later class has the larger SUM and the same MEAN: the first wins
        lg[0, 1::2, 3], lg[0, 1::2, 9] = b, a
    elif kind == 'summation order':                   # class k + 1 holds class k's values in another sample order: equal up to round-off
        lg = rng.standard_normal((s, n, c)).astype(F32)
        for k in range(1, c):
            lg[:, :, k] = lg[rng.permutation(s), :, 0]
    else:
        lg = _tie_logits(rng, s, n, c)
    if kind == 'all -100':
        lm[:] = -100
    yield dict(tag='N257', logits=lg, lm=lm, lv=lv)


def eval_reference(run):
    lg = run['logits']
    samples = list(lg) if lg.ndim == 3 else [lg]
    with np.errstate(all='ignore'):
        pred, cm, correct, counted = MO.aggregate(samples, run['lm'], run['lv'], lg.shape[-1])
    assert np.abs(cm).max(initial=0) < 2.0 ** 53
    return pred, cm.astype(np.int64), np.array([correct, counted], np.int64)


def check_eval(case, dev, report):
    for run in eval_runs(case):
        name = f"{case['name']} {run['tag']}"
        c = run['logits'].shape[-1]
        pred, cm, cnt = dev.evaluate(run['logits'], run['lm'], run['lv'], np.zeros((c, c), np.int64), np.zeros(2, np.int64))
        wpred, wcm, wcnt = eval_reference(run)
        exact(report, name, 'eval_accumulate', 'pred', pred, wpred)
        exact(report, name, 'eval_accumulate', 'confusion', cm, wcm)
        exact(report, name, 'eval_accumulate', 'counters', cnt, wcnt)
        if case['kind'] == 'two calls':
            _, cm2, cnt2 = dev.evaluate(run['logits'], run['lm'], run['lv'], cm, cnt)
            exact(report, name, 'eval_accumulate', 'confusion, second call', cm2, 2 * wcm)
            exact(report, name, 'eval_accumulate', 'counters, second call', cnt2, 2 * wcnt)


# ---------------------------------------------------------------------------------------------------------------------
# every table, and the planted faults
# ---------------------------------------------------------------------------------------------------------------------
TABLES = {'loader': (loader_cases, check_loader), 'random': (random_cases, check_random), 'batch': (batch_cases, check_batch),
          'features': (ef_cases, check_ef), 'evaluation': (eval_cases, check_eval)}

# knob -> (table, case, the check that must catch it)
KNOBS = {'pairwise_mean': ('loader', 'values npts1000', 'cloud'),
         'raw_diameter': ('loader', 'npts100', 'diam'),
         'no_epsilon': ('loader', 'values npts100', 'cloud'),
         'f32_product': ('loader', 'M npts100', 'cloud.M'),
         'one_rounding': ('features', 'E257', 'scaler'),
         'f32_on_f64': ('features', 'counts', 'copy d r const'),
         'unstable_segment': ('batch', 'hubs N12', 'idxn'),
         'last_maximum': ('evaluation', 'S1 C13', 'pred'),
         'divide_first': ('evaluation', 'summation order', 'pred'),
         'transposed_confusion': ('evaluation', 'S2 C13', 'confusion')}


def case_of(table, name):
    return next(c for c in TABLES[table][0]() if c['name'] == name)
