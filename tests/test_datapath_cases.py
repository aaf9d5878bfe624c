"""CPU side of the loader / batch / evaluation edge suite (tests/datapath_cases.py; the device runs in
tests/test_gpu_datapath_edges.py):

* every reference agrees with the reference-made goldens where they overlap (tests/golden/loader.npz, metrics.npz) and with the
  existing oracles (load_batch, apply_augmentation, the host spg_edge_features, a row-by-row sequential mean);
* the numpy stand-in for the device goes through the very check functions the GPU test calls and passes every one;
* every planted fault of the stand-in fails the check named for it on the case named for it;
* every case is admitted by the library's own argument limits, and the tables hold the lattice they are there for."""
import os
import types

import numpy as np
import pytest

import datapath_cases as C
from conftest import GOLDEN
from oracle import spg_loader_oracle as L
from oracle import spg_metrics_oracle as MO

ALL = [(t, c['name']) for t, (cases, _) in C.TABLES.items() for c in cases()]


# ---------------------------------------------------------------------------------------------------------------------
# the references against the goldens and the existing oracles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,attribs,norm', [('s3dis', 'xyzrgbelpsvXYZ', 1), ('sema3d', 'xyzrgbelpsv', 1), ('nonorm', 'xyzelpsv', 0)])
def test_loader_reference_and_standin_reproduce_the_golden_clouds(tag, attribs, norm):
    g = np.load(os.path.join(GOLDEN, 'loader.npz'))
    m = L.load_batch(g['points'], g['offsets'], g['ids'], 40, 128, norm, attribs, train=False, test_seed_offset=3)
    assert np.array_equal(m['flag'], g[f'{tag}/flag'])
    run = dict(points=g['points'], offsets=g['offsets'], slot=m['slot'], sidx=m['sample_idx'], n_valid=int((m['flag'] == 0).sum()),
               colmap=L.column_map(attribs), norm=norm, M=None, noise=None)
    clouds, diam, _, _ = C.loader_reference(run)
    assert C.same_bits(clouds, g[f'{tag}/clouds']) and C.same_bits(diam, g[f'{tag}/diam'])
    s_clouds, s_diam = C.StandIn().load(run['points'], run['offsets'], run['slot'], run['sidx'], run['colmap'], norm, run['n_valid'])
    assert C.same_bits(s_clouds, clouds) and C.same_bits(s_diam, diam)


def test_numpy_mean_is_the_row_sequential_sum_at_every_table_size():
    """What makes the kernel's one-thread sum numpy's: float32 add.reduce over axis 0 of an [npts, 3] view adds row by row."""
    rng = np.random.default_rng(0)
    for npts in C.LOADER_NPTS:
        x = (rng.standard_normal((npts, 14)) * 3 + 1000).astype(np.float32)[:, :3]
        acc = np.zeros(3, np.float32)
        for row in x:
            acc = acc + row
        assert C.same_bits(np.mean(x, axis=0), acc / np.float32(npts)), npts


def test_rotated_reference_holds_the_oracles_augmentation_inside_its_bound():
    """oracle.apply_augmentation (np.dot in float64, rounded on the store, float32 noise on top) against the float64 reference"""
    for case in (c for c in C.loader_cases() if c['kind'] == 'M'):
        for run in C.loader_runs(case):
            _, _, ref64, slack = C.loader_reference(run)
            plain, _, _, _ = C.loader_reference(dict(run, M=None, noise=None))
            for s, k in enumerate(run['slot']):
                if k >= 0:
                    got = L.apply_augmentation(plain[k].T, run['M'][s], None if run['noise'] is None else run['noise'][k]).T[:3].astype(np.float64)
                    bound = 0.5 * C.ulp32(np.maximum(np.abs(got), np.abs(ref64[k]))) + slack[k]
                    assert np.all(np.abs(got - ref64[k]) <= bound), (case['name'], run['tag'], s)


def test_cancelling_rows_cancel():
    run = next(C.loader_runs(C.case_of('loader', 'M npts100')))
    _, _, ref64, slack = C.loader_reference(run)
    k = 3                                                    # the 'cancel' superpoint
    assert C.M_KINDS[k % 4] == 'cancel' and np.abs(ref64[k, 0]).max() < 1e-6 and np.abs(ref64[k, 1]).max() > 0.1
    assert np.median(slack[k, 0]) > 100 * 2.0 ** -149        # the term bound, not the half ulp of a result near zero, carries this row


def test_edge_feature_reference_is_the_host_function():
    """(without `size/d`: numpy subtracts the uint64 point counts modulo 2^64 where the float64 path of the device gives the signed
    difference -- no configuration of the reference uses that column)"""
    from superpoint_graph_amd.learning import spg
    rng = np.random.default_rng(2)
    n, e = 60, 300
    edges = rng.integers(0, n, (e, 2)).astype(np.int64)
    node = dict(xyz=rng.uniform(0, 9, (n, 3)).astype(np.float32), size=rng.integers(1, 2 ** 40, (n, 1)).astype(np.uint64))
    edge = dict(delta_avg=rng.standard_normal((e, 3)).astype(np.float32))
    ref = spg.spg_edge_features(edges, node, edge, types.SimpleNamespace(edge_attribs='delta_avg,xyz/d,size/r,xyz/r,constant,xyz/ld,size/ld'))
    size = node['size'].astype(np.float64)
    columns = [('copy', edge['delta_avg'], c) for c in range(3)] + [('d', node['xyz'], c) for c in range(3)] + [('r', size, 0)]
    columns += [('r', node['xyz'], c) for c in range(3)] + [('const', None, 0)] + [('ld', node['xyz'], c) for c in range(3)] + [('ld', size, 0)]
    want, is_ld, ref64, slack = C.ef_reference(columns, edges)
    assert C.same_bits(want[:, ~is_ld], ref[:, ~is_ld])
    bound = slack[:, is_ld] + 0.5 * C.ulp32(ref64[:, is_ld])
    assert np.all(np.abs(ref[:, is_ld] - ref64[:, is_ld]) <= bound)          # numpy's own float32 / float64 logarithms


@pytest.mark.parametrize('tag', ['multi', 'single'])
def test_standin_evaluation_reproduces_the_golden_metrics(tag):
    g = np.load(os.path.join(GOLDEN, 'metrics.npz'))
    lg = g['samples'] if tag == 'multi' else g['samples'][0]
    c = lg.shape[-1]
    pred, cm, cnt = C.StandIn().evaluate(lg, g['label_mode'], g['label_vec'], np.zeros((c, c), np.int64), np.zeros(2, np.int64))
    assert np.array_equal(pred, g[f'{tag}/pred']) and np.array_equal(cm, g[f'{tag}/cm'])
    assert tuple(cnt) == (int(g[f'{tag}/correct']), int(g[f'{tag}/counted']))
    wpred, wcm, wcnt = C.eval_reference(dict(logits=lg, lm=g['label_mode'], lv=g['label_vec']))
    assert np.array_equal(wpred, pred) and np.array_equal(wcm, cm) and np.array_equal(wcnt, cnt)
    assert MO.scores(wcm.astype(np.float64))[1] == float(g[f'{tag}/oa'])


def test_division_tie_is_one():
    a, b = C.division_tie()
    assert a < b and np.float32(a / np.float32(33)) == np.float32(b / np.float32(33))
    run = next(C.eval_runs(C.case_of('evaluation', 'division tie')))
    assert np.all(C.eval_reference(run)[0] == 3)             # the first of the two classes, whichever has the larger sum


# ---------------------------------------------------------------------------------------------------------------------
# the stand-in passes, the planted faults do not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table,name', ALL)
def test_standin_passes_every_check(table, name):
    report = []
    C.TABLES[table][1](C.case_of(table, name), C.Twice(C.StandIn()), report)
    assert report and max(r[4] for r in report) <= 1.0
    print(f'{table} {name}: {len(report)} checks, worst ratio {max(r[4] for r in report):.3f}')


@pytest.mark.parametrize('knob', sorted(C.KNOBS))
def test_planted_fault_fails_its_check(knob):
    table, name, check = C.KNOBS[knob]
    with pytest.raises(AssertionError) as e:
        C.TABLES[table][1](C.case_of(table, name), C.StandIn(**{knob: True}), [])
    assert f': {check}: element' in str(e.value) and str(e.value).startswith(name), (knob, str(e.value))


def test_every_fault_of_the_list_is_planted():
    assert len(C.KNOBS) == 10 and all(any(c['name'] == name for c in C.TABLES[t][0]()) for t, name, _ in C.KNOBS.values())


# ---------------------------------------------------------------------------------------------------------------------
# admission by the library's limits; the lattice
# ---------------------------------------------------------------------------------------------------------------------
def test_limits_against_the_sources():
    assert (C.MAX_FEATS, C.EF_MAX_COLS) == (16, 32)
    csrc = os.path.join(C.ROOT, 'superpoint_graph_amd', 'csrc')
    loader, batch = open(os.path.join(csrc, 'spg_loader.hip')).read(), open(os.path.join(csrc, 'spg_batch.hip')).read()
    assert 'npts >= 1 && npts <= 4096' in loader and 'npts <= 64 ? 64 : (npts <= 128 ? 128 : 256)' in loader
    assert f'kBgMaxNodes = {C.BG_MAX_NODES}, kBgMaxEdges = {C.BG_MAX_EDGES}' in batch and 'per = (N + 1023) / 1024' in batch


def test_loader_cases_are_admitted_and_hold_the_lattice():
    assert {c['npts'] for c in C.loader_cases() if c['kind'] == 'shape'} == set(C.LOADER_NPTS)
    seen = set()
    for case in C.loader_cases():
        assert 1 <= case['npts'] <= C.LOADER_MAX_NPTS
        for run in C.loader_runs(case):
            ncols, npts = run['points'].shape[1], run['sidx'].shape[1]
            assert ncols >= 3 and 1 <= len(run['colmap']) <= C.MAX_FEATS and all(0 <= c < ncols for c in run['colmap']) and len(run['slot']) <= 8
            counts = np.diff(run['offsets'])
            valid = run['slot'] >= 0
            assert np.array_equal(np.sort(run['slot'][valid]), np.arange(run['n_valid']))
            assert np.all((run['sidx'][valid] >= 0) & (run['sidx'][valid] < counts[valid, None]))      # every gathered row exists
            if run['M'] is not None:
                assert len(run['colmap']) >= 3 and run['M'].shape == (len(run['slot']), 3, 3)
            if len(counts) and valid.any():
                assert not valid[0] and not valid[-1] and {1, max(1, npts - 1), npts, npts + 1, 5 * npts} <= set(counts[valid])
            seen.add((ncols, len(run['colmap']), run['norm']))
    assert {s[0] for s in seen} == set(C.LOADER_NCOLS) and {1, 3, C.MAX_FEATS} <= {s[1] for s in seen} and {s[2] for s in seen} == {0, 1}
    maps = C.column_maps(14)
    assert maps['single'] == [3] and maps['permuted'][:3] == [2, 0, 1] and maps['front'][:3] == [5, 4, 3] and len(set(maps['max repeats'])) < C.MAX_FEATS
    # the value edges are what they are named
    for run in C.loader_runs(C.case_of('loader', 'values npts100')):
        _, diam, _, _ = C.loader_reference(dict(run, norm=1))
        edge = run['tag'].split()[0]
        if edge == 'identical':
            assert np.all(diam == 0)
        if edge == 'tiny':
            assert np.all(diam + np.float32(1e-10) != diam) and np.all(diam[1:] > 0)      # (the first valid superpoint has one point)
        if edge == 'far':
            assert np.all(diam <= 1.1e-2) and np.abs(run['points'][:, :3]).min() > 8e3


def test_random_cases_hold_the_lattice():
    res, flags, counts_seen = set(), set(), set()
    for case in C.random_cases():
        for run in C.random_runs(case):
            counts, ids, slot, npts, nfeat, nv, seed, step, *fl = run['args']
            assert len(counts) == len(ids) == len(slot) and nv == int((slot >= 0).sum()) and npts >= 1 and nfeat >= 1
            res.add((npts * nfeat) % 4)
            flags.add(tuple(bool(f) for f in fl))
            counts_seen |= {(int(c) - npts) if abs(int(c) - npts) <= 1 else int(c) for c in counts}
    assert res == {0, 1, 2, 3} and len(flags) == 17 and {-1, 0, 1, 2 ** 31 - 1} <= counts_seen
    assert {0, 2 ** 32 - 1, 2 ** 32, -1} <= set(C.RANDOM_IDS.tolist()) and set(C.RANDOM_STEPS) == {0, 2 ** 32 - 1}


def test_batch_cases_hold_the_lattice():
    for case in (c for c in C.batch_cases() if c['kind'] != 'gather'):
        edges, feats = C.batch_edges(case)
        n = case['N']
        assert n >= 1 and edges.shape == (case['E'], 2) and feats.shape == (case['E'], case['F'])
        assert np.all((edges >= 0) & (edges < n))
        if n > 1:
            assert not np.any(edges == n - 1)                                         # the isolated last node
        if case['E'] >= 345 and n >= 12:
            deg_in, deg_out = np.bincount(edges[:, 1], minlength=n), np.bincount(edges[:, 0], minlength=n)
            assert tuple(deg_in[:3]) == (64, 65, 129) and deg_out.max() >= 65
            assert np.any(edges[:, 0] == edges[:, 1]) and len({tuple(r) for r in edges.tolist()}) < len(edges)      # self loops, duplicates
        if case['kind'] == 'malformed':
            bad = C.malformed(case, edges)
            rows = np.nonzero(((bad < 0) | (bad >= n)).any(1))[0]
            assert len(rows) == 3
            if case['bad'] == 'source':
                assert np.all((bad[rows, 1] >= 0) & (bad[rows, 1] < n))               # a bad source ALONE: the target is good
    names = {c['name'] for c in C.batch_cases()}
    assert {f'N{n} E{e}' for n in C.BATCH_N for e in (0, 1, 3 * n)} <= names and {c['F'] for c in C.batch_cases() if 'F' in c} == {1, 13}
    assert all((rows * cols) % 256 for _, _, rows, _, cols in C.GATHER_RUNS) and any(ld > cols for _, _, _, ld, cols in C.GATHER_RUNS)


def test_feature_and_evaluation_cases_hold_the_lattice():
    for case in C.ef_cases():
        columns, edges, mean, scale = C.ef_build(case)
        assert 1 <= len(columns) <= C.EF_MAX_COLS and len(mean) == len(scale) == len(columns)
        assert {(k, t.dtype.name) for k, t, _ in columns if t is not None} == {(k, d) for k in ('d', 'ld', 'r', 'copy') for d in ('float32', 'float64')}
    assert len(C.ef_build(C.case_of('features', 'max cols'))[0]) == C.EF_MAX_COLS
    assert C.ef_build(C.case_of('features', 'counts'))[0][6][1][:, 1].max() == 1e12 and 1e-12 in C.ef_build(C.case_of('features', 'scale 1e-12'))[3]
    assert {(c['E'] * len(C.ef_build(c)[0])) % 256 != 0 for c in C.ef_cases() if c['E']} == {True}
    seen = set()
    for case in C.eval_cases():
        for run in C.eval_runs(case):
            lg = run['logits']
            seen.add((1 if lg.ndim == 2 else lg.shape[0], lg.shape[-2], lg.shape[-1]))
    assert {(s, n, c) for s in C.EVAL_S for n in C.EVAL_N for c in C.EVAL_C} <= seen
    run = next(C.eval_runs(C.case_of('evaluation', 'labels 2^40')))
    assert run['lv'].max() == 2 ** 40 and C.eval_reference(run)[1].max() > 2 ** 32
    assert np.all(next(C.eval_runs(C.case_of('evaluation', 'all -100')))['lm'] == -100)
