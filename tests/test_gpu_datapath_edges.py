"""GPU: the units that feed and drain the training step -- the device loader (ops.load_superpoints, ops.loader_random), batch
construction (ops.set_batch, ops.gather_rows, ops.batch_graph_build from host and from device inputs, ops.edge_features) and the
evaluation accounting (ops.eval_accumulate) -- at their launch-shape and value edges, against the references and bounds of
tests/datapath_cases.py (whose tables tests/test_datapath_cases.py admits and probes on the CPU).  One parametrised test per entry
point; every call runs twice and the two results must agree bit for bit.

What this does NOT see: the arrival order inside a bucket (integer atomics; only the sorted result is visible); the contents of the
outputs after a malformed edge list (only the flag, and that the next call is clean); `size/d` on the uint64 point count, where numpy
wraps modulo 2^64 and the device's float64 path does not; the host-stream path of learning/spg.py load_superpoints_device, which stays
judged by tests/test_gpu_loader.py.

`python tests/test_gpu_datapath_edges.py` prints the measured worst ratio per entry point and check (profiles/datapath_errors.txt)."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import datapath_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return None if t is None else t.cpu().numpy()


class Device:
    """datapath_cases' device interface (numpy in, numpy out) on the ops of the package"""

    def __init__(self, hip):
        from superpoint_graph_amd import ops
        self.hip, self.ops = hip, ops

    def load(self, points, offsets, slot, sidx, colmap, norm, n_valid, M=None, noise=None):
        clouds, diam = self.ops.load_superpoints(_t(points), _t(offsets), _t(slot), _t(sidx), colmap, bool(norm), n_valid, _t(M), _t(noise))
        return _n(clouds), _n(diam)

    def random(self, counts, ids, slot, *args):
        return tuple(_n(r) for r in self.ops.loader_random(_t(counts), _t(ids), _t(slot), *args))

    def set_batch(self, edges, n):
        idxn, degs, perm, err = self.ops.set_batch(_t(edges), n)
        if int(err):                      # flagged: the other buffers hold nothing defined
            return None, None, None, 1
        return _n(idxn), _n(degs), _n(perm), 0

    def gather(self, src, perm, cols=None):
        if cols is None or cols == src.shape[1]:
            return _n(self.ops.gather_rows(_t(src), _t(perm)))
        from superpoint_graph_amd._lib import check      # a source wider than the gathered rows: the C ABI's ld_src
        s, p = _t(src), _t(perm)
        dst = torch.empty(len(perm), cols, dtype=torch.float32, device=DEV)
        check(self.hip.spg_gather_rows(s.data_ptr(), src.shape[1], p.data_ptr(), len(perm), cols, dst.data_ptr(), cols, torch.cuda.current_stream().cuda_stream),
              'spg_gather_rows')
        return _n(dst)

    def build(self, edges, feats, n, on_device):
        e, f = torch.from_numpy(edges), torch.from_numpy(feats)
        built = self.ops.batch_graph_build(e.to(DEV), f.to(DEV), n) if on_device else self.ops.batch_graph_build(e, f, n)
        assert built is not None
        idxn, degs, fs, graph, err = built
        if int(err):                      # flagged: the other buffers hold nothing defined
            return dict(err=1)
        rowptr, src, dst, rev_rowptr, rev = graph.export()
        return dict(err=0, hdr=_n(graph.hdr), idxn=_n(idxn), degs=_n(degs), feats=_n(fs), rowptr=_n(rowptr), src=_n(src), dst=_n(dst),
                    rev_rowptr=_n(rev_rowptr), rev=_n(rev))

    def edge_features(self, columns, edges, mean=None, scale=None):
        cache = {}
        cols = [(k, None if t is None else cache.setdefault(id(t), _t(t)), c) for k, t, c in columns]
        return _n(self.ops.edge_features(cols, _t(edges), _t(mean), _t(scale)))

    def evaluate(self, logits, label_mode, label_vec, confusion, counters):
        cm, cnt = _t(confusion), _t(counters)
        pred = self.ops.eval_accumulate(_t(logits), _t(label_mode), _t(label_vec), cm, cnt)
        return _n(pred), _n(cm), _n(cnt)


def _run(hip, table, name, report=None):
    report = [] if report is None else report
    C.TABLES[table][1](C.case_of(table, name), C.Twice(Device(hip)), report)
    assert report, name
    return report


def _names(table):
    return [c['name'] for c in C.TABLES[table][0]()]


@pytest.mark.parametrize('name', _names('loader'))
def test_load_superpoints(hip, name):
    _run(hip, 'loader', name)


@pytest.mark.parametrize('name', _names('random'))
def test_loader_random(hip, name):
    _run(hip, 'random', name)


@pytest.mark.parametrize('name', _names('batch'))
def test_batch_builders(hip, name):
    _run(hip, 'batch', name)


@pytest.mark.parametrize('name', _names('features'))
def test_edge_features(hip, name):
    _run(hip, 'features', name)


@pytest.mark.parametrize('name', _names('evaluation'))
def test_eval_accumulate(hip, name):
    _run(hip, 'evaluation', name)


def test_confusion_matrix_class_on_a_tie_case(hip):
    """ConfusionMatrix.count_predicted_batch_device (what the evaluation loop calls): ties, NaN rows and two accumulating calls"""
    from superpoint_graph_amd.learning import metrics
    run = next(C.eval_runs(C.case_of('evaluation', 'two calls')))
    wpred, wcm, wcnt = C.eval_reference(run)
    m = metrics.ConfusionMatrix(run['logits'].shape[-1])
    for k in (1, 2):
        pred = m.count_predicted_batch_device(_t(run['lv']), _t(run['logits']), _t(run['lm']))
        assert np.array_equal(_n(pred), wpred) and np.array_equal(m.confusion_matrix, k * wcm) and m.accuracy_counts() == tuple(k * wcnt)


def test_empty_outputs_are_returned_without_a_launch(hip):
    """No superpoint of ptn_minpts points, no edge, no superpoint to score: empty results, no 'null pointer' refusal."""
    dev = Device(hip)
    for run in C.loader_runs(C.case_of('loader', 'no superpoint')):
        clouds, diam = dev.load(run['points'], run['offsets'], run['slot'], run['sidx'], run['colmap'], 1, 0)
        assert clouds.shape == (0, 14, 128) and diam.shape == (0,)
    columns, edges, mean, scale = C.ef_build(C.case_of('features', 'E0'))
    assert dev.edge_features(columns, edges, mean, scale).shape == (0, len(columns))
    cm, cnt = np.full((5, 5), 7, np.int64), np.array([3, 4], np.int64)
    pred, cm2, cnt2 = dev.evaluate(np.zeros((2, 0, 5), np.float32), np.zeros(0, np.int64), np.zeros((0, 5), np.int64), cm, cnt)
    assert pred.shape == (0,) and np.array_equal(cm2, cm) and np.array_equal(cnt2, cnt)


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    from superpoint_graph_amd import _lib
    hip = _lib.lib()
    lines = ['# python tests/test_gpu_datapath_edges.py',
             '# Per entry point and check: the worst |device - reference| over its bound (tests/datapath_cases.py) over all cases, and the case',
             '# and element where it stands.  A bit-exact check reads 0 (identical) or inf.  A case that fails lists the failure.']
    for table, (cases, _) in C.TABLES.items():
        worst, failures, n = {}, [], 0
        for case in cases():
            rep = []
            try:
                _run(hip, table, case['name'], rep)
            except AssertionError as e:
                failures.append('FAILS: ' + str(e).splitlines()[0])
            n += len(rep)
            for name, entry, check, where, ratio in rep:
                if ratio >= worst.get((entry, check), (-1.0,))[0]:
                    worst[(entry, check)] = (ratio, name, where)
        lines.append(f'## {table}: {len(cases())} cases, {n} checks')
        lines += [f'#  {f}' for f in failures]
        for (entry, check), (ratio, name, where) in worst.items():
            lines.append(f'{entry:24s} {check:26s} {ratio:6.3f}' + (f'   ({name}, element {where})' if ratio > 0 else ''))
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
