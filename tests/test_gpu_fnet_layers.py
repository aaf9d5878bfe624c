"""GPU: the filter-generating network of the RNN-ECC module (csrc/spg_eccnet.hip -> spg_dense.h -> the few-row GEMMs, weight-gradient
plan and batched reduction of csrc/spg_gemm.hip) LAYER BY LAYER at its edge-count and width edges, against the float64
references and bounds of tests/fnet_cases.py (whose cases tests/test_fnet_cases.py admits and probes on the CPU).  Everything goes
through ops.make_eccrnn_cfg / ops.eccrnn_forward / ops.eccrnn_backward with one GRU iteration; the forward workspace is read through
spg_eccrnn_debug_offset.

* training: every layer's raw output against float64 on the device's OWN input to that layer, its mean / rstd / s / t and the running
  statistics against the float64 statistics of the device's own output over exactly E rows; the module output against the unconditioned
  float64 module; grad x and every filter-network and cell parameter gradient against the float64 backward with the device's ReLU
  decisions, which may differ from float64's own only on near-ties;
* evaluation: the per-edge filters and the module output against the float64 oracle with the running statistics, which stay untouched;
* a second run of every case is bit-identical (statistics slots that are not cleared, an order-dependent reduction), and so is a run
  under every spg_tune key that must be neutral for the case (fnet_cases.neutral_keys: direct instead of grouped launches always, the
  finalize path where there is no train-mode BatchNorm); slots and finalize launches (key 10) both stay inside the bounds;
* every case reaches the launch-form tokens it is listed for, and with spg_prof_enable the (tag, N, K, launches) rows the library
  records for a forward + backward under key 11 = 1 are the ones fnet_cases.prof_rows predicts;
* one edge in training mode with a BatchNorm is refused.

What this does NOT see: an error a layer makes identically in its stored output and in what the next layer reads of it; the rider path
of spg_train_step (phase 1 / 2 of spg_eccrnn_forward_phase), which stays judged end to end by the one-call step's tests.

`python tests/test_gpu_fnet_layers.py` prints the measured figures (profiles/fnet_layer_errors.txt)."""
import contextlib
import ctypes
import io

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import fnet_cases as C
from test_gpu_pointnet_layers import _same_bits, tuned

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = {c['name']: c for c in C.cases()}
# every layer shape of the table once: the subset for the profile record
PROFILED = ['E65', 'E544 matrix nc64', '[13 160] bn0', 'ef32 [128 64] bn0', 'ef32 [128 64] bn1', 'ef1 [24 40]', '[13 30 20] bn0', 'no hidden ef13 llbias',
            'vector nc8', 'ef4', 'ef33', 'bn0 E64', 'no bn E65']


def device_rows(case, state):
    """-> ({key: device tensor}, the six-pointer rows of the library's tables: one per filter layer, then the cell's).  Fresh copies: a
    training forward updates the running statistics in place."""
    P = {k: v.to(DEV) for k, v in state.items()}
    rows = []
    for l in C.layers_of(case):
        bn = tuple(P[l['n'] + s] for s in ('.weight', '.bias', '.running_mean', '.running_var')) if l['bn'] else (None,) * 4
        rows.append((P[l['lin'] + '.weight'], P[l['lin'] + '.bias'] if l['bias'] else None) + bn)
    rows.append(tuple(P[f'{C.PFX}._cell.{k}'] for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh', 'ig.weight', 'ig.bias')))
    return P, rows


def run(hip, case, built, keys=None):
    """One forward (+ backward in training mode) -> got (fnet_cases' structure), on the host."""
    from superpoint_graph_amd import ops
    L, E, nc = C.layers_of(case), case['E'], case['nc']
    with tuned(hip, {**case['keys'], **(keys or {})}):
        P, rows = device_rows(case, built['state'])
        graph = ops.DeviceGraph(built['idxn'].to(DEV), built['degs'].to(DEV))
        cfg = ops.make_eccrnn_cfg(nc, 1, case['matrix'], True, True, True, list(case['fnet']) + [C.nout(case)], case['bnidx'], case['llbias'], C.EPS, C.MOMENTUM)
        out, st = ops.eccrnn_forward(cfg, graph, built['x'].to(DEV), built['ef'].to(DEV), rows, case['training'], case['update_times'])

        def buf(layer, what, n):
            off = hip.spg_eccrnn_debug_offset(ctypes.byref(cfg), graph.N, E, int(case['training']), layer, what)
            assert off >= 0, (layer, what)
            return st.ws[off:off + 4 * n].view(torch.float32).cpu().clone()
        got = dict(layers=[], running={}, out=out.cpu().clone())
        for l in L:
            rec = dict(y=buf(l['i'], 0, E * l['cout']).view(E, l['cout']))
            if l['bn']:
                rec.update(s=buf(l['i'], 1, l['cout']), t=buf(l['i'], 2, l['cout']))
                if case['training']:
                    rec.update(mean=buf(l['i'], 3, l['cout']), rstd=buf(l['i'], 4, l['cout']))
                got['running'][l['n']] = (P[l['n'] + '.running_mean'].cpu().clone(), P[l['n'] + '.running_var'].cpu().clone())
            got['layers'].append(rec)
        got['filters'] = got['layers'][-1]['y']
        if case['training']:
            grad_x, gg = ops.eccrnn_backward(st, rows, built['go'].to(DEV))
            torch.cuda.synchronize()
            got['grad x'] = grad_x.cpu()
            for l, row in zip(L, gg):
                got['grad ' + l['lin'] + '.weight'] = row[0].cpu()
                if l['bias']:
                    got['grad ' + l['lin'] + '.bias'] = row[1].cpu()
                if l['bn']:
                    got['grad ' + l['n'] + '.weight'], got['grad ' + l['n'] + '.bias'] = row[2].cpu(), row[3].cpu()
            for k, g in zip(('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh', 'ig.weight', 'ig.bias'), gg[-1]):
                got[f'grad {C.PFX}._cell.{k}'] = g.cpu()
        else:
            torch.cuda.synchronize()
            for k, v in built['state'].items():      # inference leaves the parameters and the running statistics alone
                assert torch.equal(P[k].cpu(), v), k
    assert hip.spg_ecc_persistent_errors() == 0
    return got


def _flat(got):
    out = {k: v for k, v in got.items() if torch.is_tensor(v)}
    for i, rec in enumerate(got['layers']):
        out.update({f'layer{i}.{k}': v for k, v in rec.items()})
    for n, (rm, rv) in got['running'].items():
        out[n + '.running_mean'], out[n + '.running_var'] = rm, rv
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_filter_network_layer_by_layer(hip, name):
    case = CASES[name]
    assert set(case['reach']) <= set(C.launch_form(case).split()), name
    built = C.build(case)
    got = run(hip, case, built)
    C.check_all(case, built, got)
    first = _flat(got)
    _same_bits(first, _flat(run(hip, case, built)), f'{name}: second run')
    for keys in C.neutral_keys(case):
        _same_bits(first, _flat(run(hip, case, built, keys)), f'{name}: spg_tune {keys}')


@pytest.mark.parametrize('name', PROFILED)
def test_profile_record_shows_the_predicted_launches(hip, name):
    """The (tag, N, K, launches) rows of one training forward + backward with direct launches (key 11 = 1; a grouped launch is not
    recorded per job) are fnet_cases.prof_rows': the row-GEMMs of the filter network with their shapes, its weight gradients and the
    cell's three (the library records no shape for a weight gradient)."""
    case = CASES[name]
    built = C.build(case)
    want = {(hip.spg_prof_tag(kind, it, jt, x, y, full), n, k): cnt
            for (kind, it, jt, x, y, full, n, k), cnt in C.prof_rows(case, {**case['keys'], C.KEY_NO_GROUP: 1}).items()}
    keys, vals = (ctypes.c_int * (4 * 256))(), (ctypes.c_double * (2 * 256))()
    try:
        hip.spg_prof_read(None, None, None, 1)
        hip.spg_prof_enable(1)
        run(hip, case, built, {C.KEY_NO_GROUP: 1})
        n = hip.spg_prof_read_shapes(keys, vals, 256)
    finally:
        hip.spg_prof_enable(0)
        hip.spg_prof_read(None, None, None, 1)
    seen = {(keys[4 * j], keys[4 * j + 1], keys[4 * j + 2]): keys[4 * j + 3] for j in range(n) if keys[4 * j] >= 1000000}
    assert seen == want, (name, sorted(set(seen.items()) ^ set(want.items())))


def test_one_edge_in_training_mode_is_refused(hip):
    """BatchNorm over one row: the ValueError of ops/model.py (torch's own message), before anything is launched."""
    from superpoint_graph_amd import ops
    case = C._case('one edge', 1, '')
    built = C.build(case)
    _, rows = device_rows(case, built['state'])
    graph = ops.DeviceGraph(built['idxn'].to(DEV), built['degs'].to(DEV))
    cfg = ops.make_eccrnn_cfg(32, 1, False, True, True, True, list(case['fnet']) + [32], 2, 0, C.EPS, C.MOMENTUM)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        ops.eccrnn_forward(cfg, graph, built['x'].to(DEV), built['ef'].to(DEV), rows, True, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    from superpoint_graph_amd import _lib
    hip = _lib.lib()
    lines = ['# python tests/test_gpu_fnet_layers.py',
             '# Per case (## case, launch form of tests/fnet_cases.py): one row per check with the worst |device - float64 reference| over its bound,',
             '# where it stands (layer or tensor), and the same figure of the float32 CPU stand-in.  Bounds: raw: 2 (K + 4) 2^-24 (sum |a||w| + |b|);',
             '# bn.mean: 1e-6 rms; bn.rstd: 1e-6 kappa; bn.s, bn.t, running_mean, running_var: these propagated; eval, grad: 1e-4 |ref| + 1e-5 max|ref|',
             '# per element (conftest.assert_elementwise), the gradients with the decisions held equal; noise (the bias in front of the BatchNorm):',
             '# 1e-5.  A case that fails a check lists its figures up to the failure, then the failure.']
    top = (0.0, '', '')
    top_cpu = (0.0, '', '')
    for name, case in CASES.items():
        built = C.build(case)
        dev, cpu, note = [], [], []
        try:
            with contextlib.redirect_stdout(io.StringIO()):      # (the checks print every figure: the table holds the worst per check)
                n_cpu = C.check_all(case, built, C.standin(case, built), cpu)
                n_dev = C.check_all(case, built, run(hip, case, built), dev)
            if case['training']:
                note.append(f'ReLU decisions that differ from float64: device {n_dev}, float32 CPU {n_cpu}')
            if case['edge'] == 'zero row' and case['training']:
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    C.check_constant(case, built, run(hip, case, built))
                note += [ln.split(': ', 1)[1] for ln in buf.getvalue().splitlines()]
        except AssertionError as e:
            note.append('FAILS: ' + str(e).splitlines()[0])
        lines += [f'## {name}   {C.launch_form(case)}'] + [f'#  {n}' for n in note]
        worst_cpu = {}
        for ident, what, _, ratio, _ in cpu:
            worst_cpu[what] = max(worst_cpu.get(what, 0.0), ratio)
            top_cpu = max(top_cpu, (ratio, name, f'{ident} {what}'))
        worst_dev = {}
        for ident, what, err, ratio, _ in dev:
            if ratio >= worst_dev.get(what, (-1.0,))[0]:
                worst_dev[what] = (ratio, err, ident)
            top = max(top, (ratio, name, f'{ident} {what}'))
        for what, (ratio, err, ident) in worst_dev.items():
            what = 'raw' if what == 'y' else what
            lines.append(f"{what:13s} device {ratio:6.3f} (worst error {err:.3e} at {'layer ' + str(ident) if isinstance(ident, int) else ident})   "
                         f"float32 CPU {worst_cpu.get('y' if what == 'raw' else what, float('nan')):6.3f}")
    lines += ['', f'## worst device ratio: {top[0]:.3f}  {top[1]}: {top[2]}', f'## worst float32 CPU ratio: {top_cpu[0]:.3f}  {top_cpu[1]}: {top_cpu[2]}']
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
