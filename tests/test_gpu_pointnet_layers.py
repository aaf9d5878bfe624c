"""GPU: the BatchNorm PointNet (csrc/spg_gemm.hip, spg_narrow.hip, spg_pointnet.hip, spg_convstack.hip) LAYER BY LAYER
at its tile and dispatch edges, against the float64 references and bounds of tests/pointnet_cases.py (whose cases
tests/test_pointnet_cases.py admits and probes on the CPU).  Everything goes through ops.make_pointnet_cfg / ops.pointnet_forward /
ops.pointnet_backward; the workspace is read through spg_pointnet_debug_offset.

* training forward: every layer's raw output against float64 on the device's OWN input to that layer (no ReLU or max-pool near-tie
  can enter, a failure names its layer), its mean / rstd / s / t and the running statistics against the float64 statistics of the
  device's own output, the pooled rows bit for bit against the device's own output and its extremum (max, or min where gamma < 0);
* inference: pooled rows and embeddings against the float64 eval forward, two calls bit-identical;
* backward: every element of every gradient (parameters, global features, an external transform) against the float64 backward with the device's decisions, the decisions admitted by
  the tie rules of test_gpu_baseline_parity._decision_conditioned; a second run bit-identical;
* every case runs under the launch form the library's predicates give for its shape (launch_form); where a shape already runs a
  fallback, switching the spg_tune key that selects it leaves every output bit unchanged.

What this does NOT see: an error a layer makes identically in its stored output and in what the next layer reads of it (the
one-pass first layers hand the first output over in registers).  The end-to-end tests remain the judge of that.

`python tests/test_gpu_pointnet_layers.py` prints the measured figures (profiles/pointnet_layer_errors.txt)."""
import contextlib
import ctypes
import io

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import pointnet_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = {c['name']: c for c in C.cases()}
TRAIN = [n for n, c in CASES.items() if c['mode'] == 'train']
EVAL = [n for n, c in CASES.items() if c['mode'] == 'eval']
BACKWARD = [n for n in TRAIN if not CASES[n]['ordinary']]      # (`ordinary`: no conditioning of the case data, forward checks only)


def make_cfg(case):
    from superpoint_graph_amd import ops
    wd, stn = case['widths'], C.has_stn(case)
    return ops.make_pointnet_cfg(case['nfeat'], case['nfeat_stn'], case['nglob'], case['P'], wd['stn_conv'] if stn else [],
                                 wd['stn_fc'] if stn else [], wd['conv'], wd['fc'], False, C.EPS, C.MOMENTUM)


def device_groups(case, state):
    """-> ({key: device tensor}, one (weight, bias, bn.weight, bn.bias, running_mean, running_var) per layer).  Fresh copies: a
    training forward updates the running statistics in place."""
    P = {k: v.to(DEV) for k, v in state.items()}
    return P, [(P[l['w'] + '.weight'], P[l['w'] + '.bias']) + (tuple(P[l['n'] + s] for s in ('.weight', '.bias', '.running_mean', '.running_var'))
                                                              if l['bn'] else (None,) * 4) for l in C.layers_of(case)]


class tuned:
    """spg_tune keys for the length of a block; restored on the way out."""

    def __init__(self, hip, keys):
        self.hip, self.keys, self.old = hip, dict(keys), {}

    def __enter__(self):
        for k, v in self.keys.items():
            self.old[k] = self.hip.spg_tune(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.hip.spg_tune(k, v)


def _buf(hip, st, training, layer, what, n, dtype=torch.float32):
    off = hip.spg_pointnet_debug_offset(ctypes.byref(st.cfg), st.B, training, layer, what)
    assert off >= 0, (layer, what)
    return st.ws[off:off + 4 * n].view(dtype).cpu().clone()


def _pooled(hip, case, st, training):
    out = {}
    for seg, code in (('stn', -1), ('main', -2)):
        if seg == 'stn' and not C.has_stn(case):
            continue
        last = [l for l in C.layers_of(case) if l['seg'] == seg and l['pooled']][0]
        Cc, ng, B = last['cout'], case['nglob'] if seg == 'main' else 0, case['B']
        ld = int(hip.spg_pointnet_debug_offset(ctypes.byref(st.cfg), B, training, code, 2))
        assert ld >= Cc + ng and ld % 4 == 0
        out[seg] = dict(pooled=_buf(hip, st, training, code, 0, B * ld).view(B, ld)[:, :Cc + ng].contiguous(),
                        aidx=_buf(hip, st, training, code, 1, B * ld, torch.int32).view(B, ld)[:, :Cc].long().contiguous())
    return out


def read_forward(hip, case, st, emb, P):
    """The training forward's workspace as pointnet_cases' fw."""
    B, Pn = case['B'], case['P']
    L = C.layers_of(case)
    fw = dict(layers=[], running={}, emb=emb.cpu().clone())
    for l in L:
        rows = B * Pn if l['kind'] == 'conv' else B
        # (the library writes the last layer's output into `emb` itself: there is no second copy to compare the embedding with)
        rec = dict(y=fw['emb'] if l['i'] == len(L) - 1 else _buf(hip, st, 1, l['i'], 0, rows * l['cout']).view(rows, l['cout']))
        if l['bn']:
            rec.update(s=_buf(hip, st, 1, l['i'], 1, l['cout']), t=_buf(hip, st, 1, l['i'], 2, l['cout']),
                       mean=_buf(hip, st, 1, l['i'], 3, l['cout']), rstd=_buf(hip, st, 1, l['i'], 4, l['cout']))
            fw['running'][l['n']] = (P[l['n'] + '.running_mean'].cpu().clone(), P[l['n'] + '.running_var'].cpu().clone())
        fw['layers'].append(rec)
    fw.update(_pooled(hip, case, st, 1))
    return fw


def run_train(hip, case, built, keys=None):
    """One training forward + backward -> (fw, {parameter key: gradient} + 'd_glob')."""
    from superpoint_graph_amd import ops
    state, clouds, glob, w = built
    with tuned(hip, {**case['keys'], **(keys or {})}):
        P, groups = device_groups(case, state)
        emb, st = ops.pointnet_forward(make_cfg(case), clouds.to(DEV), None if glob is None else glob.to(DEV), groups, True, case['update_times'],
                                       ext_transform=P.get('ext_transform'))
        fw = read_forward(hip, case, st, emb, P)
        gg, g_T, g_glob = ops.pointnet_backward(st, groups, w.to(DEV), want_input_grads=True)
        torch.cuda.synchronize()
    assert (g_T is not None) == case['ext'] and (g_glob is not None) == (glob is not None)
    grads = {}
    for l, row in zip(C.layers_of(case), gg):
        grads[l['w'] + '.weight'], grads[l['w'] + '.bias'] = row[0].cpu(), row[1].cpu()
        if l['bn']:
            grads[l['n'] + '.weight'], grads[l['n'] + '.bias'] = row[2].cpu(), row[3].cpu()
    if g_glob is not None:
        grads['d_glob'] = g_glob.cpu()
    if g_T is not None:
        grads['d_T'] = g_T.cpu()
    return fw, grads


def run_eval(hip, case, built):
    from superpoint_graph_amd import ops
    state, clouds, glob, _ = built
    P, groups = device_groups(case, state)
    emb, st = ops.pointnet_forward(make_cfg(case), clouds.to(DEV), None if glob is None else glob.to(DEV), groups, False,
                                   ext_transform=P.get('ext_transform'))
    got = {'emb': emb.cpu().clone()}
    got.update({seg + '.pooled': v['pooled'] for seg, v in _pooled(hip, case, st, 0).items()})
    for k in state:      # inference leaves the parameters and the running statistics alone
        assert torch.equal(P[k].cpu(), state[k]), k
    return got


def _flat(fw, grads):
    out = {'emb': fw['emb']}
    for i, rec in enumerate(fw['layers']):
        out.update({f'layer{i}.{k}': v for k, v in rec.items()})
    for seg in ('stn', 'main'):
        if seg in fw:
            out.update({f'{seg}.{k}': v for k, v in fw[seg].items()})
    for n, (rm, rv) in fw['running'].items():
        out[n + '.running_mean'], out[n + '.running_var'] = rm, rv
    out.update({'grad ' + k: v for k, v in grads.items()})
    return out


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                        b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), f'{what}: {k}'


@pytest.fixture(scope='module')
def runs(hip):
    """One device run per training case, shared by the forward and the backward test (the reference data are left unchanged)."""
    cache = {}

    def get(name):
        if name not in cache:
            case = CASES[name]
            assert C.launch_form(case) == case['form'], name
            built = C.build(case)
            cache[name] = (built,) + run_train(hip, case, built)
        return cache[name]
    return get


@pytest.mark.parametrize('name', TRAIN)
def test_training_forward_layer_by_layer(hip, runs, name):
    case = CASES[name]
    (state, clouds, glob, w), fw, _ = runs(name)
    C.check_forward(case, state, clouds, glob, fw)


def _expected(exceeds, reason):
    """xfail(strict=True) for ONE figure: everything before this call has been asserted; the figure exceeds its bound -> expected
    failure with the measured value, it meets the bound -> the exception is stale and the test fails."""
    if exceeds:
        pytest.xfail(reason)
    pytest.fail('XPASS(strict): the recorded exception no longer occurs: ' + reason)


@pytest.mark.parametrize('name', BACKWARD)
def test_backward_with_the_decisions_held_equal(hip, runs, name):
    case = CASES[name]
    (state, clouds, glob, w), fw, grads = runs(name)
    excess = {} if name in C.ILL_CONDITIONED else None
    C.check_backward(case, state, clouds, glob, w, fw, grads, excess=excess)
    if excess is not None:      # (every gradient finite: asserted above)
        _expected(excess['tie'] > 1.0 or excess['grad'] > 1.0, f'{C.ILL_CONDITIONED[name]}; measured {_rounded(excess)}')


def test_constant_channel_normalises_to_beta(hip, runs):
    """Edge c.  Asserted: y is the bias on every row and the batch mean within 1e-6 of it in both layers, the FC layer's channel within
    rstd ulp(y) of beta.  Expected failure: the 64 -> 128 convolution's channel (measured 4.2 x; profiles/pointnet_layer_errors.txt)."""
    name = 'train B3 P128 edge c'
    (state, clouds, glob, w), fw, _ = runs(name)
    ratios = C.constant_channel(CASES[name], state, fw)
    assert set(ratios) == {C.EDGE_C_CONV, C.EDGE_C_FC} and ratios[C.EDGE_C_FC] <= 1.0, ratios
    _expected(ratios[C.EDGE_C_CONV] > 1.0, f'{C.CONSTANT_XFAIL}; measured {ratios[C.EDGE_C_CONV]:.2f} of rstd ulp(y)')


@pytest.mark.parametrize('name', TRAIN)
def test_training_step_is_deterministic_and_fallback_keys_are_neutral(hip, runs, name):
    case = CASES[name]
    built, fw, grads = runs(name)
    first = _flat(fw, grads)
    _same_bits(first, _flat(*run_train(hip, case, built)), f'{name}: second run')
    for keys in C.neutral_keys(case):
        _same_bits(first, _flat(*run_train(hip, case, built, keys)), f'{name}: spg_tune {keys}')


@pytest.mark.parametrize('name', EVAL)
def test_inference(hip, name):
    case = CASES[name]
    assert C.launch_form(case) == case['form']
    built = C.build(case)
    got = run_eval(hip, case, built)
    C.check_eval(case, built[0], built[1], built[2], got)
    _same_bits(got, run_eval(hip, case, built), f'{name}: second call')


def test_one_feature_above_the_gram_kernels_is_refused(hip):
    """nfeat = SPG_GRAM_MAXF + 1 = 33 is outside the library's range: refused before anything is launched, in both modes."""
    from superpoint_graph_amd import ops
    case = C._case('refused', 'train', 3, 128, None, nfeat=C.GRAM_MAXF + 1, nfeat_stn=C.GRAM_MAXF + 1)
    state, clouds, glob, _ = C.build(case)
    _, groups = device_groups(case, state)
    for training in (True, False):
        with pytest.raises(RuntimeError, match='nfeat'):
            ops.pointnet_forward(make_cfg(case), clouds.to(DEV), glob.to(DEV), groups, training)


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def _rounded(excess):
    return {k: round(float(v), 2) for k, v in excess.items()}


def report():
    from superpoint_graph_amd import _lib
    hip = _lib.lib()
    lines = ['# python tests/test_gpu_pointnet_layers.py',
             '# Per case (## case, launch form): one row per tensor, one column per layer in the library\'s order (STN convolutions, STN FC layers,',
             '# projection, convolutions, FC layers).  A cell is  worst |device - float64 reference| / that error over its bound / the same ratio',
             '# of the float32 CPU stand-in of tests/pointnet_cases.py (row y: of a float32 CPU evaluation of the same layer on the same input);',
             '# n marks a gradient without signal (conftest.noise_grad), - a tensor the layer does not have.  Bounds: y: 2 (K + 4) 2^-24',
             '# (sum |a||w| + |b|); mean: 1e-6 rms; rstd: 1e-6 kappa; s, t, rmean, rvar (running statistics): these propagated; dW, db, dgamma, dbeta,',
             '# d_glob, d_T and the inference rows: 1e-4 |ref| + 1e-5 max|ref| per element (conftest.assert_elementwise), the gradients with the',
             '# decisions held equal; n: 1e-5.  The pooling checks are exact and have no figure.  A case that fails a',
             '# check lists its figures up to the failure, then the failure.']
    top = (0.0, '', '')
    for name, case in CASES.items():
        built = C.build(case)
        state, clouds, glob, w = built
        dev, cpu, note = [], [], []
        try:
            with contextlib.redirect_stdout(io.StringIO()):      # (the checks print every figure: the table holds them)
                if case['mode'] == 'eval':
                    C.check_eval(case, state, clouds, glob, run_eval(hip, case, built), dev)
                else:
                    fw, grads = run_train(hip, case, built)
                    sfw = C.standin_forward(case, state, clouds, glob)
                    C.check_forward(case, state, clouds, glob, sfw, report=cpu)
                    C.check_forward(case, state, clouds, glob, fw, report=dev)
                    if case['ordinary']:
                        note.append('forward checks only (no conditioning of the case data)')
                    else:
                        ill = name in C.ILL_CONDITIONED
                        ex_cpu, ex_dev = ({}, {}) if ill else (None, None)
                        C.check_backward(case, state, clouds, glob, w, sfw, C.standin_backward(case, state, clouds, glob, w, sfw), cpu, ex_cpu)
                        counts = C.check_backward(case, state, clouds, glob, w, fw, grads, dev, ex_dev)
                        note.append(f'decisions: ReLU {counts[0]} / {counts[1]} differ from float64, max-pool {counts[2]} / {counts[3]}')
                        if ill:
                            note.append(f'EXPECTED FAILURE, recorded and not asserted: {C.ILL_CONDITIONED[name]}')
                            note.append(f'  device: {_rounded(ex_dev)}; float32 CPU: {_rounded(ex_cpu)}  (tie: worst distance / admitted; count: most differing ReLU '
                                        'decisions of a layer; grad: worst error / bound; noise: largest no-signal value / 1e-5)')
                if case['edge'] == 'c' and case['mode'] == 'train':
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        ratios = C.constant_channel(case, state, fw)
                    if ratios[C.EDGE_C_CONV] > 1.0:
                        note.append('EXPECTED FAILURE (constant channel of the convolution): ' + C.CONSTANT_XFAIL)
                    note += [ln.split(': ', 1)[1] for ln in buf.getvalue().splitlines()]
        except AssertionError as e:
            note.append('FAILS: ' + str(e).splitlines()[0])
        cpu_of = {(ident, what): ratio for ident, what, _, ratio, _ in cpu}
        L = C.layers_of(case)
        where = {l['w'] + '.weight': (l['i'], 'dW') for l in L}
        where.update({l['w'] + '.bias': (l['i'], 'db') for l in L})
        where.update({l['n'] + '.weight': (l['i'], 'dgamma') for l in L if l['bn']})
        where.update({l['n'] + '.bias': (l['i'], 'dbeta') for l in L if l['bn']})
        short = {'bn.mean': 'mean', 'bn.rstd': 'rstd', 'bn.s': 's', 'bn.t': 't', 'running_mean': 'rmean', 'running_var': 'rvar'}
        cells, other = {}, []
        for ident, what, err, ratio, c in dev:
            c = c if what in ('y', 'eval') else cpu_of.get((ident, what), float('nan'))
            cell = '/'.join([f'{err:.0e}'.replace('e-0', 'e-').replace('e+00', '')] + [f'{v:.2f}'.lstrip('0') for v in (ratio, c)]) + ('n' if what == 'noise' else '')
            if not (name in C.ILL_CONDITIONED and what in ('grad', 'noise')):      # (the recorded exception has its own line)
                top = max(top, (ratio, name, f'{ident} {what}'))
            if isinstance(ident, int):
                cells[(ident, short.get(what, what))] = cell
            elif ident in where:
                cells[where[ident]] = cell
            else:
                other.append(f'{ident} {cell}')
        rows = [f"{r:7s}" + ' '.join(f"{cells.get((l['i'], r), '-'):>13s}" for l in L)
                for r in ('y', 'mean', 'rstd', 's', 't', 'rmean', 'rvar', 'dW', 'db', 'dgamma', 'dbeta') if any(k[1] == r for k in cells)]
        if case['mode'] == 'eval' and not note:      # (one line per inference case)
            lines.append(f"## {name}   {case['form']}   " + '   '.join(other))
            continue
        if other:
            rows.append('   '.join(other))
        lines += [f"## {name}   {case['form']}"] + [f'#  {n}' for n in note] + rows
    lines += ['', f'## worst device ratio outside the recorded exceptions: {top[0]:.3f}  {top[1]}: {top[2]}']
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
