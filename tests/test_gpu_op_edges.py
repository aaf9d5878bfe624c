"""GPU: the small operators of the training step at their edges, element by element against the float64 references of
tests/op_cases.py (whose cases tests/test_op_cases.py admits and probes on the CPU), through the C ABI:

* GRUCellEx / LSTMCellEx (learning.modules; ops.lstm_cell_bwd with grad_cy = NULL) for all four (layernorm, ingate) pairs at
  n = 1, 3, 5, 64 rows of unit, 1e-2, 1e-3, saturating and exactly-zero aggregate / hidden / cx: outputs, input gradients and
  every parameter gradient;
* ops.cross_entropy at row counts around its 64-row tiles and 1024-row stride, logits at offsets 1e4 / -3e4, a -inf entry,
  ignored / single / no labelled rows, a zero class weight, class indices outside [0, C): loss, gradient, normaliser; and
  spg_cross_entropy_fwd_bwd bit-identical to spg_cross_entropy_fwd + spg_cross_entropy_bwd at every shape;
* spg_adam_clamp_step_scaled around its 256-thread blocks: gradients of 1e-15 ... 1e2, exact zeros, +-clip, beyond the clip, weight
  decay, grad_div, step 1 and step 1000: p, the stored gradient, both moments;
* ops.linear_dgrad, ops.colsum, ops.linear_wgrad_bias at the column sum's row-group / slice edges, and ops.linear_backward
  bit-identical to the separate launches with and without dx and dbias.

The bound is conftest.assert_elementwise with its defaults for every element of every tensor; no case is left out and no element
is masked.  `python tests/test_gpu_op_edges.py` prints the measured figures (profiles/op_edges_errors.txt)."""
import functools

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import op_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CELL_CASES = {c['name']: c for c in C.cell_cases()}
CE_CASES = {c['name']: c for c in C.ce_cases()}
ADAM_CASES = {c['name']: c for c in C.adam_cases()}
DENSE_CASES = {c['name']: c for c in C.dense_cases()}
EVAL = {'cell': C.cell_eval, 'ce': C.ce_reference, 'adam': C.adam_eval, 'dense': C.dense_eval}
TABLE = {'cell': CELL_CASES, 'ce': CE_CASES, 'adam': ADAM_CASES, 'dense': DENSE_CASES}


@functools.lru_cache(maxsize=None)
def reference(op, name):
    """The float64 reference of a case: computed once, shared by the tests and the table."""
    return EVAL[op](TABLE[op][name], torch.float64)


def judge(op, name, got):
    """Prints each figure, then asserts the bound on every tensor of the case."""
    ref = reference(op, name)
    for k, (err, ratio) in C.measure(got, ref).items():
        print(f'{name}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound')
    for k in ref:
        C.assert_bound(got[k], ref[k], f'{name}: {k}')


# ---------------------------------------------------------------------------------------------------------------------
# GRU / LSTM cell
# ---------------------------------------------------------------------------------------------------------------------
def run_cell(case):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import modules
    cls = modules.GRUCellEx if case['kind'] == 'gru' else modules.LSTMCellEx
    cell = cls(32, 32, bias=True, layernorm=case['layernorm'], ingate=case['ingate'])
    cell.load_state_dict(case['params'])
    cell = cell.to(DEV)
    xi, xh, xc = [case[k].to(DEV).requires_grad_(True) for k in ('inp', 'hid', 'cx')]
    gh, gc = case['gh'].to(DEV), case['gc'].to(DEV)
    names = ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh', 'ig.weight', 'ig.bias')
    if case['kind'] == 'gru':
        hy = cell(xi, xh)
        hy.backward(gh)
        res = {'hy': hy, 'd_input': xi.grad, 'd_hidden': xh.grad}
    elif case['grad_cy']:
        hy, cy = cell(xi, (xh, xc))
        torch.autograd.backward([hy, cy], [gh, gc])
        res = {'hy': hy, 'cy': cy, 'd_input': xi.grad, 'd_hidden': xh.grad, 'd_cx': xc.grad}
    else:           # no gradient enters through cy: a NULL pointer in the C ABI (autograd would hand the kernel a tensor of zeros)
        params = [None if p is None else p.detach() for p in cell.param_tensors()]
        hy, cy = ops.lstm_cell_fwd(xi.detach(), xh.detach(), xc.detach(), params, case['layernorm'], case['ingate'])
        di, dh, dc, grads = ops.lstm_cell_bwd(xi.detach(), xh.detach(), xc.detach(), gh, None, params, case['layernorm'], case['ingate'])
        res = {'hy': hy, 'cy': cy, 'd_input': di, 'd_hidden': dh, 'd_cx': dc}
        res.update({'d_' + k: g for k, g in zip(names, grads) if g is not None})
        return {k: v.detach().cpu() for k, v in res.items()}
    res.update({'d_' + k: p.grad for k, p in zip(names, cell.param_tensors()) if p is not None})
    return {k: v.detach().cpu() for k, v in res.items()}


@pytest.mark.parametrize('name', list(CELL_CASES))
def test_cell_edges(hip, name):
    judge('cell', name, run_cell(CELL_CASES[name]))


# ---------------------------------------------------------------------------------------------------------------------
# weighted cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def run_ce(case):
    from superpoint_graph_amd import ops
    x = case['logits'].to(DEV).requires_grad_(True)
    w = None if case['weight'] is None else case['weight'].to(DEV)
    loss, norm = ops.cross_entropy(x, case['target'].to(DEV), weight=w, reduction=case['reduction'], return_normaliser=True)
    norm = norm.clone()
    (loss * case['upstream']).backward()
    return {'loss': loss.detach().cpu(), 'grad': x.grad.cpu(), 'normaliser': norm[0].cpu()}


def run_ce_launches(case):
    """-> ({loss, lse, normaliser, grad} of spg_cross_entropy_fwd + spg_cross_entropy_bwd with an upstream gradient of 1, the same
    of the single launch spg_cross_entropy_fwd_bwd)."""
    from superpoint_graph_amd._lib import check, lib
    N, C_ = case['N'], case['C']
    x, t = case['logits'].to(DEV), case['target'].to(DEV)
    w = None if case['weight'] is None else case['weight'].to(DEV)
    wp = None if w is None else w.data_ptr()
    mean = int(case['reduction'] == 'mean')
    st = torch.cuda.current_stream().cuda_stream
    one = torch.ones(1, device=DEV)
    out = []
    for single in (False, True):
        loss, lse, wsum, grad = [torch.full(s, 7.0, device=DEV) for s in ((1,), (N,), (1,), (N, C_))]
        if single:
            check(lib().spg_cross_entropy_fwd_bwd(x.data_ptr(), t.data_ptr(), wp, N, C_, C.IGNORE, mean, loss.data_ptr(), lse.data_ptr(),
                                                  wsum.data_ptr(), grad.data_ptr(), st), 'spg_cross_entropy_fwd_bwd')
        else:
            check(lib().spg_cross_entropy_fwd(x.data_ptr(), t.data_ptr(), wp, N, C_, C.IGNORE, mean, loss.data_ptr(), lse.data_ptr(),
                                              wsum.data_ptr(), st), 'spg_cross_entropy_fwd')
            check(lib().spg_cross_entropy_bwd(x.data_ptr(), t.data_ptr(), wp, lse.data_ptr(), wsum.data_ptr(), one.data_ptr(), N, C_,
                                              C.IGNORE, mean, grad.data_ptr(), st), 'spg_cross_entropy_bwd')
        out.append({'loss': loss.cpu(), 'lse': lse.cpu(), 'normaliser': wsum.cpu(), 'grad': grad.cpu()})
    return out


def _ce_names(N, C_):
    return [n for n, c in CE_CASES.items() if (c['N'], c['C']) == (N, C_)]


@pytest.mark.parametrize('N,C_', C.CE_SHAPES)
def test_cross_entropy_edges(hip, N, C_):
    for name in _ce_names(N, C_):
        case = CE_CASES[name]
        got = run_ce(case)
        judge('ce', name, got)
        if 'all ignored' in name or case['upstream'] == 0:
            assert float(got['grad'].abs().max()) == 0.0, name
        if case['bad']:
            bad = (case['target'] != C.IGNORE) & ~C._ce_valid(case)
            assert float(got['grad'][bad].abs().max()) == 0.0 and bool(torch.isnan(got['loss'])), name


@pytest.mark.parametrize('N,C_', C.CE_SHAPES)
def test_cross_entropy_single_launch_bit_identical(hip, N, C_):
    """spg_cross_entropy_fwd_bwd (the launch of the fused step) against the forward + backward pair: every bit of the loss, the
    log-sum-exp, the normaliser and the gradient -- at row counts with a partial 64-row tile (NaN losses included)."""
    bits = lambda v: v.view(torch.int32)
    for name in _ce_names(N, C_):
        pair, single = run_ce_launches(CE_CASES[name])
        for k in pair:
            assert torch.equal(bits(pair[k]), bits(single[k])), f'{name}: {k} differs between the two launches and the single one'
        ref, upstream = reference('ce', name), CE_CASES[name]['upstream']
        C.assert_bound(single['loss'][0], ref['loss'], f'{name}: loss')
        if upstream != 0:                   # the reference gradient belongs to upstream * loss
            C.assert_bound(single['grad'], ref['grad'] / upstream, f'{name}: grad')


# ---------------------------------------------------------------------------------------------------------------------
# clamp + Adam
# ---------------------------------------------------------------------------------------------------------------------
def run_adam(case):
    from superpoint_graph_amd._lib import check, lib
    p, g, m, v = [case[k].to(DEV).clone() for k in ('p', 'g', 'm', 'v')]
    div = None if case['div'] is None else case['div'].to(DEV)
    b1, b2 = C.ADAM_BETAS
    check(lib().spg_adam_clamp_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), case['n'], C.ADAM_LR, b1, b2, C.ADAM_EPS,
                                           case['wd'], case['clip'], case['step'], None if div is None else div.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), 'spg_adam_clamp_step_scaled')
    return C.split_adam(p.cpu(), g.cpu(), m.cpu(), v.cpu())


@pytest.mark.parametrize('n', C.ADAM_SIZES)
def test_adam_edges(hip, n):
    assert hip.spg_ecc_persistent_errors() == 0            # (a pending time-out word would withhold every update)
    for name, case in ADAM_CASES.items():
        if case['n'] == n:
            judge('adam', name, run_adam(case))


# ---------------------------------------------------------------------------------------------------------------------
# dense-layer backward
# ---------------------------------------------------------------------------------------------------------------------
def run_dense(case):
    """-> (results of the separate launches incl. the column sums of both entry points, the device tensors for the bit comparison)."""
    from superpoint_graph_amd import ops
    DY, X, W = [case[k].to(DEV) for k in ('dy', 'x', 'w')]
    dx = ops.linear_dgrad(DY, W)
    db_colsum = ops.colsum(DY)
    dw, db = ops.linear_wgrad_bias(DY, X)
    return {'dx': dx.cpu(), 'dW': dw.cpu(), 'dbias': db_colsum.cpu(), 'dbias (wgrad_bias)': db.cpu()}, (DY, X, W, dx, dw, db)


def dense_figures(case):
    got, _ = run_dense(case)
    ref = dict(reference('dense', case['name']))
    ref['dbias (wgrad_bias)'] = ref['dbias']
    return got, ref


@pytest.mark.parametrize('name', list(DENSE_CASES))
def test_dense_backward_edges(hip, name):
    from superpoint_graph_amd import ops
    case = DENSE_CASES[name]
    got, (DY, X, W, dx, dw, db) = run_dense(case)
    ref = reference('dense', name)
    for k, r in (('dx', 'dx'), ('dW', 'dW'), ('dbias', 'dbias'), ('dbias (wgrad_bias)', 'dbias')):
        err, ratio = C.bound_ratio(got[k], ref[r])
        print(f'{name}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound')
    for k, r in (('dx', 'dx'), ('dW', 'dW'), ('dbias', 'dbias'), ('dbias (wgrad_bias)', 'dbias')):
        C.assert_bound(got[k], ref[r], f'{name}: {k}')
    # the grouped launch runs the unchanged bodies of the kernels it replaces (csrc/spg_gemm.h): every bit of the separate launches
    for need_dx in (True, False):
        for has_bias in (True, False):
            bx, bw, bb = ops.linear_backward(DY, X, W, need_dx=need_dx, has_bias=has_bias)
            what = f'{name}: linear_backward(need_dx={need_dx}, has_bias={has_bias})'
            assert (bx is None) == (not need_dx) and (bb is None) == (not has_bias), what
            assert torch.equal(bw, dw), what + ': dW differs from linear_wgrad_bias'
            if need_dx:
                assert torch.equal(bx, dx), what + ': dx differs from linear_dgrad'
            if has_bias:
                assert torch.equal(bb, db), what + ': dbias differs from linear_wgrad_bias'


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    lines = ['# python tests/test_gpu_op_edges.py',
             '# per case and tensor: worst |device - float64 reference|, worst error / bound of the device, the same ratio of the float32',
             '# CPU evaluation of the reference.  bound = 1e-4 |ref| + 1e-5 max|ref| per element (conftest.assert_elementwise).',
             f'# saturating row scale of the cell cases: s = {C.SAT_SCALE:g}',
             f"{'case':72s} {'tensor':20s} {'abs error':>10s} {'device':>8s} {'cpu f32':>8s}"]
    top = {}

    def rows(op, name, got, ref, cpu):
        dev_f, cpu_f = C.measure(got, ref), C.measure(cpu, ref)
        for k in ref:
            lines.append(f'{name:72s} {k:20s} {dev_f[k][0]:10.3e} {dev_f[k][1]:8.3f} {cpu_f[k][1]:8.3f}')
            top[op] = max(top.get(op, (0.0, '', '')), (dev_f[k][1], name, k))

    for title, op, run in (('GRU / LSTM cell', 'cell', run_cell), ('weighted cross entropy', 'ce', run_ce), ('clamp + Adam', 'adam', run_adam)):
        lines += ['', f'## {title}']
        for name, case in TABLE[op].items():
            rows(op, name, run(case), reference(op, name), EVAL[op](case, torch.float32))
    lines += ['', '## dense-layer backward']
    for name, case in DENSE_CASES.items():
        got, ref = dense_figures(case)
        cpu = dict(C.dense_eval(case, torch.float32))
        cpu['dbias (wgrad_bias)'] = cpu['dbias']
        rows('dense', name, got, ref, cpu)
    lines += ['', '## worst device ratio per operator'] + [f'{op:6s} {r:8.3f}  {name}: {k}' for op, (r, name, k) in top.items()]
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
