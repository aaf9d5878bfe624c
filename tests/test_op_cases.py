"""CPU: the cases of tests/op_cases.py (GRU / LSTM cell, weighted cross entropy, clamp + Adam, dense-layer backward) before
the device sees them in tests/test_gpu_op_edges.py:

* every case is ADMITTED: the float32 CPU evaluation of its reference stays within 0.25 of the bound on every compared tensor;
* the builders reach the edges they claim (row classes, exact zeros, closed / open gates, partial tiles);
* the knobbed restatements equal the oracle / torch when every knob is off;
* every deliberately altered reference -- one plausible kernel mistake each, evaluated in float32 on the CPU -- LEAVES the bound
  on at least one case, while the unaltered float32 evaluation of the same restatement stays inside it on all of them.  This
  is what shows that the cases can tell a wrong kernel from a right one; no device code is altered for it."""
import math

import pytest
import torch

import op_cases as C
from oracle import spg_oracle as O

F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------------------------------
_REFERENCES = {}


def _reference(evaluate, case):
    """The float64 reference of a case, computed once for all tests of this module."""
    key = (evaluate.__name__, case['name'])
    if key not in _REFERENCES:
        _REFERENCES[key] = evaluate(case, torch.float64)
    return _REFERENCES[key]


def _admit(cases, evaluate):
    worst = ('', '', 0.0)
    for c in cases:
        ref = _reference(evaluate, c)
        for k, (_, r) in C.measure(evaluate(c, F32), ref).items():
            assert r <= C.ADMIT, f"{c['name']}: {k}: float32 on the CPU is at {r:.3f} of the bound (admission: {C.ADMIT})"
            worst = max(worst, (c['name'], k, r), key=lambda w: w[2])
    print('worst float32 / bound:', worst)


def test_cell_cases_admitted():
    _admit(C.cell_cases(), C.cell_eval)


def test_cross_entropy_cases_admitted():
    _admit(C.ce_cases(), C.ce_reference)


def test_adam_cases_admitted():
    _admit(C.adam_cases(), C.adam_eval)


def test_dense_cases_admitted():
    _admit(C.dense_cases(), C.dense_eval)


# ---------------------------------------------------------------------------------------------------------------------
# the builders reach their edges
# ---------------------------------------------------------------------------------------------------------------------
def test_cell_rows_hold_every_class():
    rows = C.cell_rows()
    assert {(a, b) for a, b in zip(rows['row_class'], rows['cx_class'])} == {(a, b) for a in C.ROW_CLASSES for b in C.CX_CLASSES}
    for r, (a, b) in enumerate(zip(rows['row_class'], rows['cx_class'])):
        assert bool((rows['inp'][r] == 0).all()) == (a in ('aggregate 0', 'both 0'))
        assert bool((rows['hid'][r] == 0).all()) == (a in ('hidden 0', 'both 0'))
        assert bool((rows['cx'][r] == 0).all()) == (b == '0') and bool((rows['cx'][r].abs() == 20).all()) == (b == '+-20')
    # the small cases are not all plain rows
    assert set(rows['row_class'][:5]) - {'unit'} and {c['n'] for c in C.cell_cases()} == set(C.CELL_SIZES)
    combos = {(c['kind'], c['layernorm'], c['ingate'], c['grad_cy']) for c in C.cell_cases()}
    assert len(combos) == 4 + 8
    # row variance around and below eps on the 1e-3 rows (with row normalisation), saturated gates on the saturating rows (without)
    P = {'c.' + k: v.double() for k, v in C.cell_params('gru', True, False).items()}
    r3 = [i for i, a in enumerate(rows['row_class']) if a == '1e-3']
    var = (rows['inp'][r3].double() @ P['c.weight_ih'].t()).var(1, unbiased=False)
    assert float(var.max()) < 10 * O.IN_EPS and float(var.min()) < O.IN_EPS
    P = {'c.' + k: v.double() for k, v in C.cell_params('lstm', False, False).items()}
    rs = [i for i, a in enumerate(rows['row_class']) if a == 'saturating']
    pre = rows['inp'][rs].double() @ P['c.weight_ih'].t() + rows['hid'][rs].double() @ P['c.weight_hh'].t()
    assert float((pre.abs() > 16.7).double().mean()) > 0.03            # sigmoid rounds to 0 / 1 in float32 (1 - 2^-24)
    # a closed and an open input gate
    P = C.cell_params('gru', True, True)
    gate = torch.sigmoid(rows['hid'][[i for i, a in enumerate(rows['row_class']) if a == 'unit']].double() @ P['ig.weight'].double().t() + P['ig.bias'].double())
    assert float(gate[:, list(C.IG_CLOSED)].max()) < 1e-6 and float(gate[:, list(C.IG_OPEN)].min()) > 1 - 1e-6


def test_cell_restatement_is_the_oracle():
    for c in C.cell_cases():
        if c['n'] != 64:
            continue
        a, b = C.cell_eval(c), C.cell_eval(c, eps=O.IN_EPS)          # a knob at its default value selects the restatement
        for k in a:
            assert torch.equal(a[k], b[k]), (c['name'], k)


def test_cross_entropy_cases_reach_their_edges():
    cases = C.ce_cases()
    assert {(c['N'], c['C']) for c in cases} == set(C.CE_SHAPES)
    assert {c['upstream'] for c in cases} == set(C.CE_UPSTREAM) and {c['reduction'] for c in cases} == {'mean', 'sum'}
    for N, C_ in C.CE_SHAPES:
        assert {c['upstream'] for c in cases if (c['N'], c['C']) == (N, C_)} == set(C.CE_UPSTREAM)
    seen_inf = seen_zero_weight = 0
    for c in cases:
        x, t, valid = c['logits'], c['target'], C._ce_valid(c)
        inf = torch.isinf(x)
        seen_inf += int(inf.any())
        assert not bool(inf[valid, t[valid]].any()), 'the target entry itself is never -inf'
        ref = C.ce_reference(c)
        if 'all ignored' in c['name']:
            assert not bool(valid.any()) and float(ref['grad'].abs().max()) == 0.0
            assert math.isnan(float(ref['loss'])) if c['reduction'] == 'mean' else float(ref['loss']) == 0.0
        elif 'one labelled' in c['name']:
            assert int(valid.sum()) == 1 and float(ref['normaliser']) > 0
        elif c['bad']:
            bad = (t != C.IGNORE) & ~valid
            assert int(bad.sum()) == 2 and set(t[bad].tolist()) in ({c['C']}, {-1})
            assert math.isnan(float(ref['loss'])) and float(ref['grad'][bad].abs().max()) == 0.0 and float(ref['grad'][valid].abs().max()) > 0
        else:
            assert math.isfinite(float(ref['loss'])) and float(ref['normaliser']) > 0
        if 'zero class' in c['name'] and 'all ignored' not in c['name']:
            z = c['C'] - 1
            assert float(c['weight'][z]) == 0.0 and float(ref['normaliser']) > 0
            if '10% ignored' in c['name']:
                seen_zero_weight += 1
                assert bool((t == z).any()) and bool((valid & (t != z)).any())
                assert float(ref['grad'][t == z].abs().max()) == 0.0
    assert sorted(int(c['target'][65 // 3]) for c in cases if c['bad']) == [-1, 13]
    assert seen_inf > len(cases) // 2 and seen_zero_weight >= 2 * (len(C.CE_SHAPES) - 2)
    # the large offsets are there: a log-sum-exp of magnitude 1e4 and 3e4 whose row spread is a few units / a few hundred
    big = [c for c in cases if c['N'] >= 63][0]['logits']
    assert float(big[torch.isfinite(big)].max()) > 9e3 and float(big[torch.isfinite(big)].min()) < -2.9e4


def test_adam_cases_reach_their_edges():
    cases = C.adam_cases()
    assert {c['n'] for c in cases} == set(C.ADAM_SIZES) and {c['step'] for c in cases} == set(C.ADAM_STEPS)
    assert {(c['wd'], c['clip'], None if c['div'] is None else round(float(c['div']), 6)) for c in cases} == set(C.ADAM_HYPER)
    for c in cases:
        g, p = c['g'], c['p']
        assert bool((p[1::2] == 0).all()) and (c['n'] == 1 or bool((p[0::2] != 0).all()))
        mag = g[g != 0].abs()
        assert float(mag.min()) >= 1e-15 and float(mag.max()) <= 1e2 + 1 and bool((g.double() ** 2).float()[g != 0].min() >= torch.finfo(F32).tiny)
        if c['n'] >= 255:
            clip, div = c['clip'] or 0.5, 1.0 if c['div'] is None else float(c['div'])
            assert bool((g == 0).any()) and bool((g == clip).any()) and bool((g == -clip).any()) and bool((g.abs() > clip * div).any())
            assert float(mag.min()) < 1e-12
        assert bool((c['v'] >= 0).all()) and ((c['step'] == 1) == (not bool(c['m'].any())))
        ref = C.adam_eval(c)
        if c['clip'] > 0:
            assert float(ref['g'].abs().max()) <= c['clip']
        if c['step'] == 1 and c['wd'] == 0 and c['n'] >= 255:          # zero gradient, zero moments: denominator = eps, update exactly 0
            zero = (c['g'] == 0)[1::2]
            assert bool(zero.any()) and float(ref['p (p was 0)'][zero].abs().max()) == 0.0


def test_adam_restatement_is_torch_optim_adam():
    """The float64 restatement against torch.optim.Adam itself (float64 parameters, the reference loop's clamp)."""
    for c in C.adam_cases():
        if c['n'] != 257:
            continue
        p = torch.nn.Parameter(c['p'].double().clone())
        opt = torch.optim.Adam([p], lr=C.ADAM_LR, betas=C.ADAM_BETAS, eps=C.ADAM_EPS, weight_decay=c['wd'])
        p.grad = c['g'].double().clone()
        if c['div'] is not None:
            p.grad /= c['div'].double()
        if c['clip'] > 0:
            p.grad.clamp_(-c['clip'], c['clip'])
        opt.state[p] = {'step': torch.tensor(float(c['step'] - 1)), 'exp_avg': c['m'].double().clone(), 'exp_avg_sq': c['v'].double().clone()}
        opt.step()
        st = opt.state[p]
        got = C.split_adam(p.detach(), p.grad, st['exp_avg'], st['exp_avg_sq'])
        for k, (_, r) in C.measure(C.adam_eval(c), got).items():
            assert r < 1e-6, (c['name'], k, r)            # 1e-10 relative: float64 round-off


def test_dense_cases_reach_the_column_sum_paths():
    for c in C.dense_cases():
        M = c['M']
        rps = max(16, -(-M // 64))                       # spg_colsum: 64 slices of at least 16 rows
        slices = -(-M // rps)
        assert {1: (16, 1), 15: (16, 1), 16: (16, 1), 17: (16, 2), 1024: (16, 64), 1025: (17, 61), 129: (16, 9), 300: (16, 19)}[M] == (rps, slices)


# ---------------------------------------------------------------------------------------------------------------------
# altered references leave the bound
# ---------------------------------------------------------------------------------------------------------------------
def _caught(cases, evaluate, reference, knobs):
    """(largest ratio of the float32 evaluation with `knobs` over the cases, the case and tensor where it occurs)."""
    top = (0.0, '', '')
    for c in cases:
        for k, (_, r) in C.measure(evaluate(c, F32, **knobs), _reference(reference, c)).items():
            if r > top[0]:
                top = (r, c['name'], k)
    return top


CELL_ALTERATIONS = {
    'row-norm eps 1e-6': ('both', dict(eps=1e-6)),
    'row-norm eps 0': ('both', dict(eps=0.0)),
    'unbiased variance': ('both', dict(unbiased=True)),
    'GRU biases before the normalisation': ('gru', dict(bias_before_norm=True)),
    'LSTM biases after the normalisation': ('lstm', dict(bias_after_norm=True)),
    'hidden - newgate sign flipped': ('gru', dict(flip_sign=True)),
}


@pytest.mark.parametrize('name', list(CELL_ALTERATIONS))
def test_cell_alteration_is_caught(name):
    kinds, knobs = CELL_ALTERATIONS[name]
    for kind in (('gru', 'lstm') if kinds == 'both' else (kinds,)):
        cases = [c for c in C.cell_cases() if c['kind'] == kind and c['n'] == 64]
        r, where, tensor = _caught(cases, C.cell_eval, C.cell_eval, knobs)
        print(name, kind, f'{r:.3g}', where, tensor)
        assert r > 1.0, f'{name} ({kind}) stays inside the bound on every case: worst {r:.3f}'
        # ... and on EVERY output tensor of some case with row normalisation, not only on a gradient
        if 'eps' in knobs or 'unbiased' in knobs:
            c = [c for c in cases if c['layernorm']][0]
            assert C.bound_ratio(C.cell_eval(c, F32, **knobs)['hy'], C.cell_eval(c)['hy'])[1] > 1.0


CE_ALTERATIONS = {
    'log-sum-exp without max subtraction': dict(max_subtraction=False),
    'mean normalised by the row count': dict(normaliser='rows'),
    'log-sum-exp rounded to float32 before it is subtracted': dict(lse_first=True),
}


def test_cross_entropy_restatement_inside_the_bound():
    r, where, tensor = _caught(C.ce_cases(), C.ce_restatement, C.ce_reference, {})
    assert r <= C.ADMIT, (r, where, tensor)
    for c in C.ce_cases()[::7]:
        assert C.worst(C.measure(C.ce_restatement(c, torch.float64), C.ce_reference(c))) < 1e-6


@pytest.mark.parametrize('name', list(CE_ALTERATIONS))
def test_cross_entropy_alteration_is_caught(name):
    r, where, tensor = _caught(C.ce_cases(), C.ce_restatement, C.ce_reference, CE_ALTERATIONS[name])
    print(name, f'{r:.3g}', where, tensor)
    assert r > 1.0, f'{name} stays inside the bound on every case: worst {r:.3f}'


ADAM_ALTERATIONS = {
    'weight decay added before the clamp': dict(wd_before_clamp=True),
    'grad_div applied after the clamp': dict(div_after_clamp=True),
    'eps inside the square root': dict(eps_inside_sqrt=True),
    'missing bias correction': dict(bias_correction=False),
}


@pytest.mark.parametrize('name', list(ADAM_ALTERATIONS))
def test_adam_alteration_is_caught(name):
    r, where, tensor = _caught(C.adam_cases(), C.adam_eval, C.adam_eval, ADAM_ALTERATIONS[name])
    print(name, f'{r:.3g}', where, tensor)
    assert r > 1.0, f'{name} stays inside the bound on every case: worst {r:.3f}'


def test_column_sum_alteration_is_caught():
    for c in C.dense_cases():
        got, ref = C.dense_eval(c, F32, drop_partial_group=True), C.dense_eval(c)
        r = C.bound_ratio(got['dbias'], ref['dbias'])[1]
        assert (r > 1.0) == (c['M'] % 16 != 0), (c['name'], r)        # caught at every M with a partial group: 1, 15, 17, 1025, 129, 300
