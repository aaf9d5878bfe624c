"""CPU: the cases of tests/wide_cell_cases.py are what they claim to be -- every row class and (row class, cx class) pair is present,
every case is admitted (its float32 CPU evaluation stays within ADMIT of the bound on every compared tensor), the restatements with
every knob off are the oracle, and every knob leaves the bound on at least one case.

`python tests/test_wide_cell_cases.py` prints the admission figures (the CPU column of profiles/wide_cell_errors.txt)."""
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import ecc_cases as EC
import wide_cell_cases as C


def test_cell_cases_cover_the_classes_and_sizes():
    cases = C.cell_cases()
    assert len(cases) == 2 * 4 * 4 * 4
    for nc in C.WIDTHS:
        nb = C.BLOCK_NODES[nc]
        sizes = C.cell_sizes(nc)
        assert sizes[:3] == (1, nb - 1, nb + 1) and sizes[3] > 3 * nb and sizes[3] % nb != 0
        rows = C.cell_rows(nc)
        pairs = set(zip(rows['row_class'][:sizes[3]], rows['cx_class'][:sizes[3]]))
        assert len(pairs) == len(C.ROW_CLASSES) * len(C.CX_CLASSES)
        for r, c in enumerate(rows['row_class']):
            a0, h0 = float(rows['inp'][r].abs().max()) == 0.0, float(rows['hid'][r].abs().max()) == 0.0
            assert a0 == (c in ('aggregate 0', 'both 0')) and h0 == (c in ('hidden 0', 'both 0'))
        P = C.cell_params('lstm', nc, True, True)
        assert P['weight_ih'].shape == (4 * nc, nc) and P['ig.weight'].shape == (nc, nc)
        assert C.cell_params('gru', nc, True, False)['weight_hh'].shape == (3 * nc, nc)
    assert any(c['grad_cy'] is False for c in cases) and any(c['grad_cy'] for c in cases)


_cell_figures = {}


def cell_admission(case):
    if case['name'] not in _cell_figures:
        _cell_figures[case['name']] = C.measure(C.cell_eval(case, torch.float32), C.cell_eval(case, torch.float64))
    return _cell_figures[case['name']]


@pytest.mark.parametrize('nc', C.WIDTHS)
def test_cell_cases_are_admitted(nc):
    for case in C.cell_cases():
        if case['nc'] != nc:
            continue
        fig = cell_admission(case)
        assert C.worst(fig) <= C.ADMIT, (case['name'], {k: v for k, v in fig.items() if v[1] > C.ADMIT})
        ref = C.cell_eval(case, torch.float64)
        assert set(ref) == {'hy', 'd_input', 'd_hidden'} | ({'cy', 'd_cx'} if case['kind'] == 'lstm' else set()) | {'d_' + k for k in case['params']}


def test_cell_restatement_with_every_knob_off_is_the_oracle():
    for case in C.cell_cases():
        if case['n'] != C.cell_sizes(case['nc'])[3]:
            continue
        ref = C.cell_eval(case, torch.float64)
        got = C.cell_eval(case, torch.float64, unbiased=False)         # a knob at its default: the restatement is evaluated
        for k in ref:
            assert torch.equal(got[k], ref[k]), (case['name'], k)


@pytest.mark.parametrize('knob', list(C.CELL_KNOBS))
def test_every_cell_knob_leaves_the_bound(knob):
    seen = []
    for case in C.cell_cases():
        if case['n'] != C.cell_sizes(case['nc'])[3]:
            continue
        ref = C.cell_eval(case, torch.float64)
        seen.append(C.worst(C.measure(C.cell_eval(case, torch.float64, **C.CELL_KNOBS[knob]), ref)))
    assert max(seen) > 1.0, (knob, max(seen))


def _module_admission(args):
    case = C.module_case(*args) if len(args) == 8 else C.network_case(*args)
    rec32 = {}
    cpu = C.module_eval(case, torch.float32, rec=rec32)
    refs, n_diff = C.module_refs(case, EC.decisions(rec32))
    return case, {k: C.bound_ratio(cpu[k], r) for k, r in refs.items()}, n_diff


@pytest.mark.parametrize('args', C.MODULE_CASES + (C.NETWORK_CASE,), ids=lambda a: '-'.join(str(v) for v in a))
def test_module_cases_are_admitted(args):
    case, fig, _ = _module_admission(args)
    assert C.worst(fig) <= C.ADMIT, (case['name'], {k: v for k, v in fig.items() if v[1] > C.ADMIT})
    if case['training']:
        assert 'grad x' in fig and any(k.startswith('grad ecc.0._cell.weight_ih') for k in fig) and any('_fnet.0.weight' in k for k in fig)


def test_module_cases_cover_the_configurations():
    cells, widths = {a[0] for a in C.MODULE_CASES}, {(a[1], a[2]) for a in C.MODULE_CASES}
    assert cells == {'gru', 'lstm'} and widths == {(8, True), (64, True), (16, False), (128, False)}
    assert {a[3] for a in C.MODULE_CASES} == {1, 3} and {a[4] for a in C.MODULE_CASES} == {True, False}
    assert {a[7] for a in C.MODULE_CASES} == {True, False}
    for kind in cells:
        assert {(a[1], a[2]) for a in C.MODULE_CASES if a[0] == kind and a[7]} == widths, kind
    _, degs, _ = EC.graph(C.GKEY)
    assert int(degs.max()) == 100 and int((degs == 0).sum()) > 0


def test_module_restatement_and_its_knob():
    """The restated aggregation with the knob off stays within 1e-6 of the bound of the oracle (another summation order in float64);
    `mean divided by the out-degree` leaves the bound."""
    for args in (C.MODULE_CASES[0], C.MODULE_CASES[4]):
        case = C.module_case(*args)
        ref, _ = C.module_reference(case['config'], case['nc'], True)
        keys = C.compared(ref)
        plain = C.module_eval(case, torch.float64, restated=True)
        assert max(C.bound_ratio(plain[k], ref[k])[1] for k in keys) < 1e-6
        for knob, kw in C.MODULE_KNOBS.items():
            wrong = C.module_eval(case, torch.float64, **kw)
            assert max(C.bound_ratio(wrong[k], ref[k])[1] for k in keys) > 1.0, knob


def report():
    lines = ['# python tests/test_wide_cell_cases.py: worst |float32 CPU - float64| / bound per case family (admission: <= %.2f)' % C.ADMIT]
    fam = {}
    for case in C.cell_cases():
        key = f"cell {case['kind']} nc{case['nc']}"
        fam[key] = max(fam.get(key, 0.0), C.worst(cell_admission(case)))
    for args in C.MODULE_CASES + (C.NETWORK_CASE,):
        case, fig, _ = _module_admission(args)
        fam['module ' + case['name']] = C.worst(fig)
    return '\n'.join(lines + [f'{k:70s} {v:8.3f}' for k, v in fam.items()])


if __name__ == '__main__':
    print(report())
