"""GPU: GRUCellEx / LSTMCellEx at the state widths 8, 16, 64 and 128 (csrc/spg_ecc_wide.hip through spg_cell_fwd / spg_cell_bwd),
element by element against the float64 references of tests/wide_cell_cases.py (whose cases and knobs tests/test_wide_cell_cases.py
checks on the CPU): both cells x the four widths x the four (layernorm, ingate) combinations x the row counts 1, one less and one
more than the rows of a workgroup, a few workgroups (wide_cell_cases.cell_sizes: (1, 15, 17, 50) at 8 and 16, (1, 7, 9, 26) at 64,
(1, 3, 5, 22) at 128); row classes unit, 1e-3, saturating, aggregate 0, hidden 0, both 0 and for the LSTM the cx classes 0, unit,
+-20.  Compared under conftest.assert_elementwise: the outputs and every gradient (input, hidden, cell state, all parameters).  A
second run is bit-identical (no atomics).

`python tests/test_gpu_wide_cell.py` prints the measured figures (profiles/wide_cell_errors.txt)."""
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import wide_cell_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def run_cell(case):
    """-> {hy, (cy), d_input, d_hidden, (d_cx), d_<parameter>} on the host, through the modules' public forward / backward."""
    from superpoint_graph_amd.learning.modules import GRUCellEx, LSTMCellEx
    nc = case['nc']
    cell = (GRUCellEx if case['kind'] == 'gru' else LSTMCellEx)(nc, nc, bias=True, layernorm=case['layernorm'], ingate=case['ingate'])
    cell.load_state_dict(case['params'])
    cell = cell.to(DEV)
    inp, hid, cx = [case[k].to(DEV).requires_grad_(True) for k in ('inp', 'hid', 'cx')]
    if case['kind'] == 'gru':
        hy = cell(inp, hid)
        hy.backward(case['gh'].to(DEV))
        res = {'hy': hy, 'd_input': inp.grad, 'd_hidden': hid.grad}
    else:
        hy, cy = cell(inp, (hid, cx))
        if case['grad_cy']:
            torch.autograd.backward([hy, cy], [case['gh'].to(DEV), case['gc'].to(DEV)])
        else:
            hy.backward(case['gh'].to(DEV))
        res = {'hy': hy, 'cy': cy, 'd_input': inp.grad, 'd_hidden': hid.grad, 'd_cx': cx.grad}
    for k, p in cell.named_parameters():
        res['d_' + k] = p.grad
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def test_rows_per_workgroup_are_the_stated_ones(hip):
    from superpoint_graph_amd import ops
    for nc in C.WIDTHS:
        assert ops.model.cell_block_nodes(nc) == C.BLOCK_NODES[nc]


@pytest.mark.parametrize('case', C.cell_cases(), ids=lambda c: c['name'].replace(' ', '-'))
def test_cell_against_float64(hip, case):
    ref = C.cell_eval(case, torch.float64)
    got = run_cell(case)
    assert set(got) == set(ref)
    for k, (err, ratio) in C.measure(got, ref).items():
        print(f"{case['name']}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound")
    for k in ref:
        C.assert_bound(got[k], ref[k], f"{case['name']}: {k}")
    again = run_cell(case)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{case['name']}: {k} differs between two runs"


def report():
    from superpoint_graph_amd import _lib
    _lib.lib()
    lines = ['# python tests/test_gpu_wide_cell.py: worst error / bound (1e-4 |ref| + 1e-5 max|ref| per element, float64 reference) per case',
             '# family, over all its cases and compared tensors: the device, and the float32 CPU evaluation of the same reference',
             f"{'family':24s} {'device':>8s} {'cpu f32':>8s}  worst device tensor"]
    fam = {}
    for case in C.cell_cases():
        ref = C.cell_eval(case, torch.float64)
        dev_f, cpu_f = C.measure(run_cell(case), ref), C.measure(C.cell_eval(case, torch.float32), ref)
        key = f"cell {case['kind']} nc{case['nc']}"
        k = max(dev_f, key=lambda t: dev_f[t][1])
        old = fam.get(key, (0.0, 0.0, ''))
        fam[key] = (max(old[0], dev_f[k][1]), max(old[1], C.worst(cpu_f)), f"{case['name']}: {k}" if dev_f[k][1] >= old[0] else old[2])
    return '\n'.join(lines + [f'{k:24s} {d:8.3f} {c:8.3f}  {w}' for k, (d, c, w) in fam.items()])


if __name__ == '__main__':
    print(report())
