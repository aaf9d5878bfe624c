"""GPU: the stand-alone cell's scratch -- spg_cell_scratch_floats and the carving of spg_cell_bwd are one layout (csrc/spg_api.hip:
cell_scratch).  Both cells x the widths 8, 16, 32, 64, 128 x the row counts 1, one less and one more than the rows of a workgroup
(spg_cell_block_nodes), layernorm and input gate on, the LSTM once with grad_cy and once without; one more GRU case at 128 with
16384 rows, inside the first window of row counts (16321 .. 16384; the next are 32641 .. 32768, 48961 .. 49152, ...; GRU at 128
only) in which the input gate's [nc, nc] weight gradient splits into partials that need MORE room than those of the [3 nc, nc]
gradients: 512 x 128 x 128 = 8 388 608 floats against 128 x 384 x 128 = 6 291 456 (wgrad_plan, csrc/spg_gemm.hip).

Run A hands spg_cell_bwd a scratch of exactly spg_cell_scratch_floats floats INSIDE a larger tensor, 4096 guard floats in front and
behind, everything pre-filled with one bit pattern: both guards keep it bit for bit.  Run B, with twice the scratch, returns every
output and every parameter gradient bit for bit (nothing depends on the scratch size or on what the scratch held: the pattern is a
NaN).  The two older size functions answer what spg_cell_scratch_floats answers at 32, and every forward entry accepts scratch =
NULL with the result it gives with one."""
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WIDTHS = (8, 16, 32, 64, 128)
KINDS = {'gru': 0, 'lstm': 1}
GUARD = 4096
PATTERN = 0x7FA5C3E1      # a NaN as float32


def rows_of(L, nc):
    b = L.spg_cell_block_nodes(nc)
    return sorted({n for n in (1, b - 1, b + 1) if n > 0})


_inputs = {}


def inputs(kind, nc, n):
    """-> dict of device tensors (built once per case, never written)."""
    key = (kind, nc, n)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * nc + n)
        G = (4 if kind == 'lstm' else 3) * nc
        r = lambda *s: torch.randn(*s, generator=g)
        t = {'inp': r(n, nc), 'h': r(n, nc), 'c': r(n, nc), 'ghy': r(n, nc), 'gcy': r(n, nc),
             'params': [r(G, nc) / nc ** 0.5, r(G, nc) / nc ** 0.5, 0.1 * r(G), 0.1 * r(G), r(nc, nc) / nc ** 0.5, 0.1 * r(nc)]}
        _inputs[key] = {k: [p.to(DEV) for p in v] if k == 'params' else v.to(DEV) for k, v in t.items()}
    return _inputs[key]


def bits(t):
    return t.contiguous().view(torch.int32)


def run_bwd(L, kind, nc, n, grad_cy, scale, guard=GUARD):
    """spg_cell_bwd with scale * spg_cell_scratch_floats floats of scratch -> (outputs, guard in front, guard behind)."""
    from superpoint_graph_amd._lib import check
    from superpoint_graph_amd.ops._core import _ptr, _ptr_array, _stream
    t = inputs(kind, nc, n)
    lstm = kind == 'lstm'
    floats = L.spg_cell_scratch_floats(KINDS[kind], nc, n)
    assert floats > 0
    big = torch.full((2 * guard + scale * floats,), PATTERN, dtype=torch.int32, device=DEV)
    gi, gh = torch.zeros_like(t['inp']), torch.zeros_like(t['h'])
    gc = torch.zeros_like(t['c']) if lstm else None
    grads = [torch.zeros_like(p) for p in t['params']]
    check(L.spg_cell_bwd(KINDS[kind], nc, _ptr(t['inp']), _ptr(t['h']), _ptr(t['c']) if lstm else None, _ptr(t['ghy']),
                         _ptr(t['gcy']) if (lstm and grad_cy) else None, n, _ptr_array(t['params']), 1, 1, _ptr(gi), _ptr(gh), _ptr(gc),
                         _ptr_array(grads), big.data_ptr() + 4 * guard, _stream()), 'spg_cell_bwd')
    torch.cuda.synchronize()
    outs = [gi, gh] + ([gc] if lstm else []) + grads
    return outs, big[:guard], big[guard + scale * floats:]


def check_guarded(L, kind, nc, n, grad_cy, guard=GUARD):
    a, front, behind = run_bwd(L, kind, nc, n, grad_cy, 1, guard)
    assert front.numel() == behind.numel() == guard
    assert bool((front == PATTERN).all()), f'{kind} nc{nc} n{n}: spg_cell_bwd wrote in front of its scratch'
    assert bool((behind == PATTERN).all()), f'{kind} nc{nc} n{n}: spg_cell_bwd wrote behind spg_cell_scratch_floats floats'
    b, _, _ = run_bwd(L, kind, nc, n, grad_cy, 2)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(x).all()), f'{kind} nc{nc} n{n}: output {i} is not finite'
        assert torch.equal(bits(x), bits(y)), f'{kind} nc{nc} n{n}: output {i} depends on the scratch size'


@pytest.mark.parametrize('nc', WIDTHS)
@pytest.mark.parametrize('kind,grad_cy', [('gru', False), ('lstm', True), ('lstm', False)])
def test_backward_stays_inside_its_scratch(hip, kind, grad_cy, nc):
    for n in rows_of(hip, nc):
        check_guarded(hip, kind, nc, n, grad_cy)


def test_backward_scratch_where_the_input_gate_splits_finer(hip):
    # (a layout sized by the [3 nc, nc] plan alone is 2 097 152 floats short here: the guards, 2^22 floats each, are wider than that)
    check_guarded(hip, 'gru', 128, 16384, False, guard=1 << 22)


def test_older_size_functions_are_the_layout_at_32(hip):
    for n in rows_of(hip, 32) + [50, 1000]:
        assert hip.spg_gru_scratch_floats(n) == hip.spg_cell_scratch_floats(KINDS['gru'], 32, n) > 0
        assert hip.spg_lstm_scratch_floats(n) == hip.spg_cell_scratch_floats(KINDS['lstm'], 32, n) > 0


@pytest.mark.parametrize('nc', WIDTHS)
def test_forward_takes_no_scratch(hip, nc):
    from superpoint_graph_amd.ops._core import _ptr, _ptr_array, _stream
    L = hip
    n = L.spg_cell_block_nodes(nc) + 1
    for kind in KINDS:
        t = inputs(kind, nc, n)
        lstm = kind == 'lstm'
        some = torch.empty(L.spg_cell_scratch_floats(KINDS[kind], nc, n), dtype=torch.float32, device=DEV)

        def fwd(entry, scratch):
            hy = torch.zeros_like(t['h'])
            cy = torch.zeros_like(t['h']) if lstm else None
            head = (_ptr(t['inp']), _ptr(t['h'])) + ((_ptr(t['c']),) if lstm or entry == 'spg_cell_fwd' else ())
            tail = (n, _ptr_array(t['params']), 1, 1, _ptr(hy)) + ((_ptr(cy),) if lstm or entry == 'spg_cell_fwd' else ())
            pre = (KINDS[kind], nc) if entry == 'spg_cell_fwd' else ()
            assert getattr(L, entry)(*pre, *head, *tail, _ptr(scratch), _stream()) == 0, L.spg_last_error()
            torch.cuda.synchronize()
            return [hy] + ([cy] if lstm else [])
        for entry in ['spg_cell_fwd'] + ([f'spg_{kind}_cell_fwd'] if nc == 32 else []):
            for x, y in zip(fwd(entry, None), fwd(entry, some)):
                assert bool(torch.isfinite(x).all()) and torch.equal(bits(x), bits(y)), f'{entry} {kind} nc{nc}'
