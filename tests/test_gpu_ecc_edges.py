"""GPU: the edge-conditioned graph convolution at its degree thresholds, element by element against the float64 references of
tests/ecc_cases.py (whose graphs, cases and knobs tests/test_ecc_cases.py checks on the CPU):

a. GRAPH BUILD: ops.DeviceGraph(...).export() and the single-launch builder (ops.batch_graph_build, fed the edges in a shuffled
   order) on every ladder / tiny graph against oracle.csr_by_target / edge_targets / csr_by_source, bit for bit; every source's
   rev_eid list ascending; the error word of hdr 0.
b. THE OPERATOR ALONE (ecc.GraphConvFunction.apply): float32 32 -> 32 matrix and vector filters (the fused wave-per-node /
   wave-per-source / wave-per-edge kernels), float32 and float64 10 -> 15, one float64 run with filter sharing (idxe, atomics); x
   scaled by 1, 1e-3, 1e3.  out / grad_x per element with the floor per ROW, grad_w with the floor per EDGE; float64 at 1e-13 of the
   row's maximum.  Degree-0 rows of out and grad_x rows of nodes without out-edges are exact zeros; a second call is bit-identical
   (except grad_w under filter sharing: atomics).
c. THE RECURRENT MODULE (graphnet.GraphNetwork) in training mode against oracle.graph_network_forward in float64.  The
   configurations END at the recurrent token with cat_all = 1 ('gru_10_0', 'gru_4_1', 'gru_3_0_0_0_1', 'lstm_3_0'; the module accepts
   them), so the output is every iteration's state [n, 32 (R + 1)] and an error of iteration 1 is seen before the cell contracts it.
   Launch forms (FORMS below): per-iteration launches (spg_tune key 8 = 1, and the LSTM always) at n = 200; persistent with one
   workgroup per CU at n = 3, 5, 200 and 1008 (the largest graph the residency bound admits on 256 CUs: 252 full workgroups); n = 1024
   lies in the band 1009 .. 1024 that falls back to the per-iteration launches on this part (256 workgroups > 256 - 4; two per CU start
   at 1025 nodes) and is listed as that; two per CU at n = 1025; the iteration-major kernels at n = 2049 (one node per wavefront in the
   forward, at most two in the backward at this size; more nodes per wavefront: tests/test_gpu_ecc_persistent.py at 5000 and 10000
   nodes); three scenes with `parts` (two rounds, two workgroups per CU, the ladder in the second).  The library has no query for the
   kernel that ran.  launch_form() restates, for the case and the device (the cell, key 8, the CUs from
   torch.cuda.get_device_properties), the plan of csrc/spg_px_plan.h -- spg_px_plan_groups and spg_px_plan, the one place that
   decides the form, swept on the host by tests/px_plan_host_test.cpp -- and every test asserts that it gives the form the case is
   listed under.  The launchers' other reasons to decline cannot be observed from outside: more than 15 iterations (none here),
   an iteration-major kernel that gets fewer workgroups per CU than it was written for, another stream still busy with a persistent
   launch (the tests use one stream), a failed allocation of the 64 MiB exchange buffer.  The tests further assert that key 8 held the intended value during the run and that
   spg_ecc_persistent_status reports no time-out and no withheld update.  Compared per element under conftest.assert_elementwise: out
   (against the reference with its own decisions), the input gradient and every parameter gradient that conftest.noise_grad does not
   exclude (against the float64 backward run with the DEVICE's filter-network ReLU decisions, which may differ from the reference's own
   only on near-ties: test_gpu_baseline_parity._hip_fnet_decisions, ecc_cases.check_near_ties).  The excluded bias gradient stays
   below 1e-5; a second run is bit-identical; evaluation mode runs forward only.

`python tests/test_gpu_ecc_edges.py` prints the measured figures (profiles/ecc_edges_errors.txt)."""
import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import ecc_cases as C
from oracle import spg_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ---------------------------------------------------------------------------------------------------------------------
# a. graph build
# ---------------------------------------------------------------------------------------------------------------------
def _check_export(graph, idxn, degs):
    n, E = int(degs.numel()), int(idxn.numel())
    rowptr, src, dst, rev_rowptr, rev = [t.cpu().numpy() for t in graph.export()]
    rrp, order = O.csr_by_source(idxn.numpy(), n)
    assert np.array_equal(rowptr, O.csr_by_target(degs.numpy()).astype(np.int32))
    assert np.array_equal(src, idxn.numpy().astype(np.int32))
    assert np.array_equal(dst, O.edge_targets(degs.numpy()).astype(np.int32))
    assert np.array_equal(rev_rowptr, rrp.astype(np.int32))
    assert np.array_equal(rev, order.astype(np.int32))
    inner = np.ones(E, dtype=bool)
    inner[rrp[:-1][rrp[:-1] < E]] = False                       # first entry of every source's list
    assert bool((np.diff(rev.astype(np.int64), prepend=-1)[inner] > 0).all()), 'a rev_eid list is not ascending'
    assert int(graph.hdr.cpu()[3]) == 0


@pytest.mark.parametrize('gkey', C.GRAPH_KEYS)
def test_graph_build_at_the_ladder(hip, gkey):
    from superpoint_graph_amd import ops
    idxn, degs, _ = C.graph(gkey)
    n, E = int(degs.numel()), int(idxn.numel())
    _check_export(ops.DeviceGraph(idxn.to(DEV), degs.to(DEV)), idxn, degs)
    # the single-launch builder, from the edge list in a shuffled order: stable by target
    rng = np.random.default_rng(E)
    edges = np.stack([idxn.numpy(), O.edge_targets(degs.numpy())], 1)[rng.permutation(E)]
    feats = torch.from_numpy(rng.standard_normal((E, 3)).astype(np.float32))
    built = ops.batch_graph_build(torch.from_numpy(edges), feats, n)
    assert built is not None
    idxn2, degs2, feats2, graph2, err = built
    order = np.argsort(edges[:, 1], kind='stable')
    assert int(err) == 0 and torch.equal(degs2.cpu(), degs)
    assert np.array_equal(idxn2.cpu().numpy(), edges[order, 0]) and torch.equal(feats2.cpu(), feats[torch.from_numpy(order)])
    _check_export(graph2, idxn2.cpu(), degs)


# ---------------------------------------------------------------------------------------------------------------------
# b. the operator alone
# ---------------------------------------------------------------------------------------------------------------------
_graphs = {}


def device_graph(gkey):
    from superpoint_graph_amd import ops
    if gkey not in _graphs:
        idxn, degs, _ = C.graph(gkey)
        idxn_d = idxn.to(DEV)
        _graphs[gkey] = (idxn_d, ops.DeviceGraph(idxn_d, degs.to(DEV)))
    return _graphs[gkey]


def run_op(case, dtype):
    from superpoint_graph_amd.learning import ecc
    idxn_d, graph = device_graph(case['gkey'])
    _, degs, _ = C.graph(case['gkey'])
    x, w = [case[k].to(dtype).to(DEV).requires_grad_(True) for k in ('x', 'w')]
    idxe = None if case['idxe'] is None else case['idxe'].to(DEV)
    cin, cout = x.shape[1], w.shape[-1]
    out = ecc.GraphConvFunction.apply(x, w, cin, cout, idxn_d, idxe, degs, graph)
    out.backward(case['go'].to(dtype).to(DEV))
    return {'out': out.detach().cpu(), 'grad_x': x.grad.cpu(), 'grad_w': w.grad.cpu()}


_op_refs = {}


def op_reference(args):
    if args not in _op_refs:
        _op_refs[args] = C.op_eval(C.op_case(*args), torch.float64)
    return _op_refs[args]


def judge_op(args, dtype):
    case, ref = C.op_case(*args), op_reference(args)
    got = run_op(case, dtype)
    kw = {} if dtype == torch.float32 else dict(rtol=0.0, atol_frac=C.F64_TOL)
    for k, (err, ratio) in C.measure_rows(got, ref, **kw).items():
        print(f"{case['name']} {str(dtype)[6:]}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound")
    for k in ref:
        C.assert_row_bound(got[k], ref[k], f"{case['name']} {str(dtype)[6:]}: {k}", **kw)
    idxn, degs, _ = C.graph(case['gkey'])
    sink = torch.from_numpy(np.bincount(idxn.numpy(), minlength=degs.numel()) == 0)
    assert float(got['out'][degs == 0].abs().max()) == 0.0, 'degree-0 rows of out must be exact zeros'
    if bool(sink.any()):
        assert float(got['grad_x'][sink].abs().max()) == 0.0, 'grad_x rows of nodes without out-edges must be exact zeros'
    again = run_op(case, dtype)
    for k in got:
        if k != 'grad_w' or case['idxe'] is None:
            assert torch.equal(got[k], again[k]), f"{case['name']}: {k} differs between two calls"
    return got


OP_F32 = [a for a in C.OP_CASES if not a[3]]
OP_F64 = [a for a in C.OP_CASES if a[1] == '10x15 matrix']


@pytest.mark.parametrize('args', OP_F32, ids=lambda a: '-'.join(str(v) for v in a))
def test_operator_float32_at_the_ladder(hip, args):
    judge_op(args, torch.float32)


@pytest.mark.parametrize('args', OP_F64, ids=lambda a: '-'.join(str(v) for v in a))
def test_operator_float64_at_the_ladder(hip, args):
    judge_op(args, torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# c. the recurrent module
# ---------------------------------------------------------------------------------------------------------------------
# the launch form every graph is meant to run with a GRU cell and spg_tune key 8 = 0, on the 256 CUs of an MI355X
PER_ITERATION = 'per-iteration launches'
FORMS = {3: 'persistent, 1 workgroup per CU', 5: 'persistent, 1 workgroup per CU', 200: 'persistent, 1 workgroup per CU',
         1008: 'persistent, 1 workgroup per CU', 1024: PER_ITERATION, 1025: 'persistent, 2 workgroups per CU', 2049: 'iteration-major',
         'scenes': 'persistent, 2 workgroups per CU, 2 rounds'}
# (config, graph key, training, spg_tune key 8): the cases of ecc_cases.MODULE_CASES in their default launch form, and the GRU
# configurations at n = 200 through the per-iteration launches
GPU_MODULE = [a + (0,) for a in C.MODULE_CASES] + [(c, 200, True, 1) for c in ('matrix', 'vector', 'plain')]
WG_NODES, MAX_NODES, MAX_GROUPS, MULTI_MAX_NODES, MULTI_NPW = 1024, 2048, 8, 16000, 8        # csrc/spg_ecc.h, csrc/spg_ecc.hip


def plan_rounds(n, parts):
    """spg_px_plan_groups: node counts of the rounds of a launch, or None (per-iteration launches)."""
    big = [n] if n <= MULTI_MAX_NODES else None
    if n <= MAX_NODES:
        return [n]
    if parts is None or len(parts) < 3:                       # (RNNGraphConvModule._cfg_for hands the parts over above 2048 nodes only)
        return big
    bounds, start = [0], 0
    for a, b in zip(parts[:-1], parts[1:]):
        if b - a > MAX_NODES:
            return big
        if b - start > MAX_NODES:
            if len(bounds) >= MAX_GROUPS:
                return big
            bounds.append(a)
            start = a
    bounds.append(n)
    return [int(v) for v in np.diff(bounds)]


def launch_form(config, n, parts, per_iteration, cus):
    """The form eccrnn_recurrent_forward / spg_launch_ecc_persist_{fwd,bwd} / px_acquire choose for a case on a device of `cus` CUs."""
    rounds = None if (config == 'lstm' or per_iteration) else plan_rounds(n, parts)
    if rounds is None:
        return PER_ITERATION
    mg = max(rounds)
    if len(rounds) == 1 and mg > MAX_NODES:
        return 'iteration-major' if mg <= 4 * 2 * (cus - 4) * MULTI_NPW else PER_ITERATION
    wpc = 1 if mg <= WG_NODES else 2
    if -(-mg // 4) > wpc * (cus - 4):                          # px_acquire: every workgroup must be resident at once
        return PER_ITERATION
    return f'persistent, {wpc} workgroup{"s" if wpc > 1 else ""} per CU' + (f', {len(rounds)} rounds' if len(rounds) > 1 else '')


def intended_form(config, gkey, per_iteration):
    return PER_ITERATION if (config == 'lstm' or per_iteration) else FORMS[gkey]


def run_module(case, per_iteration):
    """-> ({out, 'grad x', 'grad ecc.<parameter>'} on the host, the device's filter-network ReLU decisions or None in evaluation mode)."""
    from superpoint_graph_amd import _lib, ops
    from superpoint_graph_amd.learning import ecc, graphnet
    from test_gpu_baseline_parity import _hip_fnet_decisions
    L = _lib.lib()
    idxn, degs, parts = C.graph(case['gkey'])
    net = graphnet.GraphNetwork(C.CONFIGS[case['config']], 32, list(C.FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    net.load_state_dict({k[4:]: v for k, v in C.module_state(case['config']).items()})
    net = net.to(DEV)
    net.train(case['training'])
    gi = ecc.GraphConvInfo.from_buffers(idxn.clone(), degs.clone(), case['edgefeats'].clone(), None, None,
                                        parts=parts if len(parts) > 2 else None)
    captured = {}
    real = ops.eccrnn_forward

    def spy(*a, **kw):
        out = real(*a, **kw)
        captured['ecc'] = out[1]
        return out
    old = L.spg_tune(8, per_iteration)
    ops.eccrnn_forward = spy
    try:
        net.set_info([gi], 1)
        if not case['training']:
            with torch.no_grad():
                res, dec = {'out': net(case['x'].to(DEV))}, None
        else:
            xg = case['x'].to(DEV).requires_grad_(True)
            out = net(xg)
            out.backward(case['go'].to(DEV))
            res = {'out': out.detach(), 'grad x': xg.grad}
            res.update({'grad ecc.' + k: p.grad for k, p in net.named_parameters()})
        torch.cuda.synchronize()
        if case['training']:
            dec = _hip_fnet_decisions(captured['ecc'], C.module_spec(case['config']))
    finally:
        ops.eccrnn_forward = real
        held = L.spg_tune(8, old)
    assert held == per_iteration, 'spg_tune key 8 changed during the run'
    return {k: v.detach().cpu() for k, v in res.items()}, dec


def judge_module(args):
    from superpoint_graph_amd import _lib, ops
    config, gkey, training, per_iteration = args
    case = C.module_case(config, gkey, training)
    name = case['name'] + (', per-iteration launches' if per_iteration else '')
    _, degs, parts = C.graph(gkey)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    form = launch_form(config, int(degs.numel()), parts, per_iteration, cus)
    assert form == intended_form(config, gkey, per_iteration), f'{name}: a device of {cus} CUs runs this case as "{form}"'
    before = ops.persistent_ecc_status()
    got, dec = run_module(case, per_iteration)
    refs, n_diff, cond = C.module_refs(case, dec)
    fig = {k: C.bound_ratio(got[k], r) for k, r in refs.items()}
    for k, (err, ratio) in fig.items():
        print(f'{name}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound')
    print(f'{name}: {n_diff} ReLU decisions differ from the float64 reference')
    for k, r in refs.items():
        C.assert_bound(got[k], r, f'{name}: {k}')
    if training:
        assert set(refs) == set(got) - {'grad ' + k for k in C.NOISE[config]}
        for k in C.NOISE[config]:
            assert float(got['grad ' + k].abs().max()) < 1e-5, k
    assert _lib.lib().spg_ecc_persistent_errors() == 0
    assert before[0] == 0 and ops.persistent_ecc_status() == (0, before[1])        # no time-out, no optimiser update withheld
    again, _ = run_module(case, per_iteration)
    for k in got:
        assert torch.equal(got[k], again[k]), f'{name}: {k} differs between two runs'
    return fig, n_diff


@pytest.mark.parametrize('args', GPU_MODULE, ids=lambda a: '-'.join(str(v) for v in a))
def test_module_at_the_ladder(hip, args):
    judge_module(args)


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    from superpoint_graph_amd import _lib
    _lib.lib()
    lines = ['# python tests/test_gpu_ecc_edges.py',
             '# per case and tensor: worst |device - float64 reference|, worst error / bound of the device, the same ratio of the float32 CPU',
             '# evaluation of the reference.  Operator: bound = 1e-4 |ref| + 1e-5 max|ref row| (float64 runs: 1e-13 max|ref row|); module:',
             '# bound = 1e-4 |ref| + 1e-5 max|ref| per element (conftest.assert_elementwise); gradients of the module against the float64',
             '# backward with the decisions of the side under test.  In brackets: the launch form of the case (launch_form(), from the',
             '# case and the number of CUs of the device).',
             f"{'case':78s} {'tensor':30s} {'abs error':>10s} {'device':>8s} {'cpu f32':>8s}", '', '## the operator alone']
    top = {}
    for dtype, table in ((torch.float32, OP_F32), (torch.float64, OP_F64)):
        kw = {} if dtype == torch.float32 else dict(rtol=0.0, atol_frac=C.F64_TOL)
        for args in table:
            case, ref = C.op_case(*args), op_reference(args)
            dev_f, cpu_f = C.measure_rows(run_op(case, dtype), ref, **kw), C.measure_rows(C.op_eval(case, dtype), ref, **kw)
            for k in ref:
                lines.append(f"{case['name'] + ' ' + str(dtype)[6:]:78s} {k:30s} {dev_f[k][0]:10.3e} {dev_f[k][1]:8.3f} {cpu_f[k][1]:8.3f}")
                top['operator ' + str(dtype)[6:]] = max(top.get('operator ' + str(dtype)[6:], (0.0, '', '')), (dev_f[k][1], case['name'], k))
    lines += ['', '## the recurrent module (out, grad x, the worst parameter gradient)']
    for args in GPU_MODULE:
        case = C.module_case(*args[:3])
        name = case['name'] + (', per-iteration launches' if args[3] else '')
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        form = launch_form(args[0], int(C.graph(args[1])[1].numel()), C.graph(args[1])[2], args[3], cus)
        got, dec = run_module(case, args[3])
        refs, n_diff, _ = C.module_refs(case, dec)
        rec32 = {}
        cpu = C.module_eval(case, torch.float32, rec=rec32)
        refs32, _, _ = C.module_refs(case, C.decisions(rec32))
        dev_f = {k: C.bound_ratio(got[k], r) for k, r in refs.items()}
        cpu_f = {k: C.bound_ratio(cpu[k], r) for k, r in refs32.items()}
        params = [k for k in refs if k.startswith('grad ecc.')]
        shown = [k for k in ('out', 'grad x') if k in refs] + ([max(params, key=lambda k: dev_f[k][1])] if params else [])
        for k in shown:
            lines.append(f'{name:78s} {k:30s} {dev_f[k][0]:10.3e} {dev_f[k][1]:8.3f} {cpu_f[k][1]:8.3f}')
            top['module'] = max(top.get('module', (0.0, '', '')), (dev_f[k][1], name, k))
        lines.append(f"{name:78s} {'ReLU decisions that differ':30s} {n_diff:10d}   [{form}]")
    lines += ['', '## worst device ratio'] + [f'{op:18s} {r:8.3f}  {name}: {k}' for op, (r, name, k) in top.items()]
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
