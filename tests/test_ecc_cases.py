"""CPU: the graphs, cases, references and knobs of tests/ecc_cases.py, which tests/test_gpu_ecc_edges.py holds the device to.

* every ladder graph has exactly the stated in- and out-degrees, edges sorted by target, whole scenes as parts;
* ADMISSION: the float32 CPU evaluation of every case stays within ADMIT of the bound on every compared tensor (the worst figure per
  case is printed; run with -s) -- the filter network's ReLU decisions of the float32 run are handed to the float64 backward, and
  they differ from the float64 run's own only on near-ties;
* KNOBS: every restated kernel mistake leaves the bound on at least one case, the order-only knob stays inside it, and the
  restatement with all knobs off equals the oracle bit for bit;
* the parameter gradients left out of the comparison are exactly the filter network's bias in front of its train-mode BatchNorm."""
import numpy as np
import pytest
import torch

import ecc_cases as C
from conftest import noise_grad
from oracle import spg_oracle as O


# ---------------------------------------------------------------------------------------------------------------------
# graph shape
# ---------------------------------------------------------------------------------------------------------------------
def _edges(idxn, degs):
    return idxn.numpy(), O.edge_targets(degs.numpy())


@pytest.mark.parametrize('key', C.SIZES + ('scenes',))
def test_ladder_graph_has_the_stated_degrees(key):
    idxn, degs, parts = C.graph(key)
    n = int(degs.numel())
    src, tgt = _edges(idxn, degs)
    assert int(degs.sum()) == idxn.numel() == len(tgt) and bool((np.diff(tgt) >= 0).all())
    assert 0 <= src.min() and src.max() < n
    indeg, outdeg = degs.numpy(), np.bincount(src, minlength=n)
    scenes = C.SCENES if key == 'scenes' else None
    node = C.ladder_nodes(n, 0, scenes)
    assert len(set(node.tolist())) == C.MIN_N
    for role, (di, do) in C.ladder_degrees().items():
        assert (indeg[node[role]], outdeg[node[role]]) == (di, do), (role, node[role])
    base = n - (scenes[-1] if scenes else n)
    assert node[C.IN0 + 19] == n - 1 and node[C.OUT0 + 19] == n - 2
    # the special rungs
    e_self = (src == node[C.SELF]) & (tgt == node[C.SELF])
    assert e_self.sum() == 1 and ((src == tgt).sum() == 1)
    assert ((src == node[C.TRI_SRC]) & (tgt == node[C.TRI_DST])).sum() == 3
    assert set(src[tgt == node[C.MONO_HUB]].tolist()) == {int(node[C.MONO_SRC])}
    for k, d in enumerate(C.LADDER):                               # ladder hubs: distinct sources / targets
        assert len(set(src[tgt == node[C.IN0 + k]].tolist())) == d and len(set(tgt[src == node[C.OUT0 + k]].tolist())) == d
    # everything outside the 200 roles is isolated (single graph) or on the other scenes' rings
    other = np.setdiff1d(np.arange(base, n), node)
    assert indeg[other].sum() == 0 and outdeg[other].sum() == 0
    ladder_edges = 2 * sum(C.LADDER) + 2 * len(C.LADDER) + 2 * C.BOTH_DEG + 3 + 5 + C.MONO_DEG + 2 + 2 + (C.RING1 - C.POOL0)
    assert ladder_edges == 1202 and idxn.numel() == ladder_edges + (60 * (len(scenes) - 1) if scenes else 0)
    # parts are whole scenes: no edge crosses a boundary
    assert parts[0] == 0 and parts[-1] == n and parts == sorted(parts)
    inner = np.asarray(parts[1:-1])
    assert np.array_equal(np.searchsorted(inner, src, side='right'), np.searchsorted(inner, tgt, side='right'))
    if scenes:
        assert parts == [0, 700, 1600, 2200] and node.min() >= 1600


@pytest.mark.parametrize('n', C.TINY)
def test_tiny_graph_has_the_stated_degrees(n):
    idxn, degs, parts = C.graph(n)
    src, tgt = _edges(idxn, degs)
    assert int(degs.sum()) == idxn.numel() and bool((np.diff(tgt) >= 0).all()) and parts == [0, n]
    assert tuple(degs.tolist()) == C.TINY_IN[n] and tuple(np.bincount(src, minlength=n).tolist()) == C.TINY_OUT[n]
    assert ((src == 0) & (tgt == 0)).sum() == 1 and ((src == 1) & (tgt == 0)).sum() == 2


def test_ladder_graph_depends_on_the_seed_only():
    a, b, c = C.ladder_graph(200, 0), C.ladder_graph(200, 0), C.ladder_graph(200, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])


# ---------------------------------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('args', C.OP_CASES, ids=lambda a: '-'.join(str(v) for v in a))
def test_operator_cases_are_admitted(args):
    case = C.op_case(*args)
    ref, cpu = C.op_eval(case, torch.float64), C.op_eval(case, torch.float32)
    fig = C.measure_rows(cpu, ref)
    print(f"{case['name']}: float32 CPU worst ratio {C.worst(fig):.4f} ({', '.join(f'{k} {r:.4f}' for k, (_, r) in fig.items())})")
    assert C.worst(fig) <= C.ADMIT, fig
    idxn, degs, _ = C.graph(case['gkey'])
    sink = torch.from_numpy(np.bincount(idxn.numpy(), minlength=degs.numel()) == 0)
    assert bool((degs == 0).any()) and float(ref['out'][degs == 0].abs().max()) == 0.0
    assert not bool(sink.any()) or float(ref['grad_x'][sink].abs().max()) == 0.0


@pytest.mark.parametrize('args', C.MODULE_CASES, ids=lambda a: '-'.join(str(v) for v in a))
def test_module_cases_are_admitted(args):
    case = C.module_case(*args)
    rec32 = {}
    cpu = C.module_eval(case, torch.float32, rec=rec32)
    refs, n_diff, _ = C.module_refs(case, C.decisions(rec32))
    fig = {k: C.bound_ratio(cpu[k], r) for k, r in refs.items()}
    top = max(fig, key=lambda k: fig[k][1])
    print(f"{case['name']}: float32 CPU worst ratio {fig[top][1]:.4f} ({top}); {n_diff} ReLU decisions differ from float64")
    assert fig[top][1] <= C.ADMIT, {k: v for k, v in fig.items() if v[1] > C.ADMIT}


# ---------------------------------------------------------------------------------------------------------------------
# knobs
# ---------------------------------------------------------------------------------------------------------------------
KNOB_OP = [C.op_case(200, s, 1.0) for s in ('32x32 matrix', '32 vector')] + [C.op_case(5, '32x32 matrix', 1.0)]
KNOB_MODULE = [C.module_case('matrix', 200), C.module_case('vector', 5)]


def _op_ratio(case, knobs):
    ref, bad = C.op_eval(case, torch.float64), C.op_eval(case, torch.float64, **knobs)
    return C.worst(C.measure_rows(bad, ref))


def _module_ratio(case, knobs):
    ref, bad = C.module_eval(case, torch.float64), C.module_eval(case, torch.float64, **knobs)
    return max(C.bound_ratio(bad[k], ref[k])[1] for k in C.compared(case, ref))


@pytest.mark.parametrize('name', list(C.KNOBS))
def test_every_mistake_leaves_the_bound(name):
    knobs = C.KNOBS[name]
    op = {} if name in C.MODULE_ONLY else {c['name']: _op_ratio(c, knobs) for c in KNOB_OP}
    module = {c['name']: _module_ratio(c, knobs) for c in KNOB_MODULE}
    print(name, {k: f'{v:.3g}' for k, v in {**op, **module}.items()})
    assert max(module.values()) > 1.0, module
    if name not in C.MODULE_ONLY:            # ... and the operator cases see it as well as the ladder module case
        assert max(op.values()) > 1.0 and module[KNOB_MODULE[0]['name']] > 1.0, (op, module)


def test_order_only_knob_stays_inside_the_bound():
    (name, knobs), = C.ORDER_ONLY.items()
    for c in KNOB_OP:
        ref, got = C.op_eval(c, torch.float64), C.op_eval(c, torch.float64, **knobs)
        assert C.worst(C.measure_rows(got, ref, rtol=0.0, atol_frac=C.F64_TOL)) <= 1.0
        ref32, got32 = C.op_eval(c, torch.float32), C.op_eval(c, torch.float32, **knobs)        # ... in float32 as well
        assert C.worst(C.measure_rows(got32, ref)) <= C.ADMIT and C.worst(C.measure_rows(ref32, ref)) <= C.ADMIT
    assert _module_ratio(KNOB_MODULE[0], knobs) <= C.ADMIT
    # the knob does change the order: some element of the float32 grad_x differs
    c = KNOB_OP[0]
    assert not torch.equal(C.op_eval(c, torch.float32)['grad_x'], C.op_eval(c, torch.float32, **knobs)['grad_x'])


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restatement_with_all_knobs_off_is_the_oracle(dtype):
    for c in KNOB_OP + [C.op_case(200, '10x15 matrix', 1.0, True)]:
        a, b = C.op_eval(c, dtype), C.op_eval(c, dtype, tail=None)
        for k in a:
            assert torch.equal(a[k], b[k]), (c['name'], k)
    for c in KNOB_MODULE + [C.module_case('lstm', 200)]:
        a, b = C.module_eval(c, dtype), C.module_eval(c, dtype, tail=None)
        for k in a:
            assert torch.equal(a[k], b[k]), (c['name'], k)


# ---------------------------------------------------------------------------------------------------------------------
# excluded parameter gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', list(C.CONFIGS))
def test_excluded_gradients_are_the_bias_in_front_of_the_batchnorm(config):
    for gkey in sorted({g for c, g, t in C.MODULE_CASES if c == config and t}, key=str):
        case = C.module_case(config, gkey)
        ref = C.module_eval(case, torch.float64)
        pg = C.param_grads(ref)
        excluded = tuple(sorted(k for k in pg if noise_grad(k, pg)))
        assert excluded == C.NOISE[config], (gkey, excluded)
        assert set(C.compared(case, ref)) == set(ref) - {'grad ' + k for k in C.NOISE[config]}
        # analytically zero: the float64 reference holds round-off only
        top = max(float(v.abs().max()) for v in pg.values())
        assert float(pg['ecc.0._fnet.4.bias'].abs().max()) <= 1e-9 * top
        spec = C.module_spec(config)
        assert spec.fnet_bnidx == 2 and 'ecc.0._fnet.5.running_mean' in C.module_state(config)
