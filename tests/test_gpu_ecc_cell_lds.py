"""The cell backward and the edge products of the one-launch RNN-ECC recurrences (spg_ecc_persist_{fwd,bwd}_kernel) with their
LDS reads issued in batches: the W^T and input-gate products of spg_gru_backward_node read a batch of gate rows (weights by column,
operands as 128-bit broadcasts) in front of that batch's multiply-adds under a loop counter that is the same for every lane, and
the products over the register-resident edges read all neighbour rows first and skip the products of absent edges.  Only the
order in which reads are issued changed, so

  * outputs, the gradient wrt h^0 and every parameter gradient are BIT-IDENTICAL between the one-launch path, the per-iteration
    launches (spg_tune key 8) and -- at 10 iterations -- the one-launch backward behind a per-iteration forward (that forward clears
    the save tag: the backward then recomputes the cell from aggregate and state instead of reading the forward's internals);
  * because both paths share spg_gru_backward_node, one case per (input gate, row normalisation) is also compared per element
    with the float64 oracle (oracle/spg_oracle.py) under the bound of tests/test_gpu_ecc_edges.py (conftest.assert_elementwise's
    defaults, ReLU near-ties of the filter network handed over as that file does).

THE GRAPH has 39 nodes (no multiple of the 4 nodes of a workgroup).  Nodes 0 .. 11 carry the prescribed degrees -- a node of
in-degree and one of out-degree 0, 1, 11, 12 (the register-resident edges of a wavefront, SPG_PX_KMAX1), 13 and above
SPG_PX_CH = 32 (a second gather pass) -- and 12 .. 38 are a ring that supplies their sources and takes their edges.  A 5-node
ring is the smallest graph.

THE CELL WEIGHTS (weight_ih, weight_hh, ig.weight) are drawn i.i.d. normal with standard deviation 32^-1/2: no symmetric or
structured initialisation behind which a transposed or shifted index of the batched reads could hide, and a scale that keeps the
pre-activations of a 32-wide row of order 1 (a larger one saturates the gates without row normalisation, and the float32 round-off
of any correct kernel then leaves the bound: the CPU test below admits the cases with a float32 evaluation of the oracle).

One case runs the whole training step (FusedStep) on two scenes of 520 superpoints -- 1040 nodes, above the 1024 of one workgroup
per CU: the kernels with two workgroups per CU and the small batch depth -- against the module path."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path)
import ecc_cases as C
from conftest import build_model, noise_grad
from oracle import spg_oracle as O

gpu = pytest.mark.gpu
DEV = 'cuda'
KMAX, CH = 12, 32      # SPG_PX_KMAX1, SPG_PX_CH (csrc/spg_ecc.hip)
N_NODES = 39
DEGREES = (1, KMAX - 1, KMAX, KMAX + 1, CH + 2)
FNET = [13, 32, 128, 64]


# =====================================================================================================================
# graphs and inputs
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def degree_graph():
    """-> (idxn, degs, in-degrees, out-degrees), edges sorted by target (stable)."""
    pool = list(range(12, N_NODES))
    edges = [(pool[k], pool[(k + 1) % len(pool)]) for k in range(len(pool))]      # (source, target)
    edges += [(0, pool[0]), (pool[1], 1)]                                           # node 0: no in-edge; node 1: no out-edge
    for node, deg in zip((2, 4, 6, 8, 10), DEGREES):                                # prescribed in-degrees (out-degree 0)
        edges += [(pool[(3 * node + k) % len(pool)], node) for k in range(deg)]
    for node, deg in zip((3, 5, 7, 9, 11), DEGREES):                                # prescribed out-degrees (in-degree 0)
        edges += [(node, pool[(5 * node + k) % len(pool)]) for k in range(deg + (deg > CH))]
    src = np.array([e[0] for e in edges]); tgt = np.array([e[1] for e in edges])
    order = np.argsort(tgt, kind='stable')
    src, tgt = src[order], tgt[order]
    indeg, outdeg = np.bincount(tgt, minlength=N_NODES), np.bincount(src, minlength=N_NODES)
    return torch.from_numpy(src.astype(np.int64)), torch.from_numpy(indeg.astype(np.int64)), indeg, outdeg


@functools.lru_cache(maxsize=None)
def ring_graph(n=5):
    src = np.arange(n); tgt = (src + 1) % n
    order = np.argsort(tgt, kind='stable')
    return torch.from_numpy(src[order].astype(np.int64)), torch.from_numpy(np.bincount(tgt, minlength=n).astype(np.int64))


def test_the_graph_has_the_degrees_it_is_meant_to_have():
    _, degs, indeg, outdeg = degree_graph()
    assert N_NODES % 4 != 0 and N_NODES <= 40 and int(degs.numel()) == N_NODES
    for d in (indeg, outdeg):
        assert {0, 1, KMAX - 1, KMAX, KMAX + 1} <= set(d.tolist()) and d.max() > CH


def config_of(R, vv, layernorm, ingate, cat_all):
    return f'gru_{R}_{vv}_{layernorm}_{ingate}_{cat_all}'


@functools.lru_cache(maxsize=None)
def make_case(config, ring=False):
    """Inputs and the float32 state_dict (keys as graphnet.GraphNetwork names them) of one case: the module's own initialisation
    (seed 7) with the cell's three weight matrices redrawn i.i.d. normal, standard deviation 32^-1/2."""
    from superpoint_graph_amd.learning import graphnet
    idxn, degs = ring_graph() if ring else degree_graph()[:2]
    n, e = int(degs.numel()), int(idxn.numel())
    g = torch.Generator().manual_seed(41 + n)
    x = torch.randn(n, 32, generator=g)
    ef = torch.randn(e, 13, generator=g)
    with torch.random.fork_rng():
        torch.manual_seed(7)
        net = graphnet.GraphNetwork(config, 32, list(FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    drawn = [k for k in state if '_cell.' in k and k.endswith(('ig.weight', 'weight_ih', 'weight_hh'))]
    assert len(drawn) == 2 + int(config.split('_')[4]), drawn
    for k in drawn:
        state[k] = torch.randn(state[k].shape, generator=g) * 32 ** -0.5
    R, cat_all = int(config.split('_')[1]), int(config.split('_')[5])
    go = torch.randn(n, 32 * (R + 1) if cat_all else 32, generator=g)
    return dict(config=config, idxn=idxn, degs=degs, x=x, ef=ef, go=go, state=state, name=config + (' on a 5-node ring' if ring else ''))


def oracle_eval(case, dtype=torch.float64, dec=None, rec=None):
    """-> {out, 'grad x', 'grad ecc.<parameter>'} of oracle.spg_oracle.graph_network_forward under torch autograd, on the CPU."""
    spec = O.ModelSpec(model_config=case['config'])
    P = {'ecc.' + k: (v.to(dtype).clone().requires_grad_(True) if (O.is_param_key('ecc.' + k) and v.is_floating_point()) else v.clone())
         for k, v in case['state'].items()}
    x = case['x'].to(dtype).clone().requires_grad_(True)
    out = O.graph_network_forward(x, case['ef'].to(dtype), case['idxn'], case['degs'], spec, P, True, dec=dec, rec=rec)
    out.backward(case['go'].to(dtype))
    res = {'out': out.detach(), 'grad x': x.grad}
    for k, v in P.items():
        if v.requires_grad:
            res['grad ' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return res


def judged(ref):
    pg = C.param_grads(ref)
    return [k for k in ref if not (k.startswith('grad ecc.') and noise_grad(k[5:], pg))]


ORACLE_CONFIGS = [config_of(3, 0, ln, ig, 1) for ln in (0, 1) for ig in (0, 1)]


@pytest.mark.parametrize('config', ORACLE_CONFIGS)
def test_the_oracle_alone_is_finite_and_admits_the_case(config):
    """On the CPU: the float64 oracle is finite on these inputs and not degenerate, and its float32 evaluation stays within
    ADMIT = 0.25 of the bound on every judged tensor (the rule of tests/ecc_cases.py: a case any correct float32 evaluation could
    miss is no case)."""
    case = make_case(config)
    rec = {}
    ref = oracle_eval(case, torch.float64, rec=rec)
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()), k
    assert float(ref['out'].abs().max()) > 0 and float(ref['grad x'].abs().max()) > 0
    for k in ('weight_ih', 'weight_hh'):
        assert float(ref['grad ecc.0._cell.' + k].abs().max()) > 0, k
    f32 = oracle_eval(case, torch.float32, dec=C.decisions(rec))
    for k in judged(ref):
        err, ratio = C.bound_ratio(f32[k], ref[k])
        print(f'{config}: {k}: float32 on the CPU: worst error {err:.3e}, {ratio:.3f} of the bound')
        assert ratio <= C.ADMIT, (k, ratio)


# =====================================================================================================================
# the device
# =====================================================================================================================
def _net(case):
    from superpoint_graph_amd.learning import ecc, graphnet
    net = graphnet.GraphNetwork(case['config'], 32, list(FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    net.load_state_dict(case['state'])
    net = net.to(DEV).train()
    gi = ecc.GraphConvInfo.from_buffers(case['idxn'].clone(), case['degs'].clone(), case['ef'].clone(), None, None)
    return net, gi


def _run(hip, case, forward_legacy, backward_legacy, capture=None):
    """One forward + backward of the module; spg_tune key 8 is set for the forward and again for the backward."""
    from superpoint_graph_amd import ops
    net, gi = _net(case)
    real = ops.eccrnn_forward

    def spy(*a, **kw):
        out = real(*a, **kw)
        if capture is not None:
            capture['ecc'] = out[1]
        return out
    old = hip.spg_tune(8, 1 if forward_legacy else 0)
    ops.eccrnn_forward = spy
    try:
        net.set_info([gi], 1)
        xg = case['x'].to(DEV).requires_grad_(True)
        out = net(xg)
        hip.spg_tune(8, 1 if backward_legacy else 0)
        out.backward(case['go'].to(DEV))
        torch.cuda.synchronize()
        res = {'out': out.detach().clone(), 'grad x': xg.grad.clone()}
        res.update({'grad ecc.' + k: p.grad.clone() for k, p in net.named_parameters()})
        return res
    finally:
        ops.eccrnn_forward = real
        hip.spg_tune(8, old)


def _same(got, ref, what):
    assert set(got) == set(ref) and len(ref) >= 10
    assert bool(torch.isfinite(ref['out']).all()) and float(ref['out'].abs().max()) > 0
    for k in ref:
        assert torch.equal(got[k], ref[k]), f'{what}: {k} differs'


def _paths_agree(hip, case, mixed):
    ref = _run(hip, case, True, True)
    _same(_run(hip, case, False, False), ref, case['name'] + ': one launch against per-iteration launches')
    if mixed:
        _same(_run(hip, case, True, False), ref, case['name'] + ': one-launch backward (recompute) behind a per-iteration forward')


@gpu
@pytest.mark.parametrize('ingate', [0, 1])
@pytest.mark.parametrize('layernorm', [0, 1])
@pytest.mark.parametrize('vv', [0, 1])
def test_batched_reads_are_bit_identical_across_the_paths(hip, vv, layernorm, ingate):
    for R, cat_all in ((1, 1), (2, 1), (10, 1), (10, 0)):
        _paths_agree(hip, make_case(config_of(R, vv, layernorm, ingate, cat_all)), mixed=R == 10)
    assert hip.spg_ecc_persistent_errors() == 0


@gpu
@pytest.mark.parametrize('config', [config_of(10, 0, 1, 1, 0), config_of(2, 1, 0, 0, 1)])
def test_batched_reads_on_the_smallest_graph(hip, config):
    _paths_agree(hip, make_case(config, ring=True), mixed=config.startswith('gru_10'))
    assert hip.spg_ecc_persistent_errors() == 0


def _fnet_decisions(hip, st, spec):
    """ReLU decisions of the filter network on the device, from the RNN-ECC forward workspace (`y > 0`, behind the BatchNorm layer
    `y s + t > 0`), as tests/test_gpu_ecc_edges.py takes them."""
    cfg, ws, N, E = st.cfg, st.ws, st.graph.N, st.graph.E
    dec = {}
    for k, c in enumerate(spec.fnet_widths):
        def buf(what, n):
            off = hip.spg_eccrnn_debug_offset(ctypes.byref(cfg), N, E, 1, k, what)
            assert off >= 0, (k, what)
            return ws[off:off + 4 * n].view(torch.float32)
        v = buf(0, E * c).view(E, c).double()
        if spec.fnet_bnidx == k:
            v = v * buf(1, c).double() + buf(2, c).double()
        dec[f'ecc.0._fnet.relu{k}'] = (v > 0).cpu()
    return dec


@functools.lru_cache(maxsize=None)
def _reference(config):
    rec = {}
    return oracle_eval(make_case(config), torch.float64, rec=rec), rec


@gpu
@pytest.mark.parametrize('per_iteration', [0, 1])
@pytest.mark.parametrize('config', ORACLE_CONFIGS)
def test_cell_backward_against_the_float64_oracle(hip, config, per_iteration):
    case = make_case(config)
    captured = {}
    got = _run(hip, case, bool(per_iteration), bool(per_iteration), capture=captured)
    free, rec = _reference(config)
    dec = _fnet_decisions(hip, captured['ecc'], O.ModelSpec(model_config=config))
    n_diff = C.check_near_ties(dec, rec)
    cond = free if n_diff == 0 else oracle_eval(case, torch.float64, dec=dec)
    keys = judged(cond)
    assert {'out', 'grad x', 'grad ecc.0._cell.weight_ih', 'grad ecc.0._cell.weight_hh'} <= set(keys)
    for k in keys:
        ref = (free if k == 'out' else cond)[k]
        err, ratio = C.bound_ratio(got[k].cpu(), ref)
        print(f'{config}, key 8 = {per_iteration}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound')
    for k in keys:
        C.assert_bound(got[k].cpu(), (free if k == 'out' else cond)[k], f'{config}: {k}')
    assert hip.spg_ecc_persistent_errors() == 0


# =====================================================================================================================
# the training step on 1040 nodes: two workgroups per CU
# =====================================================================================================================
def _step(hip, spec, state0, batch, fused):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.flat import FlatParameters
    from superpoint_graph_amd.fused import FusedStep
    from superpoint_graph_amd.learning import ecc, pointnet
    model = build_model(spec, state0).to(DEV).train()
    arena = FlatParameters(model, lazy_zero=True, host_counters=True)
    gi = ecc.GraphConvInfo.from_buffers(batch['idxn'].clone(), batch['degs'].clone(), batch['edgefeats'].clone())
    model.ecc.set_info([gi], 1)
    label = batch['label_mode'].to(DEV)
    old8, old15 = hip.spg_tune(8, 0), hip.spg_tune(15, 1)      # (key 15: classifier and loss as launches of their own, the modules' kernels)
    try:
        arena.zero_grad()
        if fused:
            step = FusedStep(model, arena)
            loss, logits = step(batch['clouds_flag'], batch['clouds'], batch['clouds_global'], gi, label)
            emb = step.embeddings
        else:
            embedder = pointnet.CloudEmbedder(types.SimpleNamespace(cuda=1, ptn_mem_monger=1))
            emb = embedder.run(model, None, batch['clouds_flag'], batch['clouds'], batch['clouds_global'])
            logits = model.ecc(emb)
            loss = ops.cross_entropy(logits, label, weight=None, reduction='mean')
            loss.backward(arena.one)
            embedder.bw_hook()
        torch.cuda.synchronize()
        return loss.detach().clone(), logits.detach().clone(), emb.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}
    finally:
        hip.spg_tune(8, old8); hip.spg_tune(15, old15)


@gpu
def test_fused_step_on_two_scenes_of_520_superpoints(hip):
    from superpoint_graph_amd import synth
    spec = O.ModelSpec()
    col = synth.collate_numpy([synth.scene(5, n_sp=520, n_edges=2600), synth.scene(6, n_sp=520, n_edges=2600)])
    idxn, degs, ef, _ = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    assert 1024 < int(degs.shape[0]) <= 2048
    batch = dict(clouds_flag=torch.from_numpy(col['clouds_flag']), clouds=torch.from_numpy(col['clouds']),
                 clouds_global=torch.from_numpy(col['clouds_global']), idxn=torch.from_numpy(idxn), degs=torch.from_numpy(degs),
                 edgefeats=torch.from_numpy(ef), label_mode=torch.from_numpy(col['targets'][:, 0].copy()))
    torch.manual_seed(1)
    ref = build_model(spec)
    with torch.no_grad():
        ref.ptn.stn.proj.weight.normal_(0, 0.02)
    state0 = {k: v.clone() for k, v in ref.state_dict().items()}
    modules = _step(hip, spec, state0, batch, fused=False)
    fused = _step(hip, spec, state0, batch, fused=True)
    assert torch.equal(fused[0], modules[0]) and float(modules[0]) > 0, (float(fused[0]), float(modules[0]))
    assert torch.equal(fused[1], modules[1]) and torch.equal(fused[2], modules[2])
    for k in modules[3]:
        assert torch.equal(fused[3][k], modules[3][k]), k
    assert hip.spg_ecc_persistent_errors() == 0
