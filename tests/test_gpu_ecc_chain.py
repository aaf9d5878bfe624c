"""The iteration chain of the one-launch RNN-ECC recurrences (spg_ecc_persist_{fwd,bwd}_kernel) at its degree and shape edges,
against the per-iteration launches (spg_tune key 8): the cell's bias values held in registers, the backward's loads of an
iteration issued as one batch in front of the wait for the neighbours, and its out-edge filters fetched back to back through
edge ids read first must leave every value BIT-IDENTICAL -- outputs (with cat_all: every saved state h^0 .. h^R; without it the
saved states reach the comparison through the weight gradients that read them), the gradient wrt h^0 and every parameter
gradient of the cell and of the filter network (the per-edge filter gradient is what the filter network's gradients start from).

One graph of 37 nodes (no multiple of the 4 nodes of a workgroup) holds a node of in-degree and one of out-degree 0, 1, 12 (the
register-resident filters of a wave), 13 and above 32 (one gather pass); every combination of input gate, row normalisation,
cat_all and matrix / vector filters runs R = 1, 2 and 10 iterations on it.  A 5-node ring is the smallest graph.  One case
drives the whole training step (FusedStep) against the module path, with superpoints that have no embedding row."""
import types

import numpy as np
import pytest
import torch

from conftest import build_model

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KMAX, CH = 12, 32      # SPG_PX_KMAX1, SPG_PX_CH (csrc/spg_ecc.hip)
N_EDGE = 37


def _edge_graph():
    """(idxn, degs, in-degrees, out-degrees): edges sorted by target.  Nodes 0 .. 9 carry the prescribed degrees, 10 .. 36 are a ring
    that also supplies their sources / takes their edges (multi-edges where a degree exceeds the 27 ring nodes)."""
    pool = list(range(10, N_EDGE))
    edges = [(pool[k], pool[(k + 1) % len(pool)]) for k in range(len(pool))]      # (source, target)
    edges += [(0, pool[0]), (pool[1], 1)]                                           # node 0: no in-edge; node 1: no out-edge
    for node, deg in ((2, 1), (4, KMAX), (6, KMAX + 1), (8, CH + 2)):               # prescribed in-degrees (out-degree 0)
        edges += [(pool[(3 * node + k) % len(pool)], node) for k in range(deg)]
    for node, deg in ((3, 1), (5, KMAX), (7, KMAX + 1), (9, CH + 3)):               # prescribed out-degrees (in-degree 0)
        edges += [(node, pool[(5 * node + k) % len(pool)]) for k in range(deg)]
    src = np.array([e[0] for e in edges]); tgt = np.array([e[1] for e in edges])
    order = np.argsort(tgt, kind='stable')
    src, tgt = src[order], tgt[order]
    indeg, outdeg = np.bincount(tgt, minlength=N_EDGE), np.bincount(src, minlength=N_EDGE)
    return torch.from_numpy(src.astype(np.int64)), torch.from_numpy(indeg.astype(np.int64)), indeg, outdeg


def _ring_graph(n):
    src = np.arange(n); tgt = (src + 1) % n
    order = np.argsort(tgt, kind='stable')
    return torch.from_numpy(src[order].astype(np.int64)), torch.from_numpy(np.bincount(tgt, minlength=n).astype(np.int64))


def test_the_edge_graph_has_the_degrees_it_is_meant_to_have():
    _, _, indeg, outdeg = _edge_graph()
    assert N_EDGE % 4 != 0 and 5 <= N_EDGE <= 40
    for d in (indeg, outdeg):
        assert {0, 1, KMAX, KMAX + 1} <= set(d.tolist()) and d.max() > CH


def _run(hip, net, gi, x, go, legacy):
    old = hip.spg_tune(8, 1 if legacy else 0)
    try:
        net.zero_grad()
        net.set_info([gi], 1)
        xg = x.clone().requires_grad_(True)
        out = net(xg)
        out.backward(go)
        torch.cuda.synchronize()
        return out.detach().clone(), xg.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters()}
    finally:
        hip.spg_tune(8, old)


def _both_paths_agree(hip, config, idxn, degs, what):
    from superpoint_graph_amd.learning import ecc, graphnet
    n, e = int(degs.numel()), int(idxn.numel())
    edgefeats = torch.randn(e, 13, generator=torch.Generator().manual_seed(1))
    x = torch.randn(n, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    torch.manual_seed(7)
    net = graphnet.GraphNetwork(config, 32, [13, 32, 128, 64], 1, 0, 2, 30000, use_pyg=0, cuda=1).to(DEV).train()
    gi = ecc.GraphConvInfo.from_buffers(idxn.clone(), degs.clone(), edgefeats.clone(), None, None)
    with torch.no_grad():
        net.set_info([gi], 1)
        width = net(x).shape[1]
    go = torch.randn(n, width, generator=torch.Generator().manual_seed(3)).to(DEV)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    ref = _run(hip, net, gi, x, go, legacy=True)
    net.load_state_dict(state0)
    got = _run(hip, net, gi, x, go, legacy=False)
    assert torch.isfinite(ref[0]).all() and float(ref[0].abs().max()) > 0
    assert torch.equal(got[0], ref[0]), f'{what}: outputs / saved states differ'
    assert torch.equal(got[1], ref[1]), f'{what}: grad_h0 differs'
    assert set(got[2]) == set(ref[2]) and len(ref[2]) >= 10
    for k in ref[2]:
        assert torch.equal(got[2][k], ref[2][k]), f'{what}: gradient of {k} differs'


@pytest.mark.parametrize('cat_all', [0, 1])
@pytest.mark.parametrize('ingate', [0, 1])
@pytest.mark.parametrize('layernorm', [0, 1])
@pytest.mark.parametrize('vv', [0, 1])
def test_one_launch_chain_is_bit_identical_at_degree_edges(hip, vv, layernorm, ingate, cat_all):
    idxn, degs, _, _ = _edge_graph()
    for R in (1, 2, 10):
        config = f'gru_{R}_{vv}_{layernorm}_{ingate}_{cat_all},f_8'
        _both_paths_agree(hip, config, idxn, degs, config)
    assert hip.spg_ecc_persistent_errors() == 0


@pytest.mark.parametrize('config', ['gru_10_0,f_13', 'gru_2_1_0_0_0,f_5'])
def test_one_launch_chain_on_the_smallest_graph(hip, config):
    idxn, degs = _ring_graph(5)
    _both_paths_agree(hip, config, idxn, degs, config + ' on a 5-node ring')
    assert hip.spg_ecc_persistent_errors() == 0


def _step(hip, spec, state0, batch, fused, legacy):
    """One training step: through the modules, or as one library call with the classifier and the loss as launches of their own
    (spg_tune key 15: the same kernels as the modules, tests/test_gpu_fused.py) -- with the one-launch recurrence or, `legacy`,
    the per-iteration launches."""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.flat import FlatParameters
    from superpoint_graph_amd.fused import FusedStep
    from superpoint_graph_amd.learning import ecc, pointnet
    model = build_model(spec, state0).to(DEV).train()
    arena = FlatParameters(model, lazy_zero=True, host_counters=True)
    gi = ecc.GraphConvInfo.from_buffers(batch['idxn'].clone(), batch['degs'].clone(), batch['edgefeats'].clone())
    model.ecc.set_info([gi], 1)
    label = batch['label_mode'].to(DEV)
    old8, old15 = hip.spg_tune(8, 1 if legacy else 0), hip.spg_tune(15, 1)
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


def test_fused_step_against_the_module_path_with_rows_without_embedding(hip):
    from oracle import spg_oracle as O
    from superpoint_graph_amd import synth
    spec = O.ModelSpec()
    col = synth.collate_numpy([synth.scene(5, n_sp=37, n_edges=150, small_frac=0.1)])
    idxn, degs, ef, _ = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    batch = dict(clouds_flag=torch.from_numpy(col['clouds_flag']), clouds=torch.from_numpy(col['clouds']),
                 clouds_global=torch.from_numpy(col['clouds_global']), idxn=torch.from_numpy(idxn), degs=torch.from_numpy(degs),
                 edgefeats=torch.from_numpy(ef), label_mode=torch.from_numpy(col['targets'][:, 0].copy()))
    assert int((batch['clouds_flag'] != 0).sum()) > 0, 'no superpoint without an embedding row'
    torch.manual_seed(1)
    ref = build_model(spec)
    with torch.no_grad():
        ref.ptn.stn.proj.weight.normal_(0, 0.02)
    state0 = {k: v.clone() for k, v in ref.state_dict().items()}
    modules = _step(hip, spec, state0, batch, fused=False, legacy=False)
    for what, other in (('one call, one-launch recurrence', _step(hip, spec, state0, batch, fused=True, legacy=False)),
                        ('one call, per-iteration launches', _step(hip, spec, state0, batch, fused=True, legacy=True))):
        assert torch.equal(other[0], modules[0]) and float(modules[0]) > 0, (what, float(other[0]), float(modules[0]))
        assert torch.equal(other[1], modules[1]) and torch.equal(other[2], modules[2]), what
        for k in modules[3]:
            assert torch.equal(other[3][k], modules[3][k]), (what, k)
    assert hip.spg_ecc_persistent_errors() == 0
