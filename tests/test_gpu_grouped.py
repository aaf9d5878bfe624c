"""Grouped launches (round 4; superpoint_graph_amd/csrc/spg_gemm.h: SpgGroupScope, spg_multi_kernel): mutually independent
few-row GEMMs / small reductions of a training step leave as jobs of ONE kernel.  Every job executes the unchanged body of the
kernel it replaces, so a whole training step must be BIT-IDENTICAL with grouping on and off (spg_tune key 11) -- loss, logits,
embeddings, all gradients, the BatchNorm running statistics -- on the production config (matrix filters), a vector-filter
config, batch sizes that make the few-row tiles complete (multiples of 32: FULL kernel variants) and ragged, with and without
the flat gradient arena."""
import pytest
import torch
import torch.nn.functional as F

from conftest import build_model, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _step(model, batch, cw, arena):
    import types
    from superpoint_graph_amd.learning import ecc, pointnet
    gi = ecc.GraphConvInfo.from_buffers(batch['idxn'].clone(), batch['degs'].clone(), batch['edgefeats'].clone())
    model.ecc.set_info([gi], 1)
    embedder = pointnet.CloudEmbedder(types.SimpleNamespace(cuda=1, ptn_mem_monger=1))
    if arena is not None:
        arena.zero_grad()
    else:
        model.zero_grad()
    emb = embedder.run(model, None, batch['clouds_flag'], batch['clouds'], batch['clouds_global'])
    logits = model.ecc(emb)
    loss = F.cross_entropy(logits, batch['label_mode'].to(DEV), weight=cw)
    loss.backward()
    embedder.bw_hook()
    torch.cuda.synchronize()
    return (loss.detach().clone(), logits.detach().clone(), emb.detach().clone(),
            {k: p.grad.clone() for k, p in model.named_parameters()},
            {k: v.clone() for k, v in model.state_dict().items() if 'running' in k})


@pytest.mark.parametrize('tag', ['s3dis_gru10_matrix', 'vector_gru4_small', 'lstm3_matrix_small'])
@pytest.mark.parametrize('flat', [False, True])
def test_training_step_bit_identical_with_and_without_grouping(hip, tag, flat):
    from superpoint_graph_amd.flat import FlatParameters
    spec, batch, state0, g = load_golden(tag)
    cw = torch.from_numpy(g['class_weights']).to(DEV) if 'class_weights' in g.files else None
    res = []
    for off in (1, 0):
        old = hip.spg_tune(11, off)
        try:
            model = build_model(spec, state0).to(DEV).train()
            arena = FlatParameters(model, lazy_zero=True) if flat else None
            res.append(_step(model, batch, cw, arena))
        finally:
            hip.spg_tune(11, old)
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k


@pytest.mark.parametrize('n_sp,n_edges', [(1000, 5000), (992, 4992), (64, 320)])
def test_baseline_scene_bit_identical_with_and_without_grouping(hip, n_sp, n_edges):
    """BASELINE-size scene (ragged few-row tiles) and sizes whose row counts are multiples of 32 (complete tiles: the FULL
    variants of the grouped bodies)."""
    import numpy as np
    from oracle import spg_oracle as O
    from superpoint_graph_amd import synth
    from superpoint_graph_amd.flat import FlatParameters
    spec = O.ModelSpec()
    col = synth.collate_numpy([synth.scene(3, n_sp=n_sp, n_edges=n_edges)])
    idxn, degs, ef, _ = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    batch = dict(clouds_flag=torch.from_numpy(col['clouds_flag']), clouds=torch.from_numpy(col['clouds']),
                 clouds_global=torch.from_numpy(col['clouds_global']), idxn=torch.from_numpy(idxn), degs=torch.from_numpy(degs),
                 edgefeats=torch.from_numpy(ef), label_mode=torch.from_numpy(col['targets'][:, 0].copy()))
    torch.manual_seed(1)
    ref = build_model(spec)
    with torch.no_grad():
        ref.ptn.stn.proj.weight.normal_(0, 0.02)
    state0 = {k: v.clone() for k, v in ref.state_dict().items()}
    res = []
    for off in (1, 0):
        old = hip.spg_tune(11, off)
        try:
            model = build_model(spec, state0).to(DEV).train()
            arena = FlatParameters(model, lazy_zero=True)
            res.append(_step(model, batch, None, arena))
        finally:
            hip.spg_tune(11, old)
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    for k in a[4]:
        assert torch.equal(a[4][k], b[4][k]), k
    assert int(np.isfinite(a[1].cpu().numpy()).all())


@pytest.mark.parametrize('bnidx', [0, 1])
def test_filter_network_batchnorm_behind_an_early_layer(hip, bnidx):
    """--fnet_bnidx 0 / 1 are legal in the reference (learning/graphnet.py:17-37; only BatchNorm behind the LAST
    filter layer is rejected).  With BatchNorm behind layer 0 the layer's own GEMM is the first producer of its fixed-point
    statistics slots, and the slot clearing used to travel as a job of the SAME grouped launch -- statistics partly wiped,
    non-deterministically.  Checked here: grouped == ungrouped bit for bit (spg_tune key 11), the one-call step (where the filter
    network's layers ride with PointNet's launches) agrees with both, repeated runs are bit-stable, and all of it matches the CPU
    oracle."""
    from conftest import maxrel, noise_grad
    from oracle import spg_oracle as O
    from superpoint_graph_amd import synth
    from superpoint_graph_amd.flat import FlatParameters
    from superpoint_graph_amd.fused import FusedStep
    from superpoint_graph_amd.learning import ecc
    spec = O.ModelSpec(fnet_bnidx=bnidx)
    col = synth.collate_numpy([synth.scene(5, n_sp=300, n_edges=1500)])
    idxn, degs, ef, _ = O.set_batch(col['edge_lists'], col['vcounts'], col['edge_feats'])
    batch = dict(clouds_flag=torch.from_numpy(col['clouds_flag']), clouds=torch.from_numpy(col['clouds']),
                 clouds_global=torch.from_numpy(col['clouds_global']), idxn=torch.from_numpy(idxn), degs=torch.from_numpy(degs),
                 edgefeats=torch.from_numpy(ef), label_mode=torch.from_numpy(col['targets'][:, 0].copy()))
    torch.manual_seed(1)
    ref = build_model(spec)
    with torch.no_grad():
        ref.ptn.stn.proj.weight.normal_(0, 0.02)
    state0 = {k: v.clone() for k, v in ref.state_dict().items()}
    res = []
    for off in (1, 0, 0):
        old = hip.spg_tune(11, off)
        try:
            model = build_model(spec, state0).to(DEV).train()
            res.append(_step(model, batch, None, FlatParameters(model, lazy_zero=True)))
        finally:
            hip.spg_tune(11, old)
    for other in res[1:]:
        assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
        for k in res[0][3]:
            assert torch.equal(res[0][3][k], other[3][k]), k
        for k in res[0][4]:
            assert torch.equal(res[0][4][k], other[4][k]), k
    # the one-call step: the filter network's stages are riders of PointNet's grouped launches
    runs = []
    for _ in range(2):
        model = build_model(spec, state0).to(DEV).train()
        arena = FlatParameters(model, lazy_zero=True, host_counters=True)
        gi = ecc.GraphConvInfo.from_buffers(batch['idxn'].clone(), batch['degs'].clone(), batch['edgefeats'].clone())
        model.ecc.set_info([gi], 1)
        arena.zero_grad()
        loss, logits = FusedStep(model, arena)(batch['clouds_flag'], batch['clouds'], batch['clouds_global'], gi, batch['label_mode'].to(DEV))
        torch.cuda.synchronize()
        runs.append((loss.clone(), logits.clone(), {k: p.grad.clone() for k, p in model.named_parameters()},
                     {k: v.clone() for k, v in model.state_dict().items() if 'running' in k}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    st = {k: v.clone() for k, v in state0.items()}
    lo, logits_o, _, grads_o = O.train_step(batch, spec, st, None)
    for name, (loss, logits, grads, running) in (('modules', (res[0][0], res[0][1], res[0][3], res[0][4])), ('one call', runs[0])):
        assert maxrel(logits, logits_o) < 1e-4 and maxrel(loss, lo) < 1e-5, name
        # the filter network and everything behind it sharply; PointNet's convolutions sit in front of ReLU / max-pool decisions
        # (near-ties flip between two correct fp32 implementations: tests/test_gpu_baseline_parity.py has the conditioned check)
        worst = max((maxrel(grads[k], grads_o[k]), k) for k in grads if not noise_grad(k, grads_o) and k.startswith('ecc.'))
        assert worst[0] < 2e-3, (name, worst)
        worst = max((maxrel(grads[k], grads_o[k]), k) for k in grads if not noise_grad(k, grads_o))
        assert worst[0] < 2e-2, (name, worst)
        for k, v in running.items():
            assert maxrel(v.double().cpu(), st[k].double()) < 1e-5, (name, k)

