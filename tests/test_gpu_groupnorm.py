"""The GroupNorm / LayerNorm local embedder on the device (spg_groupnorm.hip) against the reference's float64
record (tools/gen_groupnorm_golden.py -> tests/golden/groupnorm_embedder*.npz).

Bounds: embeddings 2e-5 absolute, gradients 2e-4 in the max|d| / max|ref| form -- the numbers of tests/test_gpu_local.py for
the BatchNorm embedder; the reference's own float32 run is within a quarter of them on every recorded case (asserted by the
tool).  The third model is recorded with n_group = 2: with n_group = 4 its 4-wide FC layer has one-channel groups (variance
exactly 0) and the reference's float32 gradients are themselves 6.7e-4 from its float64 ones."""
import ctypes

import numpy as np
import pytest
import torch

from groupnorm_golden import ARGS, CASES, build_model, golden

pytestmark = pytest.mark.gpu
EMB_TOL, GRAD_TOL = 2e-5, 2e-4


def _grad_check(ours, ref, tol):
    """tests/test_gpu_local.py::_grad_check: gradients below 1e-5 of the largest one are compared against that floor."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    worst = 0.0
    for k, r in ref.items():
        den = float(np.abs(r).max())
        if den < 1e-5 * gmax:
            assert float(ours[k].abs().max()) <= 1e-5 * gmax, k
            continue
        err = float((ours[k].cpu().double() - torch.from_numpy(r).double()).abs().max()) / den
        print(f'  {k}: {err:.3e} (max|ref| {den:.3e})')
        worst = max(worst, err)
    print('worst gradient error (max|d| / max|ref|):', worst)
    assert worst < tol


def _inputs(tag, n, k):
    g, c = golden(tag), f'{tag}/n{n}k{k}'
    return torch.from_numpy(g[f'{c}/clouds']).cuda(), torch.from_numpy(g[f'{c}/clouds_global']).cuda(), torch.from_numpy(g[f'{c}/w']).cuda()


def _run(model, clouds, glob, w=None, embedder=None):
    """-> (embeddings, gradients by the record's names or None)."""
    from superpoint_graph_amd.learning import pointnet
    embedder = embedder or pointnet.LocalCloudEmbedder(ARGS)
    if w is None:
        with torch.no_grad():
            return embedder.run_batch(model, clouds, glob), None
    clouds, glob = clouds.clone().requires_grad_(True), glob.clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    emb = embedder.run_batch(model, clouds, glob)
    (emb * w).sum().backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    grads['clouds'], grads['clouds_global'] = clouds.grad, glob.grad
    torch.cuda.synchronize()
    return emb.detach(), grads


def _parity(tag, n, k):
    g, c = golden(tag), f'{tag}/n{n}k{k}'
    model = build_model(tag).cuda().train()
    clouds, glob, w = _inputs(tag, n, k)
    emb, grads = _run(model, clouds, glob, w)
    err = float((emb.cpu().double() - torch.from_numpy(g[f'{c}/emb'])).abs().max())
    print(f'{c}: embeddings max|d| {err:.3e}')
    assert torch.isfinite(emb).all() and err < EMB_TOL
    ref = {key[len(c) + 6:]: g[key] for key in g.files if key.startswith(f'{c}/grad/')}
    assert set(ref) == set(grads)
    _grad_check(grads, ref, GRAD_TOL)
    emb_eval, _ = _run(model.eval(), clouds, glob)
    assert torch.equal(emb_eval, emb), 'eval mode must be the same function as train mode'


@pytest.mark.parametrize('n, k', CASES)
@pytest.mark.parametrize('tag', ['layer', 'group'])
def test_golden_parity(hip, tag, n, k):
    _parity(tag, n, k)


def test_third_model(hip):
    """Other widths, nfeat = 3 (use_rgb = 0), a group of two FC channels."""
    _parity('third', 9, 7)


def test_batch_independence(hip):
    """A cloud's embedding does not depend on the rest of the batch: bit-equal alone and among noise."""
    model = build_model('layer').cuda().train()
    clouds, glob, _ = _inputs('layer', 130, 33)
    full, _ = _run(model, clouds, glob)
    keep = [0, 1, 31, 32, 77, 129]
    for i in keep:
        alone, _ = _run(model, clouds[i:i + 1].contiguous(), glob[i:i + 1].contiguous())
        assert torch.equal(alone[0], full[i]), i
    gen = torch.Generator(device='cuda').manual_seed(5)
    noisy_c = torch.randn(clouds.shape, generator=gen, device='cuda') * 3
    noisy_g = torch.rand(glob.shape, generator=gen, device='cuda')
    noisy_c[keep], noisy_g[keep] = clouds[keep], glob[keep]
    noisy, _ = _run(model, noisy_c, noisy_g)
    assert torch.equal(noisy[keep], full[keep])
    assert not torch.equal(noisy[2], full[2])


def test_no_chunking(hip):
    """Training mode: a GroupNorm batch is never split at the chunk constant."""
    from superpoint_graph_amd.learning import pointnet
    model = build_model('group').cuda().train()
    clouds, glob, w = _inputs('group', 130, 33)
    emb, grads = _run(model, clouds, glob, w)
    small = pointnet.LocalCloudEmbedder(ARGS)
    small.CHUNK = 50
    emb2, grads2 = _run(model, clouds, glob, w, embedder=small)
    assert torch.equal(emb, emb2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_determinism(hip):
    model = build_model('layer').cuda().train()
    clouds, glob, w = _inputs('layer', 130, 33)
    emb, grads = _run(model, clouds, glob, w)
    emb2, grads2 = _run(model, clouds, glob, w)
    assert torch.equal(emb, emb2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k


def test_workspace_condition(hip):
    """What a forward and a backward hold in HBM is below ONE raw layer output, up to a term independent of B."""
    from superpoint_graph_amd import ops
    B, npts = 10000, 20
    cfg = ops.make_gn_cfg(6, 11, npts, [32, 128], [34, 32, 32, 4], 1)
    total = lambda b: hip.spg_gn_workspace_bytes(ctypes.byref(cfg), b) + hip.spg_gn_bwd_workspace_bytes(ctypes.byref(cfg), b)
    assert hip.spg_gn_workspace_bytes(ctypes.byref(cfg), B) > 0 and hip.spg_gn_bwd_workspace_bytes(ctypes.byref(cfg), B) > 0
    raw_layer = B * npts * 128 * 4
    assert total(B) < raw_layer + total(1)
    assert total(B) - total(1) < raw_layer // 8      # what grows with B: statistics, pooled values, arg-max


def test_refusals(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import pointnet
    with pytest.raises(NotImplementedError, match='npts'):
        ops.make_gn_cfg(6, 11, 65, [32, 128], [34, 32, 32, 4], 1)
    with pytest.raises(NotImplementedError, match='width'):
        ops.make_gn_cfg(6, 11, 20, [32, 129], [34, 32, 32, 4], 1)
    with pytest.raises(NotImplementedError, match='n_group'):
        ops.make_gn_cfg(6, 11, 20, [32, 128], [34, 32, 32, 4], 3)
    glob = torch.rand(4, 11, device='cuda')
    ptn = pointnet.PointNet([32, 128], [34, 32, 32, 4], [], [], 6, 0, prelast_do=0, nfeat_global=11, norm='layer').cuda()
    with pytest.raises(NotImplementedError, match='npts'):
        ptn(torch.rand(4, 6, 65, device='cuda'), glob)
    inner = pointnet.PointNet([32, 128], [34, 32, 32, 4], [16, 64], [32, 16], 6, 2, prelast_do=0, nfeat_global=11, norm='layer').cuda()
    with pytest.raises(NotImplementedError, match='inner STN'):
        inner(torch.rand(4, 6, 20, device='cuda'), glob)
    mixed = pointnet.PointNet([32, 128], [34, 32, 32, 4], [], [], 6, 0, prelast_do=0, nfeat_global=11, norm='layer')
    mixed.convs[1] = torch.nn.BatchNorm1d(32)
    with pytest.raises(NotImplementedError, match='mix'):
        mixed.cuda()(torch.rand(4, 6, 20, device='cuda'), glob)
    model = build_model('layer').cuda()
    model.stn = pointnet.STNkD(2, [16, 64], [32, 16]).cuda()
    with pytest.raises(NotImplementedError, match='mix'):
        pointnet.LocalCloudEmbedder(ARGS).run_batch(model, torch.rand(4, 6, 20, device='cuda'), torch.rand(4, 7, device='cuda'))
    drop = pointnet.PointNet([32, 128], [34, 32, 32, 4], [], [], 6, 0, prelast_do=0.5, nfeat_global=11, norm='layer').cuda().train()
    with pytest.raises(NotImplementedError, match='prelast_do'):
        drop(torch.rand(4, 6, 20, device='cuda'), glob)


def test_unchanged_neighbour(hip):
    """The BatchNorm embedder gives the same bits before and after the GroupNorm kernels have run in the process."""
    from superpoint_graph_amd.learning import pointnet
    clouds, glob, w = _inputs('layer', 37, 20)

    def batchnorm_run():
        torch.manual_seed(3)
        model = torch.nn.Module()
        model.stn = pointnet.STNkD(2, [16, 64], [32, 16])
        model.ptn = pointnet.PointNet([32, 128], [34, 32, 32, 4], [], [], 6, 0, prelast_do=0, nfeat_global=11, is_res=False, last_bn=True)
        torch.nn.init.normal_(model.stn.proj.weight, std=0.1)
        return _run(model.cuda().train(), clouds, glob, w)
    emb_a, grads_a = batchnorm_run()
    _run(build_model('layer').cuda().train(), clouds, glob, w)
    emb_b, grads_b = batchnorm_run()
    assert torch.equal(emb_a, emb_b)
    for k in grads_a:      # (the BatchNorm path returns no gradient wrt the clouds)
        assert (grads_a[k] is None and grads_b[k] is None) or torch.equal(grads_a[k], grads_b[k]), k
