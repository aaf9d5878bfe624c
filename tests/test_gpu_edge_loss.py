"""Graph contrastive loss of the learned partition on the device (csrc/spg_edgeloss.hip, ops.EdgeGraph / edge_dist / edge_loss /
contrastive_edge_loss / connected_components / crosspartition_weights, superpoint_graph_amd.supervized_partition.losses,
partition.libply_c.connected_comp) against the REFERENCE's recorded values (tests/golden/edge_loss.npz, written by
tools/gen_edgeloss_golden.py), against the float64 restatement pinned to it (tests/edge_loss_restatement.py, pinned by
tests/test_edge_loss_restatement.py) at other sizes, and against scipy's connected components as partitions.
Bound: conftest.assert_elementwise (rtol 1e-4 + 1e-5 max|ref|); weights bit for bit.  Under dist_type 'scalar' the reference's
TVH_zhang is NaN (square root of diff = <a, b> - 1 <= 0): the device must produce NaN in the same places."""
import os
import types

import numpy as np
import pytest
import torch
# at import time: tests/test_dropin.py restores sys.modules after its shims, which would drop a scipy.sparse first imported later
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import edge_loss_restatement as R
from conftest import GOLDEN, assert_elementwise

pytestmark = pytest.mark.gpu
LOSSES = ['tv_zhang', 'tv_TVminus', 'laplacian_zhang', 'laplacian_TVminus', 'TVH_zhang', 'TVH_TVminus']
CASES = [(name, 'euclidian') for name in LOSSES] + [('TVH_zhang', 'intrinsic'), ('TVH_zhang', 'scalar')]


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'edge_loss.npz'))


def check(a, ref, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(a), nan), f'{what}: NaN pattern differs'
    if (~nan).any():
        err = np.abs(a[~nan] - ref[~nan])
        print(f'{what}: max|d| {err.max():.3e}, max|ref| {np.abs(ref[~nan]).max():.3e}')
        assert_elementwise(torch.from_numpy(a[~nan]), ref[~nan], what=what)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ----------------------------------------------------------------------------------------------------------------------
# 1. vs the golden
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dist_type', ['euclidian', 'intrinsic', 'scalar'])
def test_distance_vs_reference(hip, golden, dist_type):
    from superpoint_graph_amd.supervized_partition import losses
    src, tgt = golden['src'].astype(np.int64), golden['tgt'].astype(np.int64)
    diff = losses.compute_dist(dev(golden['emb']), src, tgt, dist_type)
    check(diff, golden[f'diff_{dist_type}'], f'diff {dist_type}')


@pytest.mark.parametrize('name,dist_type', CASES)
def test_loss_and_gradient_vs_reference_both_paths(hip, golden, name, dist_type):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import losses
    src, tgt = golden['src'].astype(np.int64), golden['tgt'].astype(np.int64)
    E = len(src)
    trans, w = dev(golden['is_transition']), dev(golden['w_xpart'])
    args = types.SimpleNamespace(loss=name, dist_type=dist_type)
    # the reference's API, as its train() calls it (numpy indices)
    emb = dev(golden['emb']).requires_grad_(True)
    diff = losses.compute_dist(emb, src, tgt, dist_type)
    l1, l2 = losses.compute_loss(args, diff, trans, w)
    ((l1 + l2) / E * 1000).backward()
    check(diff, golden[f'diff_{dist_type}'], 'diff')
    check(torch.stack([l1, l2]), golden[f'{name}_{dist_type}_loss'], 'loss1, loss2')
    check(emb.grad, golden[f'{name}_{dist_type}_grad'], 'gradient')
    # the fused form
    g = ops.EdgeGraph(dev(src), dev(tgt), len(golden['emb']))
    emb2 = dev(golden['emb']).requires_grad_(True)
    f1, f2, fdiff = ops.contrastive_edge_loss(emb2, g, trans, w, loss=name, dist_type=dist_type)
    ((f1 + f2) / E * 1000).backward()
    check(torch.stack([f1, f2]), golden[f'{name}_{dist_type}_loss'], 'fused loss1, loss2')
    check(emb2.grad, golden[f'{name}_{dist_type}_grad'], 'fused gradient')
    assert bits_equal(fdiff, diff) and bits_equal(f1, l1) and bits_equal(f2, l2) and bits_equal(emb2.grad, emb.grad)


# ----------------------------------------------------------------------------------------------------------------------
# 2. weights
# ----------------------------------------------------------------------------------------------------------------------
def test_weights_bit_equal_to_reference(hip, golden):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import losses
    src, tgt = golden['src'].astype(np.int64), golden['tgt'].astype(np.int64)
    n = len(golden['emb'])
    pred = golden['pred_in_component']
    pred_components = [np.flatnonzero(pred == i) for i in range(int(pred.max()) + 1)]
    w = losses.compute_weights_XPART(pred_components, pred, golden['objects'], src, tgt, golden['is_transition'],
                                     float(golden['xpart_factor']), None)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), golden['w_xpart'].view(np.uint32))
    args = types.SimpleNamespace(loss_weight='crosspartition', transition_factor=int(golden['transition_factor']), k_nn_adj=5)
    emb, trans = dev(golden['emb']), dev(golden['is_transition'])
    w2, pc, pic = losses.compute_weight_loss(args, emb, dev(golden['objects']), src, tgt, trans, None, True, partition=(pred_components, pred))
    assert w2.is_cuda and np.array_equal(w2.cpu().numpy().view(np.uint32), golden['w_xpart'].view(np.uint32)) and pic is pred
    g = ops.EdgeGraph(dev(src), dev(tgt), n)
    w3, comp, k, size = ops.crosspartition_weights(g, dev(pred.astype(np.int32)), trans, float(golden['xpart_factor']), return_components=True)
    wr, comp_r, size_r = R.xpart_weights(n, src, tgt, golden['is_transition'], pred, float(golden['xpart_factor']))
    assert np.array_equal(w3.cpu().numpy().view(np.uint32), golden['w_xpart'].view(np.uint32))
    assert k == len(size_r) and np.array_equal(comp.cpu().numpy(), comp_r) and np.array_equal(size.cpu().numpy(), size_r)
    args.loss_weight = 'proportional'
    wp = losses.compute_weight_loss(args, emb, None, src, tgt, trans, None, False)
    assert np.array_equal(wp.cpu().numpy().view(np.uint32), golden['w_proportional'].view(np.uint32))
    args.loss_weight = 'none'
    assert bool((losses.compute_weight_loss(args, emb, None, src, tgt, trans, None, False) == 1).all())


# ----------------------------------------------------------------------------------------------------------------------
# 3. connected components vs scipy
# ----------------------------------------------------------------------------------------------------------------------
def scipy_components(n, src, tgt, active):
    keep = np.asarray(active) != 0
    return connected_components(coo_matrix((np.ones(int(keep.sum()), np.int8), (src[keep], tgt[keep])), shape=(n, n)), directed=False)


def check_components(n, src, tgt, active):
    from superpoint_graph_amd import ops
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    active = np.asarray(active, np.uint8)
    g = ops.EdgeGraph(dev(src), dev(tgt), n)
    comp, k, size = ops.connected_components(g, dev(active))
    comp2, k2, size2 = ops.connected_components(g, dev(active))
    assert k == k2 and torch.equal(comp, comp2) and torch.equal(size, size2)          # run to run
    comp, size = comp.cpu().numpy().astype(np.int64), size.cpu().numpy()
    ks, lab = scipy_components(n, src, tgt, active)
    assert k == ks == len(size)
    assert comp.min() == 0 and comp.max() == k - 1
    # the same partition: k distinct (ours, scipy) pairs over k labels on either side
    assert len(np.unique(comp * np.int64(ks) + lab)) == k
    assert np.array_equal(size, np.bincount(comp, minlength=k))
    first = np.full(k, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    assert np.all(np.diff(first) > 0), 'components are not numbered by ascending smallest member'
    return comp


def test_components_large_knn_like_graph(hip):
    rng = np.random.default_rng(3)
    n, k = 1_000_000, 5
    src = np.repeat(np.arange(n), k)
    tgt = np.clip(src + rng.integers(-40, 41, size=n * k), 0, n - 1)
    perm = rng.permutation(n)                                # vertex ids carry no locality
    check_components(n, perm[src], perm[tgt], rng.uniform(size=n * k) < 0.5)


def test_components_path(hip):
    n = 100_000
    comp = check_components(n, np.arange(n - 1), np.arange(1, n), np.ones(n - 1))
    assert comp.max() == 0
    rng = np.random.default_rng(4)
    perm = rng.permutation(n)                                # the same path with shuffled vertex ids, one edge cut
    active = np.ones(n - 1)
    active[n // 3] = 0
    comp = check_components(n, perm[:-1], perm[1:], active)
    assert comp.max() == 1


def test_components_degenerate_graphs(hip):
    from superpoint_graph_amd.partition import libply_c
    # isolated vertices, self loops, duplicate and antiparallel edges
    src = np.array([1, 1, 2, 5, 5, 7, 8, 8, 3])
    tgt = np.array([2, 2, 1, 5, 6, 8, 7, 7, 3])
    active = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1])
    comp = check_components(10, src, tgt, active)
    assert comp.tolist() == [0, 1, 1, 2, 3, 4, 4, 5, 5, 6]
    comp = check_components(10, src, tgt, np.zeros(9))                # no active edge at all
    assert comp.tolist() == list(range(10))
    comp = check_components(7, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))      # E = 0
    assert comp.tolist() == list(range(7))
    components, in_component = libply_c.connected_comp(10, src.astype('uint32'), tgt.astype('uint32'), active.astype('uint8'), 0)
    assert in_component.dtype == np.uint32 and in_component.tolist() == [0, 1, 1, 2, 3, 4, 4, 5, 5, 6]
    assert [c.tolist() for c in components] == [[0], [1, 2], [3], [4], [5, 6], [7, 8], [9]]


# ----------------------------------------------------------------------------------------------------------------------
# 4. training-batch scale
# ----------------------------------------------------------------------------------------------------------------------
def batch(n, k, d, seed, frac_trans=0.15):
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(n), k)
    tgt = (src + rng.integers(1, 200, size=n * k)) % n
    emb = rng.normal(size=(n, d))
    emb = (emb / np.linalg.norm(emb, axis=1, keepdims=True)).astype(np.float32)
    trans = (rng.uniform(size=n * k) < frac_trans).astype(np.uint8)
    w = np.where(trans != 0, rng.uniform(1, 60, size=n * k), 1.0).astype(np.float32)
    return emb, src, tgt, trans, w


def torch_composite(emb, src, tgt, trans, w, name, dist_type):
    """the same expressions with torch ops on the device (what a user of the package would run without these kernels)"""
    a, b = emb[src], emb[tgt]
    if dist_type == 'euclidian':
        diff = ((a - b) ** 2).sum(1)
    elif dist_type == 'intrinsic':
        diff = (torch.acos((a * b).sum(1) * 0.999) - np.arccos(0.999)) / (np.arccos(-0.999) - np.arccos(0.999)) * 3.141592
    else:
        diff = (a * b).sum(1) - 1
    intra, inter = trans == 0, trans == 1
    if 'tv' in name:
        l1 = (w[intra] * torch.sqrt(diff[intra] + 1e-10)).sum()
    elif 'laplacian' in name:
        l1 = (w[intra] * diff[intra]).sum()
    else:
        l1 = 0.2 * (w[intra] * (torch.sqrt(1 + diff[intra] / 0.2 ** 2) - 1)).sum()
    s = torch.sqrt(diff[inter] + 1e-10)
    if 'zhang' in name:
        beta = 1.0471975512 if dist_type == 'intrinsic' else 1.0
        l2 = torch.clamp(-w[inter] * s + w[inter] * beta, min=0).sum()
    else:
        l2 = (s * w[inter]).sum()
    return diff, l1, l2


@pytest.mark.parametrize('name,dist_type', [('TVH_zhang', 'euclidian'), ('tv_TVminus', 'euclidian'), ('TVH_zhang', 'intrinsic')])
def test_training_batch_scale(hip, name, dist_type):
    from superpoint_graph_amd import ops
    n, k, d = 50_000, 5, 4
    emb_h, src, tgt, trans_h, w_h = batch(n, k, d, 7)
    if dist_type == 'intrinsic':          # the generator-side condition of the golden: |<a, b>| <= 0.98 (acos amplifies beyond it)
        dot = (emb_h[src].astype(np.float64) * emb_h[tgt]).sum(1)
        w_h = np.where(np.abs(dot) > 0.98, 0.0, w_h).astype(np.float32)
    E = len(src)
    g = ops.EdgeGraph(dev(src), dev(tgt), n)
    trans, w = dev(trans_h), dev(w_h)
    grads = []
    for _ in range(2):
        emb = dev(emb_h).requires_grad_(True)
        l1, l2, diff = ops.contrastive_edge_loss(emb, g, trans, w, loss=name, dist_type=dist_type)
        ((l1 + l2) / E * 1000).backward()
        grads.append((emb.grad.clone(), l1.clone(), l2.clone(), diff.detach().clone()))
    for a, b in zip(grads[0], grads[1]):
        assert bits_equal(a, b)                                                     # run to run
    diff_r, r1, r2, g_r = R.loss_and_grad(emb_h, src, tgt, trans_h, w_h, name, dist_type, 1000.0 / E)
    check(grads[0][3], diff_r, 'diff vs float64')
    check(torch.stack([grads[0][1], grads[0][2]]), np.array([r1, r2]), 'losses vs float64')
    check(grads[0][0], g_r, 'gradient vs float64')
    emb_t = dev(emb_h).requires_grad_(True)
    dt, t1, t2 = torch_composite(emb_t, dev(src), dev(tgt), trans, w, name, dist_type)
    ((t1 + t2) / E * 1000).backward()
    check(dt, diff_r, 'torch composite diff vs float64')
    check(emb_t.grad, g_r, 'torch composite gradient vs float64')


# ----------------------------------------------------------------------------------------------------------------------
# 5. end to end through the embedder
# ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_with_local_cloud_embedder(hip):
    from oracle import validate_against_reference as V
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import pointnet
    gl = np.load(os.path.join(GOLDEN, 'local_embedder.npz'))
    model = V.make_local_model(pointnet)
    model.load_state_dict({k[7:]: torch.from_numpy(gl[k]) for k in gl.files if k.startswith('state0/')})
    clouds, cg, _ = V.local_inputs(700)
    model.cuda().train()
    emb = pointnet.LocalCloudEmbedder(types.SimpleNamespace(ptn_nfeat_stn=2, stn_as_global=1)).run_batch(model, clouds.cuda(), cg.cuda())
    assert emb.shape == (700, 4)
    emb.retain_grad()
    _, src, tgt, trans_h, w_h = batch(700, 5, 4, 9)
    g = ops.EdgeGraph(dev(src), dev(tgt), 700)
    trans, w = dev(trans_h), dev(w_h)
    l1, l2, _ = ops.contrastive_edge_loss(emb, g, trans, w)
    ((l1 + l2) / len(src) * 1000).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert float(emb.grad.abs().max()) > 0
    emb2 = emb.detach().clone().requires_grad_(True)                  # kernel (c) alone on the same g_e
    m1, m2, _ = ops.contrastive_edge_loss(emb2, g, trans, w)
    ((m1 + m2) / len(src) * 1000).backward()
    assert bits_equal(emb.grad, emb2.grad)


# ----------------------------------------------------------------------------------------------------------------------
# 6. argument handling
# ----------------------------------------------------------------------------------------------------------------------
def test_out_of_range_index_raises_and_graph_stays_usable(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.supervized_partition import losses
    src, tgt = np.array([0, 1, 2, 3]), np.array([1, 2, 3, 0])
    g = ops.EdgeGraph(dev(src), dev(tgt), 4)
    emb = dev(np.eye(4, dtype=np.float32))
    ref = ops.edge_dist(emb, g)
    for bad in (np.array([1, 2, 4, 0]), np.array([1, -1, 3, 0])):
        with pytest.raises(IndexError):
            g.build(dev(src), dev(bad))
        with pytest.raises(RuntimeError, match='build'):
            ops.edge_dist(emb, g)
        g.build(dev(src), dev(tgt))
        assert torch.equal(ops.edge_dist(emb, g), ref)
        with pytest.raises(IndexError):
            losses.compute_dist(emb, src, bad, 'euclidian')
    assert ref.tolist() == [2.0, 2.0, 2.0, 2.0]
    # a numpy pair seen twice in a row is not rebuilt
    a = losses._graph(src, tgt, 4)
    assert losses._graph(src, tgt, 4) is a and losses._graph(src.copy(), tgt, 4) is not a


def test_argument_errors(hip):
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.partition import libply_c
    from superpoint_graph_amd.supervized_partition import losses
    src, tgt = np.array([0, 1, 2]), np.array([1, 2, 0])
    emb, trans = dev(np.eye(3, 4, dtype=np.float32)), dev(np.zeros(3, np.uint8))
    args = types.SimpleNamespace(loss='TVH_zhang', dist_type='euclidian', loss_weight='crosspartition', transition_factor=5, k_nn_adj=5)
    with pytest.raises(ValueError, match='libcp is not part of this package'):
        losses.compute_weight_loss(args, emb, None, src, tgt, trans, None, False)
    args.loss_weight = 'none'
    with pytest.raises(ValueError, match='libcp is not part of this package'):
        losses.compute_weight_loss(args, emb, None, src, tgt, trans, None, True)
    args.loss_weight = 'seal'
    with pytest.raises(NotImplementedError):
        losses.compute_weight_loss(args, emb, None, src, tgt, trans, None, False)
    with pytest.raises(NotImplementedError):
        libply_c.connected_comp(3, src, tgt, np.ones(3, np.uint8), 5)
    with pytest.raises(ValueError, match='unknown argument of parameter --dist_type'):
        losses.compute_dist(emb, src, tgt, 'cosine')
    with pytest.raises(ValueError, match='unknown argument of parameter --loss'):
        losses.compute_loss(types.SimpleNamespace(loss='huber', dist_type='euclidian'), dev(np.zeros(3, np.float32)), trans, dev(np.ones(3, np.float32)))
    g = ops.EdgeGraph(dev(src), dev(tgt), 3)
    with pytest.raises(ValueError, match='d <= 64'):
        ops.edge_dist(dev(np.zeros((3, 65), np.float32)), g)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.edge_dist(torch.zeros(3, 4), g)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.connected_components(g, torch.ones(3, dtype=torch.uint8))


@pytest.mark.parametrize('d', [1, 3, 64])
def test_other_widths_and_no_transition_edge(hip, d):
    from superpoint_graph_amd import ops
    n, k = 3000, 5
    emb_h, src, tgt, trans_h, w_h = batch(n, k, d, 11 + d, frac_trans=0.0)
    if d == 1:
        emb_h = np.random.default_rng(1).normal(size=(n, 1)).astype(np.float32)
    assert not trans_h.any()
    E = len(src)
    g = ops.EdgeGraph(dev(src), dev(tgt), n)
    emb = dev(emb_h).requires_grad_(True)
    l1, l2, diff = ops.contrastive_edge_loss(emb, g, dev(trans_h), dev(w_h), loss='tv_zhang')
    assert float(l2.detach()) == 0.0
    (l2 * 1000).backward(retain_graph=True)
    assert float(emb.grad.abs().max()) == 0.0                       # nothing arrives from loss2
    emb.grad = None
    ((l1 + l2) / E * 1000).backward()
    diff_r, r1, r2, g_r = R.loss_and_grad(emb_h, src, tgt, trans_h, w_h, 'tv_zhang', 'euclidian', 1000.0 / E)
    check(diff, diff_r, 'diff')
    check(torch.stack([l1, l2]), np.array([r1, r2]), 'losses')
    check(emb.grad, g_r, 'gradient')
