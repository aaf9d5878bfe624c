"""Device cut pursuit (csrc/spg_cutpursuit.hip, ops.min_cut, ops.cut_pursuit, partition/libcp.py, compute_partition) against the
numpy restatement (cutpursuit_restatement.py): labels and partitions exactly, values and energies within 1e-11 relative (float64
sums of n <= 10^4 terms in another order: n 2^-53 with an order of magnitude to spare).

Pulse counts on the device equal the restatement's (the heights are double-buffered, so they do not depend on scheduling):
path300 needs 300, the largest of these cases."""
import types

import numpy as np
import pytest
import torch

import cutpursuit_cases as CASES
import cutpursuit_restatement as R
from superpoint_graph_amd import ops
from superpoint_graph_amd.partition import libcp
from superpoint_graph_amd.supervized_partition import losses

pytestmark = pytest.mark.gpu

MINCUT = CASES.mincut_cases()
SOLVER = CASES.solver_cases()
_REF = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(c):
    return ops.EdgeGraph(dev(np.asarray(c['src'], np.int64)), dev(np.asarray(c['tgt'], np.int64)), int(c['n'] if 'n' in c else len(c['obs'])))


def _ref_solver(name):
    if name not in _REF:
        c, stats = SOLVER[name], {}
        _REF[name] = R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], c['m'], stats=stats, **c['kw']) + (stats,)
    return _REF[name]


@pytest.mark.parametrize('name', sorted(MINCUT))
def test_min_cut_equals_restatement(name):
    c = MINCUT[name]
    want, pulses = R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])
    label, info = ops.min_cut(_graph(c), dev(c['cap']), dev(c['cost0']), dev(c['cost1']), return_info=True)
    assert label.dtype == torch.uint8 and np.array_equal(label.cpu().numpy(), want)
    assert info['pulses'] == pulses
    assert 8 * pulses <= ops.MINCUT_MAX_PULSES


def test_min_cut_pulse_cap_raises_and_returns():
    c = MINCUT['path300']
    g = _graph(c)
    with pytest.raises(RuntimeError, match='max_pulses = 5'):
        ops.min_cut(g, dev(c['cap']), dev(c['cost0']), dev(c['cost1']), max_pulses=5)
    want, _ = R.min_cut(c['n'], c['src'], c['tgt'], c['cap'], c['cost0'], c['cost1'])
    assert np.array_equal(ops.min_cut(g, dev(c['cap']), dev(c['cost0']), dev(c['cost1']), max_pulses=300).cpu().numpy(), want)


def test_min_cut_refuses_values_at_the_limit():
    c = MINCUT['n2']
    g = _graph(c)
    for which in ('cap', 'cost0', 'cost1'):
        bad = {k: c[k].copy() for k in ('cap', 'cost0', 'cost1')}
        bad[which][0] = 1 << 28
        with pytest.raises(ValueError, match=r'\[0, 2\^28\)'):
            ops.min_cut(g, dev(bad['cap']), dev(bad['cost0']), dev(bad['cost1']))
        bad[which][0] = -1
        with pytest.raises(ValueError, match=r'\[0, 2\^28\)'):
            ops.min_cut(g, dev(bad['cap']), dev(bad['cost0']), dev(bad['cost1']))
    with pytest.raises(ValueError, match='cap must be'):
        ops.min_cut(g, dev(np.zeros(3, np.int64)), dev(c['cost0']), dev(c['cost1']))


def test_min_cut_workspace_is_what_the_layout_takes():
    L = ops.lib()
    a256 = lambda b: (b + 255) // 256 * 256
    for n, E in ((1, 0), (65, 300), (1000, 4097)):
        want = 256 + 2 * a256(8 * E) + 4 * a256(4 * n) + a256(8 * n)
        assert L.spg_mincut_workspace_bytes(n, E) == want


@pytest.mark.parametrize('name', sorted(SOLVER))
def test_cut_pursuit_equals_restatement(name):
    c = SOLVER[name]
    comp_w, ncom_w, values_w, energies_w, stats_w = _ref_solver(name)
    g = _graph(c)
    comp, ncom, values, energies, stats = ops.cut_pursuit(dev(c['obs']), g, dev(c['w']), None if c['m'] is None else dev(c['m']),
                                                          return_stats=True, **c['kw'])
    assert comp.dtype == torch.int32 and ncom == ncom_w and np.array_equal(comp.cpu().numpy(), comp_w)
    assert stats['pulses'] == stats_w['pulses'] and stats['merge_rounds'] == stats_w['merge_rounds']
    assert values.dtype == torch.float32 and values.shape == values_w.shape
    v, vw = values.cpu().numpy().astype(np.float64), values_w.astype(np.float64)
    print(name, 'ncom', ncom, 'pulses', stats['pulses'], 'energies', energies, energies_w, 'values max|d|', np.abs(v - vw).max())
    assert np.all(np.abs(v - vw) <= 1e-11 * np.abs(vw))
    assert len(energies) == len(energies_w)
    assert all(abs(a - b) <= 1e-11 * abs(b) for a, b in zip(energies, energies_w))


def test_cut_pursuit_refusals_name_the_limit():
    c = SOLVER['planted_D1']
    g = _graph(c)
    n, E = len(c['obs']), len(c['src'])
    w, obs = dev(c['w']), dev(c['obs'])
    with pytest.raises(ValueError, match='D <= 32'):
        ops.cut_pursuit(torch.zeros(n, 33, device='cuda'), g, w, reg_strength=0.1)
    neg = c['w'].copy(); neg[3] = -1.0
    with pytest.raises(ValueError, match='edge_weight >= 0'):
        ops.cut_pursuit(obs, g, dev(neg), reg_strength=0.1)
    m = np.ones(n, np.float32); m[5] = -0.5
    with pytest.raises(ValueError, match='node_weight >= 0'):
        ops.cut_pursuit(obs, g, w, dev(m), reg_strength=0.1)
    for bad in (np.nan, np.inf):
        o = c['obs'].copy(); o[7, 0] = bad
        with pytest.raises(ValueError, match='NaN or infinity'):
            ops.cut_pursuit(dev(o), g, w, reg_strength=0.1)
        ww = c['w'].copy(); ww[0] = bad
        with pytest.raises(ValueError, match='NaN or infinity'):
            ops.cut_pursuit(obs, g, dev(ww), reg_strength=0.1)
    with pytest.raises(TypeError, match='reg_strength'):
        ops.cut_pursuit(obs, g, w)
    with pytest.raises(RuntimeError, match='GPU'):
        ops.cut_pursuit(torch.from_numpy(c['obs']), g, w, reg_strength=0.1)


def test_libcp_interface():
    c = SOLVER['planted_weighted']
    comp_w, ncom_w, values_w, _, _ = _ref_solver('planted_weighted')
    kw = c['kw']
    solution, in_component = libcp.cutpursuit2(c['obs'], c['src'].astype('uint32'), c['tgt'].astype('uint32'), c['w'], c['m'],
                                               kw['reg_strength'], cutoff=0, spatial=1)
    assert isinstance(solution, np.ndarray) and solution.dtype == np.float32 and solution.shape == c['obs'].shape
    assert in_component.dtype == np.uint32 and np.array_equal(in_component, comp_w)
    assert np.allclose(solution, values_w[comp_w], rtol=1e-11, atol=0)
    # cutpursuit: unit node weights
    want = R.cut_pursuit(c['obs'], c['src'], c['tgt'], c['w'], None, reg_strength=kw['reg_strength'], cutoff=10, weight_decay=0.7)
    components, in_component = libcp.cutpursuit(c['obs'], c['src'].astype('uint32'), c['tgt'].astype('uint32'), c['w'], kw['reg_strength'],
                                                cutoff=10, weight_decay=0.7)
    assert in_component.dtype == np.uint32 and np.array_equal(in_component, want[0]) and len(components) == want[1]
    for k, members in enumerate(components):
        assert np.array_equal(members, np.nonzero(want[0] == k)[0])
    comps_d, inc_d = libcp.cutpursuit(dev(c['obs']), dev(c['src']), dev(c['tgt']), dev(c['w']), kw['reg_strength'], cutoff=10,
                                      weight_decay=0.7, device=True)
    assert inc_d.is_cuda and np.array_equal(inc_d.cpu().numpy(), want[0])
    assert all(a.is_cuda and np.array_equal(a.cpu().numpy(), b) for a, b in zip(comps_d, components))


def _batch():
    """a small learned-partition batch: embeddings on the unit sphere around four planted directions, a kNN-like grid graph"""
    obs, src, tgt, planted = CASES.planted_grid(16, 4, 0.05, seed=9)
    emb = obs / np.linalg.norm(obs + 1e-3, axis=1, keepdims=True)
    emb = emb.astype(np.float32)
    xyz = np.stack(np.divmod(np.arange(256), 16) + (np.zeros(256, np.int64),), 1).astype(np.float32)
    is_transition = planted[src] != planted[tgt]
    return emb, xyz, src, tgt, planted, is_transition


@pytest.mark.parametrize('threshold,spatial', [(0.0, 0.0), (0.5, 0.0), (-0.5, 0.02)])
def test_compute_partition_and_weight_loss_on_the_device(threshold, spatial):
    emb, xyz, src, tgt, planted, is_transition = _batch()
    args = types.SimpleNamespace(loss_weight='crosspartition', transition_factor=5, k_nn_adj=5, reg_strength=0.8, CP_cutoff=10,
                                 spatial_emb=spatial, edge_weight_threshold=threshold, dist_type='euclidian', loss='TVH_zhang')
    emb_d = dev(emb)
    diff = losses.compute_dist(emb_d, src, tgt, 'euclidian')
    # the restatement on the reference's inputs (losses.py:67-84)
    d = diff.cpu().numpy()
    w = np.ones(len(src), np.float32)
    if threshold > 0:
        w[d > 1] = threshold
    if threshold < 0:
        w = torch.exp(diff * threshold).cpu().numpy() / np.float32(np.exp(threshold))
    ver = emb if spatial <= 0 else np.hstack([emb, (np.float32(spatial) * xyz).astype(np.float32)])
    want = R.cut_pursuit(ver, src, tgt, w, None, reg_strength=args.reg_strength / (4 * args.k_nn_adj), cutoff=10, weight_decay=0.7)
    components, in_component = losses.compute_partition(args, emb_d, src, tgt, diff, xyz)
    assert np.array_equal(in_component, want[0]) and len(components) == want[1] and want[1] >= 2
    tr = dev(is_transition.astype(np.uint8))
    weights, pc, pic = losses.compute_weight_loss(args, emb_d, dev(planted), src, tgt, tr, diff, True, xyz=xyz, partition='device')
    assert np.array_equal(pic.cpu().numpy(), want[0]) and len(pc) == want[1]
    g = ops.EdgeGraph(dev(src), dev(tgt), len(emb))
    ref_w = ops.crosspartition_weights(g, dev(want[0]), tr, args.transition_factor * 2 * args.k_nn_adj)
    assert torch.equal(weights, ref_w) and float(weights.max()) > 1.0
    # without a partition the refusal is what it was
    with pytest.raises(ValueError, match='libcp is not part of this package'):
        losses.compute_weight_loss(args, emb_d, dev(planted), src, tgt, tr, diff, False, xyz=xyz)
    with pytest.raises(ValueError, match="'device'"):
        losses.compute_weight_loss(args, emb_d, dev(planted), src, tgt, tr, diff, False, xyz=xyz, partition='host')
