"""GPU: the GroupNorm / LayerNorm local embedder (csrc/spg_groupnorm.hip) at its shape and value edges, element by
element against the float64 references of tests/groupnorm_cases.py (whose cases tests/test_groupnorm_cases.py admits and probes
on the CPU):

* ops.gn_forward / ops.gn_backward on every case of the table: the embeddings and the gradients wrt every parameter, the clouds,
  the global features and the external transform inside conftest.assert_elementwise's default bound on EVERY element -- batches
  of 1 ... 65 clouds and 8193 / 8225 (a second run per workgroup of the backward), 1 ... 64 points, widths 1 ... 128 around the
  32-wide tiles, odd cin, 1 + 1 ... 8 + 8 layers, one and several groups, with and without transform and cloud gradient; unit,
  identical, duplicated, all-zero, 1e-3, 1e3 and offset clouds mixed in one batch, negative / zero gamma, dead channels;
* the two declared exceptions, per tensor: exact zeros behind one-element groups, the noise floor for a bias in front of
  one-channel groups;
* LocalCloudEmbedder.run_batch (STN, transform, stn_as_global, PointNet, L2 normalisation) against the composed reference;
* two runs of the B = 8193 case give the same bits; a cloud alone (B = 1) gives the bits it gives inside a batch of 65;
* the case table runs the forward and the backward with 4, 2 and 1 wavefronts per workgroup (spg_gn_debug_waves).

`python tests/test_gpu_groupnorm_edges.py` prints the measured figures (profiles/groupnorm_edges_errors.txt)."""
import ctypes
import types

import pytest
import torch

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import groupnorm_cases as G
from conftest import assert_elementwise

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = {c['name']: c for c in G.cases()}
COMPOSED = {c['name']: c for c in G.composed_cases()}


def make_cfg(case):
    from superpoint_graph_amd import ops
    return ops.make_gn_cfg(case['nfeat'], case['nglob'], case['npts'], case['conv'], case['fc'], case['n_group'], G.EPS, bool(case['last_ac']))


def device_groups(case):
    """One (weight, bias, gamma, beta, None, None) per layer, convolutions then FCs, as ops.gn_forward takes them."""
    P = {k: v.to(DEV) for k, v in case['params'].items()}
    return [(P[f'{n}.weight'], P[f'{n}.bias'], P.get(f'{n}.gamma'), P.get(f'{n}.beta'), None, None) for n, *_ in G.layers_of(case)]


def run_device(case, rows=None):
    """ops.gn_forward + ops.gn_backward with grad_emb = w -> the tensors of gn_reference.  rows: only these clouds, as their own batch."""
    from superpoint_graph_amd import ops
    pick = (lambda v: v) if rows is None else (lambda v: v[rows].contiguous())
    groups = device_groups(case)
    clouds = pick(case['clouds']).to(DEV)
    glob = pick(case['glob']).to(DEV) if case['nglob'] else None
    T = pick(case['T']).to(DEV) if case['ext'] else None
    cfg = make_cfg(case)
    emb, state = ops.gn_forward(cfg, clouds, glob, groups, ext_transform=T)
    gg, g_T, g_glob, g_clouds = ops.gn_backward(state, groups, pick(case['w']).to(DEV), want_clouds=case['want_clouds'])
    torch.cuda.synchronize()
    assert (g_clouds is not None) == case['want_clouds'] and (g_T is not None) == case['ext'] and (g_glob is not None) == bool(case['nglob'])
    res = {'emb': emb}
    if g_clouds is not None:
        res['d_clouds'] = g_clouds
    if g_glob is not None:
        res['d_glob'] = g_glob
    if g_T is not None:
        res['d_T'] = g_T
    for (n, *_), row in zip(G.layers_of(case), gg):
        for p, g in zip(('weight', 'bias', 'gamma', 'beta'), row):
            if g is not None:
                res[f'd_{n}.{p}'] = g
    return {k: v.detach().cpu() for k, v in res.items()}


def run_composed(case):
    """LocalCloudEmbedder.run_batch on the product classes holding the case's parameters -> the tensors of composed_reference."""
    from superpoint_graph_amd.learning import pointnet
    stn, ptn = case['stn'], case['ptn']
    norm = dict(norm='group', n_group=case['n_group'])
    model = torch.nn.Module()
    model.stn = pointnet.STNkD(2, stn['conv'], stn['fc'][:-1], **norm)
    model.ptn = pointnet.PointNet(ptn['conv'], ptn['fc'], [], [], ptn['nfeat'], 0, prelast_do=0, nfeat_global=ptn['nglob'], **norm)
    named = {}
    for net, mod in (('stn', model.stn), ('ptn', model.ptn)):
        groups = mod.layer_groups()
        assert len(groups) == len(G.layers_of(case[net]))
        for (n, *_), (lin, gn) in zip(G.layers_of(case[net]), groups):
            named[f'{net}.{n}.weight'], named[f'{net}.{n}.bias'] = lin.weight, lin.bias
            if gn is not None:
                named[f'{net}.{n}.gamma'], named[f'{net}.{n}.beta'] = gn.weight, gn.bias
    assert set(named) == set(case['params'])
    with torch.no_grad():
        for k, p in named.items():
            p.copy_(case['params'][k].reshape(p.shape))
    model = model.to(DEV).train()
    clouds, glob = case['clouds'].to(DEV).requires_grad_(True), case['glob'].to(DEV).requires_grad_(True)
    emb = pointnet.LocalCloudEmbedder(types.SimpleNamespace(ptn_nfeat_stn=2, stn_as_global=1)).run_batch(model, clouds, glob)
    (emb * case['w'].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    res = {'emb': emb, 'd_clouds': clouds.grad, 'd_glob': glob.grad}
    res.update({'d_' + k: p.grad.reshape(case['params'][k].shape) for k, p in named.items()})
    return {k: v.detach().cpu() for k, v in res.items()}


def check(case, got):
    """Prints each figure, then asserts the bound -- or the declared exception -- on every tensor of the case."""
    ref = G.reference(case)
    name = case['name']
    assert set(got) == set(ref), (name, set(got) ^ set(ref))
    for k, (err, ratio) in G.judge(case, got, ref).items():
        rule = 'exact zero' if k in case['exact_zero'] else 'noise floor' if k in case['noise'] else 'bound'
        print(f'{name}: {k}: worst error {err:.3e}, {ratio:.3f} of the {rule}')
    floor = G.NOISE_FLOOR * G.gradient_scale(ref)
    for k, r in ref.items():
        assert bool(torch.isfinite(got[k]).all()), f'{name}: {k} is not finite'
        if k in case['exact_zero']:
            assert got[k].shape == r.shape and float(got[k].abs().max()) == 0.0, f'{name}: {k} must be exactly zero (one-element groups)'
        elif k in case['noise']:
            assert got[k].shape == r.shape and float(got[k].abs().max()) <= floor, f'{name}: {k} is above the noise floor {floor:.3e}'
        else:
            assert_elementwise(got[k], r, what=f'{name}: {k}')


@pytest.mark.parametrize('name', list(CASES))
def test_edges(hip, name):
    check(CASES[name], run_device(CASES[name]))


@pytest.mark.parametrize('name', list(COMPOSED))
def test_composed_run_batch(hip, name):
    case = COMPOSED[name]
    assert 'duplicate pairs' in case['classes'] and 'identical' in case['classes']
    check(case, run_composed(case))


def test_large_batch_bit_identical(hip):
    """B = 8193: workgroup 0 of the backward adds a second run into the slot it has already written; two runs, the same bits."""
    case = CASES['small B8193']
    a, b = run_device(case), run_device(case)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_alone_equals_in_batch(hip):
    """One cloud of each value class of the B = 65 case alone (B = 1, nr < NW) gives the embedding it gives inside the batch, bit for bit."""
    case = CASES['groups 2 npts8 B65']
    full = run_device(case)['emb']
    for cls in G.VALUE_CLASSES:
        b = [i for i, c in enumerate(case['classes']) if c == cls][-1]      # (the last one of the class: rows 58 ... 64, the one-cloud third run included)
        alone = run_device(case, rows=[b])['emb']
        assert torch.equal(alone[0].view(torch.int32), full[b].view(torch.int32)), (cls, b)


def waves(hip, case, backward):
    return hip.spg_gn_debug_waves(ctypes.byref(make_cfg(case)), int(backward))


def test_wave_layouts(hip):
    """gn_plan picks NW in {4, 2, 1} from the LDS layout, separately for the two passes: the table runs every one of them."""
    fwd = {c['name']: waves(hip, c, False) for c in CASES.values()}
    bwd = {c['name']: waves(hip, c, True) for c in CASES.values()}
    print('forward NW:', fwd)
    print('backward NW:', bwd)
    assert set(fwd.values()) == {4, 2, 1} and set(bwd.values()) == {4, 2, 1}
    assert (bwd['default npts16 B33'], bwd['default npts33 B31'], bwd['default npts64 B2']) == (4, 2, 1)
    assert (fwd['wide npts64 B5'], bwd['wide npts64 B5']) == (1, 1)
    assert fwd['1+1 npts2 B1'] == 4          # one cloud for four waves: nr < NW


# ---------------------------------------------------------------------------------------------------------------------
# the measured figures, as a table
# ---------------------------------------------------------------------------------------------------------------------
def report():
    from superpoint_graph_amd import _lib
    hip = _lib.lib()
    lines = ['# python tests/test_gpu_groupnorm_edges.py',
             '# per case and tensor: worst |device - float64 reference|, worst error / allowance of the device, the same ratio of the float32',
             '# CPU evaluation of the reference.  allowance = 1e-4 |ref| + 1e-5 max|ref| per element (conftest.assert_elementwise); rule',
             '# "zero": the tensor must be exactly zero (ratio 0 or inf); rule "noise": max|value| against 1e-5 of the largest gradient.',
             f"{'case':30s} {'NW f/b':>6s} {'tensor':22s} {'rule':5s} {'abs error':>10s} {'device':>8s} {'cpu f32':>8s}"]
    top = (0.0, '', '')
    for case in list(CASES.values()) + list(COMPOSED.values()):
        composed = 'stn' in case
        got = run_composed(case) if composed else run_device(case)
        ref = G.reference(case)
        cpu = (G.composed_reference if composed else G.gn_reference)(case, torch.float32, restate=bool(case['exact_zero']))
        dev_f, cpu_f = G.judge(case, got, ref), G.judge(case, cpu, ref)
        nw = 'n/a' if composed else f'{waves(hip, case, False)}/{waves(hip, case, True)}'
        for k in ref:
            rule = 'zero' if k in case['exact_zero'] else 'noise' if k in case['noise'] else 'bound'
            lines.append(f"{case['name']:30s} {nw:>6s} {k:22s} {rule:5s} {dev_f[k][0]:10.3e} {dev_f[k][1]:8.3f} {cpu_f[k][1]:8.3f}")
            top = max(top, (dev_f[k][1], case['name'], k))
    lines += ['', f'## worst device ratio: {top[0]:.3f}  {top[1]}: {top[2]}']
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
