"""CPU: the cases of tests/groupnorm_cases.py (GroupNorm / LayerNorm local embedder, csrc/spg_groupnorm.hip) before the device
sees them in tests/test_gpu_groupnorm_edges.py:

* every case is ADMITTED: the float32 CPU evaluation of its reference stays within 0.25 of the bound on every compared tensor.
  The float32 evaluation is torch.nn.functional.group_norm, except in the cases with one-element groups: torch's CPU kernel folds
  the mean into a per-channel shift (x * scale + (beta - mean * scale)), which leaves rstd = eps^-1/2 = 316 times a rounding
  error where (x - mean) * rstd -- the formula, and the kernel's arithmetic -- gives exactly 0; those cases are admitted with the
  formula (restate=True), their exact_zero tensors included;
* the builders reach the edges they claim: every axis value of the issue, exact ties, exact zeros, variance below eps, dead
  channels, pre-activations of exactly 0, zero rows of w;
* with all knobs off the float64 evaluators reproduce the reference project's float64 record (tests/golden/groupnorm_embedder*.npz)
  on all three models and every recorded shape;
* every knob -- one plausible kernel mistake each, evaluated in float32 on the CPU -- LEAVES the bound on at least one case, by a
  finite figure, while the unknobbed float32 evaluation of the same restatement stays inside it on all of them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import groupnorm_cases as G
from groupnorm_golden import CASES as GOLDEN_CASES, golden

F32 = torch.float32
ALL = G.cases() + G.composed_cases()


def _evaluate(case, dtype, **kw):
    return (G.composed_reference if 'stn' in case else G.gn_reference)(case, dtype, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------------------------------
def test_every_case_is_admitted():
    top = (0.0, '', '')
    for c in ALL:
        fig = G.judge(c, _evaluate(c, F32, restate=bool(c['exact_zero'])), G.reference(c))
        assert set(fig) == set(G.reference(c))
        for k, (_, r) in fig.items():
            assert r <= G.ADMIT, f"{c['name']}: {k}: float32 on the CPU is at {r:.3f} of the bound (admission: {G.ADMIT})"
            top = max(top, (r, c['name'], k))
    print('worst float32 / bound:', top)


# ---------------------------------------------------------------------------------------------------------------------
# the builders reach their edges
# ---------------------------------------------------------------------------------------------------------------------
def test_every_axis_value_is_reached():
    cs = G.cases()
    assert {1, 2, 31, 32, 33, 63, 64} <= {c['npts'] for c in cs}
    assert {1, 2, 31, 32, 33, 64, 65, 8193, 8192 + 33} <= {c['B'] for c in cs}
    assert {1, 31, 32, 33, 64, 65, 127, 128} <= {w for c in cs for w in c['conv']}
    assert {1, 33, 128} <= {w for c in cs for w in c['fc']}
    for stack in (True, False):
        cins = {cin for c in cs for (_, cin, _, _, conv) in G.layers_of(c) if conv == stack}
        assert any(v % 2 for v in cins) and any(v % 2 == 0 for v in cins)
    assert {c['nfeat'] for c in cs} >= {1, 2, 3, 6, 16} and all(not c['ext'] for c in cs if c['nfeat'] == 1)
    assert {c['nglob'] for c in cs} >= {0, 1, 7, 64}
    assert {(len(c['conv']), len(c['fc'])) for c in cs} >= {(1, 1), (2, 4), (3, 2), (8, 8)}
    assert {c['last_ac'] for c in cs} == {0, 1}
    assert {c['n_group'] for c in cs} >= {1, 2} and any(c['n_group'] > 1 and set(c['conv']) == {c['n_group']} for c in cs)
    assert {c['ext'] for c in cs} == {True, False} and {c['want_clouds'] for c in cs} == {True, False}
    assert any(not c['ext'] and not c['want_clouds'] for c in cs)          # the backward without dL/d cloud (want_x false)
    # the two large batches stay small networks; a workgroup of the backward takes a second run only there
    for c in cs:
        assert (c['B'] > G.RUN * G.MAX_GRID) == (c['B'] in (8193, 8225))
        if c['B'] > 8192:
            assert (c['conv'], c['fc'], c['npts']) == ([4, 8], [4, 2], 3)
            assert float(c['w'][8192:].abs().min(1).values.max()) > 0        # the clouds beyond the grid carry weight
    # head groups hold 8 elements or more, except where one-element groups are the point
    for c in cs:
        for name, _, cout, norm, conv in G.layers_of(c):
            if norm and not conv and cout != c['n_group']:
                assert cout // c['n_group'] >= 8 or c['B'] > 8192, (c['name'], name)      # (the issue's own network for the two large batches)


def test_value_classes():
    """Every class inside one batch (as op_cases.cell_rows mixes its rows), and what each class claims."""
    seen = set()
    for c in ALL:
        x, P = c['clouds'], c['npts']
        assert len(c['classes']) == c['B']
        seen |= set(c['classes'])
        for b, cls in enumerate(c['classes'][:130]):
            xb = x[b]
            if cls == 'identical':
                assert bool((xb == xb[:, :1]).all())
            elif cls == 'duplicate pairs' and P >= 2:
                assert torch.equal(xb[:, 1::2], xb[:, 0:2 * (P // 2):2]) and float(xb.abs().max()) > 0
            elif cls == 'zero':
                assert float(xb.abs().max()) == 0.0
            elif cls == '1e-3':
                assert 0 < float(xb.abs().max()) < 1e-2
            elif cls == '1e3':
                assert float(xb.abs().max()) > 1e2
            elif cls == 'offset 100':
                assert float(xb[:3].min()) > 90
    assert seen == set(G.VALUE_CLASSES)
    big = [c for c in G.cases() if c['B'] == 65][0]
    assert set(big['classes']) == set(G.VALUE_CLASSES)
    assert all(float(c['w'][3].abs().max()) == 0 and float(c['w'][0].abs().min()) > 0 for c in ALL if c['B'] >= 4)      # zero rows of w


def _first_layer(c, dtype=torch.float64):
    """Raw output, normalised pre-activation and activation of the first convolution [B, C, P] (no transform)."""
    P = {k: v.to(dtype) for k, v in c['params'].items()}
    y = F.conv1d(c['clouds'].to(dtype), P['conv0.weight'][:, :, None], P['conv0.bias'])
    u = F.group_norm(y, c['n_group'], P['conv0.gamma'], P['conv0.beta'], G.EPS)
    return y, u, F.relu(u)


def test_ties_zeros_small_variance_dead_channels():
    c = [c for c in G.cases() if c['name'] == 'groups 2 npts8 B65'][0]
    y, u, a = _first_layer(c)
    B, C, P = y.shape
    var = y.reshape(B, c['n_group'], -1).var(2, unbiased=False)
    mx = a.amax(2, keepdim=True)
    ties = (a == mx).sum(2)
    for b, cls in enumerate(c['classes']):
        if cls in ('1e-3', 'zero'):
            assert float(var[b].max()) < G.EPS, (b, cls, var[b])                 # layer variance below eps
        if cls == 'unit':
            assert float(var[b].min()) > 100 * G.EPS
        if cls == 'duplicate pairs':                                              # exact ties reach the arg-max, the first must win
            live = mx[b, :, 0] > 0
            assert bool(live.any()) and int(ties[b][live].min()) >= 2
            assert float((a[b, :, 0::2] - a[b, :, 1::2]).abs().max()) == 0.0
        if cls in ('identical', 'zero'):
            assert int(ties[b].min()) == P
    dead = (u[:, 3, :] < 0).all(1)                                               # beta = -5: the channel is dead at every point: a tie at 0 over the cloud
    assert float(dead.double().mean()) > 0.9 and {cls for b, cls in enumerate(c['classes']) if dead[b]} == set(G.VALUE_CLASSES)
    assert bool((a[dead][:, 3, :] == 0).all())
    assert bool((u[:, 6, :] == 0).all())                                         # gamma = beta = 0: pre-activation exactly 0
    assert float(c['params']['conv0.gamma'][2]) == 0.0 and float(c['params']['conv0.gamma'][1]) < 0
    # first of equal maxima: the evaluator's pooling is max_pool1d, values and gradient
    a = a.clone().requires_grad_(True)
    b_ = a.detach().clone().requires_grad_(True)
    G._pool(a, {}).sum().backward()
    vals, idx = F.max_pool1d(b_, P, return_indices=True)
    assert torch.equal(G._pool(a, {}).detach(), vals[:, :, 0].detach())
    first = torch.zeros_like(a).scatter_(2, (a.detach() == a.detach().amax(2, keepdim=True)).to(torch.int8).argmax(2, keepdim=True), 1.0)
    assert torch.equal(a.grad, first) and float(a.grad.sum()) == B * C


def test_declared_exceptions():
    by = {c['name']: c for c in G.cases()}
    assert all(not c['exact_zero'] and not c['noise'] for n, c in by.items()
               if n not in ('thin npts63 B2', 'groups = width npts5 B31', 'head group of 1, G4', 'head width 1', 'conv group of 1, npts1 B33'))
    assert by['thin npts63 B2']['noise'] == {'d_conv0.bias'} and not by['thin npts63 B2']['exact_zero']
    assert by['groups = width npts5 B31']['noise'] == {'d_conv0.bias', 'd_conv1.bias'}
    for n in ('head group of 1, G4', 'head width 1'):
        ref, z = G.reference(by[n]), by[n]['exact_zero']
        assert set(ref) - z == {'emb', 'd_fc0.beta', 'd_fc1.weight', 'd_fc1.bias'}, n
    c = by['conv group of 1, npts1 B33']
    assert set(G.reference(c)) - c['exact_zero'] == {'emb', 'd_glob', 'd_conv1.beta'} | {f'd_fc{j}.{p}' for j, ps in ((0, ('weight', 'bias', 'gamma', 'beta')), (1, ('weight', 'bias'))) for p in ps}
    for c in by.values():
        ref = G.reference(c)                      # (the builder's own check: the float64 reference is below 1e-12 of the largest gradient)
        for n in c['exact_zero']:
            assert float(ref[n].abs().max()) == 0.0
        live = [n for n in ref if n not in c['exact_zero'] | c['noise']]
        assert all(float(ref[n].abs().max()) > 1e-6 * G.gradient_scale(ref) for n in live), c['name']
    # a one-element group: the activation is relu(beta), whatever the cloud
    c = by['head width 1']
    P = {k: v.double() for k, v in c['params'].items()}
    want = F.linear(F.relu(P['fc0.beta'])[None], P['fc1.weight'], P['fc1.bias']).expand(c['B'], -1)
    assert G.bound_ratio(G.reference(c)['emb'], want)[1] < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the reference project's float64 record
# ---------------------------------------------------------------------------------------------------------------------
def _golden_case(tag, n, k):
    """The recorded model and inputs as a composed case."""
    g, pre = golden(tag), f'{tag}/n{n}k{k}'
    nfeat, nglob, n_group = (int(v) for v in g[f'{tag}/meta'])
    stn_w, ptn_w = (([8, 16], [8, 4]), ([16, 32], [16, 8, 4])) if tag == 'third' else (([16, 64], [32, 16]), ([32, 128], [34, 32, 32, 4]))
    stn = dict(nfeat=2, nglob=0, conv=stn_w[0], fc=stn_w[1] + [4], n_group=n_group, last_ac=0)
    ptn = dict(nfeat=nfeat, nglob=nglob, conv=ptn_w[0], fc=ptn_w[1], n_group=n_group, last_ac=0)
    state = {key[len(f'{tag}/state/'):]: torch.from_numpy(g[key]) for key in g.files if key.startswith(f'{tag}/state/')}
    names = {}                # record name -> case name

    def seq(net, kind, widths, pre_, normalised):
        for i in range(len(widths)):
            names[f'{net}.{pre_}.{3 * i}.weight'], names[f'{net}.{pre_}.{3 * i}.bias'] = f'{net}.{kind}{i}.weight', f'{net}.{kind}{i}.bias'
            if i < normalised:
                names[f'{net}.{pre_}.{3 * i + 1}.weight'], names[f'{net}.{pre_}.{3 * i + 1}.bias'] = f'{net}.{kind}{i}.gamma', f'{net}.{kind}{i}.beta'
    seq('stn', 'conv', stn_w[0], 'convs', 2)
    seq('stn', 'fc', stn_w[1], 'fcs', 2)
    names['stn.proj.weight'], names['stn.proj.bias'] = f'stn.fc{len(stn_w[1])}.weight', f'stn.fc{len(stn_w[1])}.bias'
    seq('ptn', 'conv', ptn_w[0], 'convs', 2)
    seq('ptn', 'fc', ptn_w[1], 'fcs', len(ptn_w[1]) - 1)
    assert set(names) == set(state)
    params = {names[key]: v.reshape(v.shape[0], -1) if v.dim() == 3 else v for key, v in state.items()}
    case = dict(name=pre, B=n, npts=k, stn=stn, ptn=ptn, params=params, clouds=torch.from_numpy(g[f'{pre}/clouds']),
                glob=torch.from_numpy(g[f'{pre}/clouds_global']), w=torch.from_numpy(g[f'{pre}/w']))
    record = {'emb': torch.from_numpy(g[f'{pre}/emb'])}
    for key in g.files:
        if key.startswith(f'{pre}/grad/'):
            nm = key[len(pre) + 6:]
            record['d_clouds' if nm == 'clouds' else 'd_glob' if nm == 'clouds_global' else 'd_' + names[nm]] = torch.from_numpy(g[key])
    return case, record


@pytest.mark.parametrize('tag, n, k', [(t, n, k) for t in ('layer', 'group') for n, k in GOLDEN_CASES] + [('third', 9, 7)])
def test_float64_evaluator_reproduces_the_record(tag, n, k):
    """Within 1e-9 of the bound on every element.  The record holds its embeddings in float64 and its gradients ROUNDED ONCE to
    float32 (tools/gen_groupnorm_golden.py), so a gradient element may differ by that rounding, 2^-24 |record|, besides."""
    case, record = _golden_case(tag, n, k)
    worst = 0.0
    for restate in (False, True):
        got = G.composed_reference(case, torch.float64, restate=restate)
        assert set(got) == set(record)
        for key, rec in record.items():
            v, rounded = got[key].reshape(rec.shape), rec.dtype == F32
            assert rounded == (key != 'emb')
            rec = rec.double()
            bound = 1e-4 * rec.abs() + 1e-5 * float(rec.abs().max())
            excess = (v - rec).abs() - (2.0 ** -24 * rec.abs() + 1e-44 if rounded else 0.0)
            r = float((excess.clamp(min=0) / bound).max())
            worst = max(worst, r)
            assert r <= 1e-9, (key, restate, r)
    print(f'{tag}/n{n}k{k}: worst error / bound against the record {worst:.3e}')


# ---------------------------------------------------------------------------------------------------------------------
# altered references leave the bound
# ---------------------------------------------------------------------------------------------------------------------
def _caught(knob):
    """(largest FINITE ratio of the float32 evaluation with `knob` over the cases, the case and tensor where it occurs)."""
    top = (0.0, '', '')
    for c in ALL:
        fig = G.judge(c, _evaluate(c, F32, restate=True, **({knob: True} if knob else {})), G.reference(c))
        for k, (_, r) in fig.items():
            if np.isfinite(r) and k not in c['exact_zero'] and r > top[0]:
                top = (r, c['name'], k)
    return top


def test_restatement_inside_the_bound():
    """All knobs off: the float32 restatement is admitted like torch's own, and its float64 is the reference."""
    r, where, tensor = _caught(None)
    print('unknobbed float32 restatement: worst', f'{r:.3f}', where, tensor)
    assert r <= G.ADMIT, (r, where, tensor)
    for c in ALL:
        fig = G.judge(c, _evaluate(c, F32, restate=True), G.reference(c))
        assert all(np.isfinite(v[1]) for v in fig.values()), c['name']
        assert G.worst(G.judge(c, _evaluate(c, torch.float64, restate=True), G.reference(c))) < 1e-6, c['name']


@pytest.mark.parametrize('knob', G.KNOBS)
def test_knob_is_caught(knob):
    r, where, tensor = _caught(knob)
    print(knob, f'{r:.3g}', where, tensor)
    assert r > 1.0, f'{knob} stays inside the bound on every case: worst {r:.3f}'
