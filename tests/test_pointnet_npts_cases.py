"""CPU: the segment rule of PointNet above 128 points per superpoint (ops.model.pointnet_segments, the library's refusal) against its
restatement in tests/pointnet_npts_cases.py, and the admission of the scenes tests/test_gpu_pointnet_npts.py runs: on those very
scenes the float32 oracle stays far inside the tolerances the device is held to, measured against the float64 oracle."""
import ctypes

import pytest
import torch

import pointnet_cases as C
import pointnet_npts_cases as N
from conftest import maxrel, noise_grad


@pytest.mark.parametrize('npts', sorted(N.RULE_CASES))
def test_segment_rule_at_the_named_sizes(npts):
    from superpoint_graph_amd import ops
    want = N.RULE_CASES[npts]
    assert N.segments(npts) == want
    if want is None:
        with pytest.raises(NotImplementedError) as exc:
            ops.model.pointnet_segments(npts)
        msg = str(exc.value)
        assert f'npts = {npts}' in msg and '[1, 128]' in msg and '4096' in msg and 'divisor in [32, 128]' in msg, msg
    else:
        assert ops.model.pointnet_segments(npts) == want
        assert want[0] * want[1] == npts and want[0] <= 128 and (want[1] == 1 or want[0] >= 32)


def test_segment_rule_everywhere():
    """Every npts from 0 to 4200: ops.model.pointnet_segments is the restated rule, accepting and refusing."""
    from superpoint_graph_amd import ops
    for npts in range(0, 4201):
        want = N.segments(npts)
        try:
            got = ops.model.pointnet_segments(npts)
        except NotImplementedError:
            got = None
        assert got == want, (npts, got, want)


def test_the_library_refuses_what_the_rule_refuses(hip):
    """make_pointnet_cfg fills any npts in (as it always did); the library's size queries return 0 for the sizes the rule refuses and
    its message states the rule.  (ops.pointnet_forward and the modules raise NotImplementedError first: tests/test_gpu_pointnet_npts.py.)"""
    from superpoint_graph_amd import ops
    wd = C.PROD
    for npts in (131, 262, 4096, 4097):
        with pytest.raises(NotImplementedError, match='divisor in'):
            ops.model.pointnet_segments(npts)
        cfg = ops.make_pointnet_cfg(14, 14, 1, npts, wd['stn_conv'], wd['stn_fc'], wd['conv'], wd['fc'])
        assert hip.spg_pointnet_workspace_bytes(ctypes.byref(cfg), 4, 1) == 0
        assert hip.spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg), 4) == 0
        msg = hip.spg_last_error().decode()
        assert f'npts = {npts}' in msg and 'divisor in [32, 128]' in msg, msg


def test_groupnorm_pointnet_keeps_its_own_limit(hip):
    """npts = 256 is a BatchNorm size only: the GroupNorm PointNet refuses it with its own message (npts <= 64)."""
    from superpoint_graph_amd import ops
    with pytest.raises(NotImplementedError) as exc:
        ops.make_gn_cfg(6, 1, 256, [32, 64], [64, 32], 1)
    assert 'divisor' not in str(exc.value) and '64' in str(exc.value), str(exc.value)
    assert ops.make_gn_cfg(6, 1, 64, [32, 64], [64, 32], 1).net.npts == 64


def test_workspaces_account_for_the_segment_buffers(hip):
    """B superpoints of 2 x 128 points against 2 B superpoints of 128 points (the same convolution problem): the forward workspace
    differs by the cloud copy, the per-segment transforms and (value, winner) tables, less the B rows of pooled tables and FC outputs
    the second plan has on top -- up to the 256-byte alignment of its ~20 buffers.  The backward workspace grows by the per-segment
    gradient rows, winners and transform partials."""
    from superpoint_graph_amd import ops
    wd, B, nf = C.PROD, 6, 14
    def cfg(npts):
        return ops.make_pointnet_cfg(nf, nf, 1, npts, wd['stn_conv'], wd['stn_fc'], wd['conv'], wd['fc'])
    c_stn, c_main = wd['stn_conv'][-1], wd['conv'][-1]
    ld_stn, ld_main = c_stn, (c_main + 1 + 3) & ~3
    fc_rows = sum(wd['stn_fc']) + 4 + sum(wd['fc'][:-1])      # (the last FC layer writes into the caller's embeddings)
    added = B * 256 * nf + 2 * B * 4 + 2 * 2 * B * (c_stn + c_main)
    less = 2 * B * (ld_stn + ld_main) + B * fc_rows
    for training in (0, 1):
        w256 = hip.spg_pointnet_workspace_bytes(ctypes.byref(cfg(256)), B, training)
        w128 = hip.spg_pointnet_workspace_bytes(ctypes.byref(cfg(128)), 2 * B, training)
        print(f'training {training}: {w256} bytes at B = {B}, 256 points; {w128} at B = {2 * B}, 128 points; expected difference {4 * (added - less)}')
        assert w256 > 0 and abs((w256 - w128) - 4 * (added - less)) <= 20 * 256, (training, w256, w128, 4 * (added - less))
    b256 = hip.spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg(256)), B)
    b128 = hip.spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg(128)), 2 * B)
    grow = 4 * (2 * 2 * B * c_main + 2 * B * 4)      # gradient rows + winners at the wider stack, transform partials
    print(f'backward: {b256} bytes against {b128}; the segment buffers are {grow}')
    assert b256 >= grow and b256 > hip.spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg(128)), B)


@pytest.mark.parametrize('name', sorted(N.SPECS))
def test_specs_are_admitted_by_the_float32_oracle(name):
    """Forward <= 1e-5 and worst gradient <= 5e-5 (max|d| / max|ref|) between the float32 and the float64 oracle on the scene the GPU
    test uses: 1e-4 / 1e-3 on the device are then a property of the device, not of the scene."""
    _, batch, _, _ = N.case(name)
    assert int((batch['clouds_flag'] != 0).sum()) > 0 and int((batch['clouds_flag'] == 0).sum()) > 1      # too-small superpoints too
    l32, lg32, e32, g32, s32 = N.oracle_step(name)
    l64, lg64, e64, g64, s64 = N.oracle_step(name, True, torch.float64)
    fwd = max(maxrel(e32, e64), maxrel(lg32, lg64), maxrel(l32, l64))
    errs = {k: maxrel(g32[k], g64[k]) for k in g32 if not noise_grad(k, g64)}
    print(f'{name}: float32 oracle vs float64: forward {fwd:.2e}, worst gradient {max(errs.values()):.2e}')
    assert fwd <= 1e-5 and max(errs.values()) <= 5e-5, (fwd, max(errs, key=errs.get), max(errs.values()))
    for k in s64:
        if 'running' in k:
            assert maxrel(s32[k].double(), s64[k].double()) < 1e-6, k


def test_external_transform_case_is_admitted_by_float32():
    """The float32 evaluation of the external-transform case stays inside tests/test_gpu_local.py's bounds (embeddings 2e-5,
    gradients 5e-4 of the largest element) against float64 autograd."""
    case = N.ext_case()
    state, clouds, glob, w = C.build(case)
    with torch.no_grad():
        e32 = C.net_forward(case, state, clouds, glob, True)
        e64 = C.net_forward(case, {k: v.double() for k, v in state.items()}, clouds.double(), glob.double(), True)
    assert maxrel(e32, e64) <= 2e-5
    g32 = C.net_grads(case, state, clouds, glob, w, torch.float32)
    g64 = C.net_grads(case, state, clouds, glob, w, torch.float64)
    params = {k: v for k, v in g64.items() if k not in ('d_glob', 'd_T')}
    worst = max(maxrel(g32[k], g64[k]) for k in g64 if k in ('d_glob', 'd_T') or not noise_grad(k, params))
    print(f'external transform case: float32 vs float64: embeddings {maxrel(e32, e64):.2e}, worst gradient {worst:.2e}')
    assert worst <= 5e-4 and float(g64['d_T'].abs().max()) > 0 and float(g64['d_glob'].abs().max()) > 0


def test_tie_cases_hold_cross_segment_ties_in_float64():
    """The tie clouds are what they claim, before any device sees them: cloud 0's halves are equal, cloud 1's first half is its point
    128; and the helpers that restate the merge agree with argmax / argmin over the whole superpoint on them."""
    for widths in ('prod', 'odd'):
        case, state, clouds, glob = N.tie_case(widths)
        assert torch.equal(clouds[0, :, :128], clouds[0, :, 128:]) and bool((clouds[1, :, :128] == clouds[1, :, 128:129]).all())
        gm = state['ptn.convs.' + str(3 * (len(case['widths']['conv']) - 1) + 1) + '.weight']
        assert bool((gm < 0).any()) and bool((gm > 0).any()) and float(gm[0]) == 0.0 and float(gm[2]) == 0.0 and bool(torch.signbit(gm[2]))
    y = torch.randn(3, 256, 7, generator=torch.Generator().manual_seed(0)).round(decimals=1)      # (rounded: plenty of ties)
    neg = torch.tensor([True, False, False, True, False, True, False])
    y3 = y.view(3, 2, 128, 7)
    vals = torch.where(neg, y3.min(2)[0], y3.max(2)[0])
    idx = torch.where(neg, y3.argmin(2), y3.argmax(2))
    # (torch's argmax / argmin return the first extremum on the CPU)
    best, win = N.first_extremum(vals, idx, neg, 128)
    first = torch.where(neg, (y == y.min(1, keepdim=True)[0]).int().argmax(1), (y == y.max(1, keepdim=True)[0]).int().argmax(1))
    assert torch.equal(win, first) and torch.equal(best, torch.where(neg, y.min(1)[0], y.max(1)[0]))
    t = torch.arange(2 * 3 * 8.0).view(2, 3, 8)
    assert torch.equal(N.by_segments(t, 2)[1], t[0, :, 4:]) and torch.equal(N.by_segments(t, 2)[2], t[1, :, :4])
