"""CPU side of the PointNet layer suite (tests/pointnet_cases.py; the device runs in tests/test_gpu_pointnet_layers.py):

* the plain-torch network of the case module IS oracle.spg_oracle.pointnet_forward: values and every gradient in float64, with its
  own decisions and with forced ones;
* launch_form() against a table of shapes written out by hand from the predicates' source (spg_narrow.hip, spg_gemm.hip,
  spg_dense.h, spg_convstack.hip), and every case listed under the form the predicates give;
* a float32 CPU evaluation standing in for the device meets every bound of the forward, the decision caps and every bound of the
  backward, on every case;
* planted faults in that stand-in each fail the check that is there to catch them."""
import pytest
import torch

import pointnet_cases as C
from oracle import spg_oracle as O

CASES = {c['name']: c for c in C.cases()}
TRAIN = [n for n, c in CASES.items() if c['mode'] == 'train']
EVAL = [n for n, c in CASES.items() if c['mode'] == 'eval']
BACKWARD = [n for n in TRAIN if not CASES[n]['ordinary']]      # (`ordinary`: no conditioning of the case data, forward checks only)


# ---------------------------------------------------------------------------------------------------------------------
# the restated network is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_grads(case, state, clouds, glob, w, dec=None):
    spec = C.oracle_spec(case)
    P = {k: v.double().clone().requires_grad_(k in set(C.param_keys(case))) for k, v in state.items()}
    gl = None if glob is None else glob.double().clone().requires_grad_(True)
    odec = None
    if dec is not None:
        odec = {('ptn.stn.pool' if k == 'stn' else 'ptn.pool'): v for k, v in dec.items() if isinstance(k, str)}
        odec.update({l['n']: dec[l['i']] for l in C.layers_of(case) if l['bn']})
    emb = O.pointnet_forward(clouds.double(), gl, spec, P, True, None, 'ptn', odec, None)
    (emb * w.double()).sum().backward()
    out = {k: P[k].grad for k in C.param_keys(case)}
    if gl is not None:
        out['d_glob'] = gl.grad
    return emb.detach(), out


@pytest.mark.parametrize('name', ['train B3 P128', 'train B3 P33 odd widths', 'train B3 P64 no stn', 'train B3 P128 nglob0', 'train B3 P128 edge a'])
def test_restated_network_is_the_oracle(name):
    case = CASES[name]
    state, clouds, glob, w = C.build(case)
    dec = C.decisions(case, C.standin_forward(case, state, clouds, glob))
    for d in (None, dec):
        emb_o, g_o = _oracle_grads(case, state, clouds, glob, w, d)
        Pm = {k: v.double() for k, v in state.items()}
        with torch.no_grad():
            emb = C.net_forward(case, Pm, clouds.double(), None if glob is None else glob.double(), True, d)
        g = C.net_grads(case, state, clouds, glob, w, torch.float64, d)
        assert float((emb - emb_o).abs().max()) <= 1e-11 * float(emb_o.abs().max())
        assert set(g) == set(g_o)
        top = max(float(v.abs().max()) for v in g_o.values())
        for k in g:
            assert float((g[k] - g_o[k].reshape(g[k].shape)).abs().max()) <= 1e-10 * top, k
    # ... and in inference mode (running statistics)
    spec = C.oracle_spec(case)
    Pm = {k: v.double() for k, v in state.items()}
    with torch.no_grad():
        a = C.net_forward(case, Pm, clouds.double(), None if glob is None else glob.double(), False)
        b = O.pointnet_forward(clouds.double(), None if glob is None else glob.double(), spec, Pm, False)
    assert float((a - b).abs().max()) <= 1e-11 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# launch forms
# ---------------------------------------------------------------------------------------------------------------------
def test_predicates_against_a_hand_table():
    """Written out from the source of the predicates, not computed."""
    np_, fcb, pair, stack = C.narrow_pair_supported, C.first_conv_bwd_supported, C.bwdpair_shape_supported, C.conv_stack_eval_supported
    assert C.GRAM_MAXF == 32 and C.FC_ROWS == 32 and C.KC == 32
    # spg_narrow_pair_supported(nfeat, c1, c2, P, M): 1 <= nfeat <= 32, both widths 64, whole blocks of 32 points, key 17 != 1
    assert np_(14, 64, 64, 128, 384, {}) and np_(1, 64, 64, 32, 64, {}) and np_(32, 64, 64, 96, 288, {}) and np_(14, 64, 64, 64, 192, {17: 2})
    assert not np_(33, 64, 64, 128, 384, {}) and not np_(0, 64, 64, 128, 384, {}) and not np_(14, 48, 64, 128, 384, {})
    assert not np_(14, 64, 128, 128, 384, {}) and not np_(14, 64, 64, 100, 300, {}) and not np_(14, 64, 64, 33, 99, {})
    assert not np_(14, 64, 64, 1, 3, {}) and not np_(14, 64, 64, 16, 48, {}) and not np_(14, 64, 64, 128, 384, {17: 1})
    assert not np_(14, 64, 64, 128, 2 ** 24, {})                    # M * 64 * 4 reaches 2^32
    # spg_first_conv_bwd_supported(nfeat, c1, P, M): 2 <= nfeat, key 17 == 0 and key 18 == 0
    assert fcb(14, 64, 128, 384, {}) and fcb(2, 64, 32, 96, {}) and fcb(32, 64, 64, 192, {})
    assert not fcb(1, 64, 128, 384, {}) and not fcb(33, 64, 128, 384, {}) and not fcb(14, 48, 128, 384, {}) and not fcb(14, 64, 50, 150, {})
    assert not fcb(14, 64, 128, 384, {17: 2}) and not fcb(14, 64, 128, 384, {17: 1}) and not fcb(14, 64, 128, 384, {18: 1})
    # spg_bwdpair_rows / the shape part of spg_bwdpair_supported(CI, CO, M, P, pooled)
    assert C.bwdpair_rows(64) == 64 and C.bwdpair_rows(128) == 32
    assert pair(64, 64, 384, 128, False, {}) and pair(64, 128, 384, 128, True, {}) and pair(128, 128, 288, 96, False, {}) and pair(128, 256, 256, 128, True, {})
    assert pair(64, 64, 64, 64, False, {}) and pair(128, 128, 32, 32, False, {}) and pair(128, 128, 96, 32, False, {})
    assert not pair(64, 64, 288, 96, False, {}) and not pair(64, 128, 96, 32, False, {}) and not pair(64, 64, 32, 32, False, {})      # M % 64
    assert not pair(128, 128, 300, 100, False, {}) and not pair(128, 128, 99, 33, False, {}) and not pair(128, 128, 3, 1, False, {})   # M % 32, M < 32
    assert not pair(128, 256, 288, 96, True, {}) and not pair(64, 128, 192, 64, True, {})                      # the pooled layer needs 128 points
    assert not pair(64, 256, 384, 128, False, {}) and not pair(256, 256, 384, 128, False, {}) and not pair(48, 80, 384, 128, False, {})
    assert not pair(128, 64, 384, 128, False, {}) and not pair(32, 64, 384, 128, False, {})
    assert not pair(64, 64, 384, 128, False, {14: 1}) and not pair(128, 256, 384, 128, True, {22: 1}) and pair(128, 128, 384, 128, False, {22: 1})
    # spg_bn_fold_allowed
    assert C.bn_fold_allowed(4 * 33, {}) and not C.bn_fold_allowed(4 * 33, {10: 1})
    # spg_conv_stack_eval_supported(cin0, couts, P): passes of 32 / 64 / 128 columns, intermediate layers of one pass
    assert stack(14, [64, 64, 128, 128, 256], 128) and stack(9, [64, 64, 128], 1) and stack(128, [32], 33)
    for last in (32, 64, 128, 160, 192, 256):
        assert stack(9, [64, 64, 128, 128, last], 33), last
    for last in (24, 48, 96, 224, 288, 320):
        assert not stack(9, [64, 64, 128, 128, last], 33), last
    assert not stack(14, [64, 96, 128, 256], 33) and not stack(9, [48, 80, 96], 64) and not stack(9, [24, 40], 64)
    assert not stack(14, [64, 160, 128], 33) and not stack(14, [64, 256, 256], 33)      # an intermediate layer is one pass
    assert not stack(129, [64], 33) and not stack(0, [64], 33) and not stack(14, [64], 129) and not stack(14, [64] * 9, 33)


def test_launch_form_against_a_hand_table():
    def form(mode, B, P, **kw):
        return C.launch_form(C._case('x', mode, B, P, None, **kw))
    assert form('train', 3, 128) == 'slots stn[nfpp] main[nfpppp]'
    assert form('train', 33, 128) == 'slots stn[nfpp] main[nfpppp]'
    assert form('train', 3, 96) == 'slots stn[nf--] main[nf--p-]'           # 288 rows: no whole tiles of 64, whole tiles of 32
    assert form('train', 3, 64) == 'slots stn[nfp-] main[nfppp-]'           # the pooled layers' pairs need 128 points
    assert form('train', 3, 32) == 'slots stn[nf--] main[nf--p-]'
    assert form('train', 2, 32) == 'slots stn[nfp-] main[nfppp-]'           # 64 rows: one tile of 64
    assert form('train', 3, 100) == 'slots stn[----] main[------]'
    assert form('train', 3, 1) == 'slots stn[----] main[------]'
    assert form('train', 3, 64, nfeat_stn=0) == 'slots main[nfppp-]'
    assert form('train', 3, 64, nfeat=9, nfeat_stn=9, widths=C.ODD) == 'slots stn[---] main[----]'
    assert form('train', 3, 128, keys={17: 1}) == 'slots stn[--pp] main[--pppp]'
    assert form('train', 3, 128, keys={17: 2}) == 'slots stn[n-pp] main[n-pppp]'
    assert form('train', 3, 128, keys={18: 1}) == 'slots stn[n-pp] main[n-pppp]'
    assert form('train', 3, 128, keys={14: 1}) == 'slots stn[nf--] main[nf----]'
    assert form('train', 3, 128, keys={22: 1}) == 'slots stn[nfpp] main[nfppp-]'
    assert form('train', 3, 128, keys={10: 1}) == 'finalize stn[----] main[------]'
    assert form('train', 3, 128, nfeat=32, nfeat_stn=2) == 'slots stn[nfpp] main[nfpppp]'
    assert form('eval', 1, 1) == 'stn[stack] main[stack]'
    assert form('eval', 2, 64, nfeat=9, nfeat_stn=9, widths=C.ODD) == 'stn[layers] main[layers]'


@pytest.mark.parametrize('name', list(CASES))
def test_case_is_listed_under_its_form(name):
    case = CASES[name]
    assert C.launch_form(case) == case['form']
    for keys in C.neutral_keys(case):
        assert C.launch_form(case, keys) == case['form']


def test_the_table_covers_what_it_is_there_for():
    forms = {c['form'] for c in CASES.values()}
    assert {'slots stn[nfpp] main[nfpppp]', 'slots stn[nf--] main[nf--p-]', 'slots stn[nfp-] main[nfppp-]', 'slots stn[----] main[------]',
            'finalize stn[----] main[------]', 'slots main[nfppp-]', 'stn[stack] main[stack]', 'stn[stack] main[layers]',
            'stn[layers] main[layers]'} <= forms
    train = [CASES[n] for n in TRAIN]
    assert {c['B'] for c in train} >= {2, 3, 5, 31, 32, 33} and {c['P'] for c in train} >= {128, 96, 64, 32, 100, 50, 33, 1}
    assert {c['nfeat'] for c in train} >= {11, 14, 16, 17, 20, C.GRAM_MAXF} and {c['nglob'] for c in train} == {0, 1, 3}
    assert any(c['update_times'] == 2 for c in train) and any(c['nfeat_stn'] == 2 for c in train)
    assert {c['form'] for c in train if c['ext']} == {'slots main[nfppp-]', 'slots main[------]'} and any(c['ext'] for c in CASES.values() if c['mode'] == 'eval')
    assert {tuple(c['keys'].items()) for c in train} >= {(), ((17, 1),), ((17, 2),), ((18, 1),), ((14, 1),), ((22, 1),), ((10, 1),)}
    ev = [CASES[n] for n in EVAL]
    assert {(c['B'], c['P']) for c in ev} >= {(b, p) for b in (1, 2, 3) for p in (1, 31, 32, 33, 64, 65, 127, 128)}
    assert {c['widths']['conv'][-1] for c in ev} >= {32, 64, 128, 160, 192, 256} and {c['nfeat'] for c in ev} >= {9, 14}
    assert {c['edge'] for c in train} >= set(C.EDGES) and {c['edge'] for c in ev} >= set(C.EDGES)
    switched = {k for c in train for keys in C.neutral_keys(c) for k in keys}      # every fallback is reached by some shape
    assert switched == {C.KEY_NO_NARROW_PAIR, C.KEY_NO_FIRST_CONV_BWD, C.KEY_NO_BWD_PAIR, C.KEY_NO_PAIR_SPLIT}


# ---------------------------------------------------------------------------------------------------------------------
# the float32 stand-in meets every bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TRAIN)
def test_standin_meets_every_forward_bound(name):
    case = CASES[name]
    state, clouds, glob, w = C.build(case)
    C.check_forward(case, state, clouds, glob, C.standin_forward(case, state, clouds, glob))


@pytest.mark.parametrize('name', BACKWARD)
def test_standin_meets_the_decision_caps_and_every_backward_bound(name):
    """The case of pointnet_cases.ILL_CONDITIONED: the tie rule and the gradient bound are recorded (and printed), everything else holds."""
    case = CASES[name]
    state, clouds, glob, w = C.build(case)
    fw = C.standin_forward(case, state, clouds, glob)
    excess = {} if name in C.ILL_CONDITIONED else None
    C.check_backward(case, state, clouds, glob, w, fw, C.standin_backward(case, state, clouds, glob, w, fw), excess=excess)
    if excess is not None:
        print(f'{name}: recorded, not asserted: {excess}')


def test_standin_constant_channel():
    """y is the bias and the mean is within 1e-6 of it in both layers (asserted inside); the FC channel (3 rows) is normalised to beta within
    rstd ulp(y).  The convolution's channel is not, with float32 block partials in the statistics (pointnet_cases.CONSTANT_XFAIL: the
    stand-in shows what the device shows); it is with exact ones."""
    case = CASES['train B3 P128 edge c']
    state, clouds, glob, _ = C.build(case)
    fw = C.standin_forward(case, state, clouds, glob)
    ratios = C.constant_channel(case, state, fw)
    assert set(ratios) == {C.EDGE_C_CONV, C.EDGE_C_FC} and ratios[C.EDGE_C_FC] <= 1.0, ratios
    print(f'float32 block partials: the convolution\'s constant channel at {ratios[C.EDGE_C_CONV]:.2f} of rstd ulp(y)')
    for l in C.layers_of(case):      # exact partial sums: mean = bias, t = beta - bias s in one rounding
        if l['w'] == C.EDGE_C_CONV:
            rec, c = fw['layers'][l['i']], C.EDGE_C_CH
            rec['mean'][c] = state[l['w'] + '.bias'][c]
            rec['t'][c] = (state[l['n'] + '.bias'][c].double() - rec['mean'][c].double() * rec['s'][c].double()).float()
    assert C.constant_channel(case, state, fw)[C.EDGE_C_CONV] <= 1.0


@pytest.mark.parametrize('name', EVAL)
def test_standin_meets_the_inference_bound(name):
    case = CASES[name]
    state, clouds, glob, _ = C.build(case)
    C.check_eval(case, state, clouds, glob, C.eval_reference(case, state, clouds, glob, torch.float32))


def test_the_33rd_feature_is_refused_by_the_table():
    """nfeat = SPG_GRAM_MAXF + 1 is outside the library's range (make_plan: nfeat <= 32): the GPU suite asserts the refusal."""
    assert C.GRAM_MAXF + 1 == 33 and not C.narrow_pair_supported(33, 64, 64, 128, 384, {})


# ---------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------
FAULT_CASES = ['train B3 P128', 'train B3 P128 edge a', 'train B3 P33 odd widths']


@pytest.mark.parametrize('fault', sorted(C.FAULTS))
def test_planted_fault_fails_its_check(fault):
    caught = []
    for name in FAULT_CASES:
        case = CASES[name]
        state, clouds, glob, w = C.build(case)
        try:
            if fault == 'wgrad_skips_last_tile':
                fw = C.standin_forward(case, state, clouds, glob)
                C.check_backward(case, state, clouds, glob, w, fw, C.standin_backward(case, state, clouds, glob, w, fw, fault))
            else:
                C.check_forward(case, state, clouds, glob, C.standin_forward(case, state, clouds, glob, fault))
        except AssertionError as e:
            assert f': {C.FAULTS[fault]}' in str(e), (fault, name, str(e))
            caught.append(name)
    assert caught, fault
