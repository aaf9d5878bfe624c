"""CPU side of the filter-network layer suite (tests/fnet_cases.py; the device runs in tests/test_gpu_fnet_layers.py):

* the restated module with every knob off IS oracle.spg_oracle.graph_network_forward / fnet_forward: output and every gradient in
  float64 BIT FOR BIT, with its own decisions and with forced ones, in training and in evaluation mode;
* launch_form()'s constants against the headers, its predicates against a table written out by hand from their source, every case
  listed under the tokens it is there to reach, and the case list reaches every form the predicates can give (the unreachable ones are
  named with the reason);
* the float32 CPU stand-in for the device goes through the very check functions the GPU test calls and stays within ADMIT = 0.25 of
  every bound on every case (the admission), the decision cap included;
* every knob (one plausible kernel mistake each), planted in the stand-in, fails the named check on the named case."""
import pytest
import torch

import fnet_cases as C
from oracle import spg_oracle as O

CASES = {c['name']: c for c in C.cases()}


# ---------------------------------------------------------------------------------------------------------------------
# the restated module is the oracle's
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(case, built, training, dec=None):
    spec = C.oracle_spec(case)
    pk = set(C.param_keys(case))
    P = {k: (v.double().clone().requires_grad_(training) if k in pk else v.double().clone()) for k, v in built['state'].items()}
    x = built['x'].double().clone().requires_grad_(training)
    out = O.graph_network_forward(x, built['ef'].double(), built['idxn'], built['degs'], spec, P, training, dec=dec)
    res = {'out': out.detach()}
    if training:
        out.backward(built['go'].double())
        res['grad x'] = x.grad
        res.update({'grad ' + k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in pk})
    return res


@pytest.mark.parametrize('name', ['E33', 'E2 bn0', 'ef1 [24 40]', '[13 160] bn0', 'no hidden ef13 llbias', 'matrix nc8', 'llbias no bn E64', 'edge gamma signs'])
def test_all_knobs_off_is_the_oracle_bit_for_bit(name):
    case = CASES[name]
    built = C.build(case)
    dec = C.decisions(case, C.evaluate(case, built, torch.float32))
    for d in (None, dec):
        want, got = _oracle(case, built, True, d), C.evaluate(case, built, torch.float64, dec=d)
        for k, v in want.items():
            if k.startswith('grad ') and any(k == 'grad ' + l['lin'] + '.bias' for l in C.layers_of(case) if l['bn']):
                continue      # (evaluate writes the exact zero the library writes for the bias in front of the BatchNorm)
            assert torch.equal(got[k], v), (name, k)
    want, got = _oracle(case, built, False), C.evaluate(case, built, torch.float64, training=False)
    assert torch.equal(got['out'], want['out'])
    P64 = {k: v.double() for k, v in built['state'].items()}
    assert torch.equal(got['filters'], O.fnet_forward(built['ef'].double(), C.oracle_spec(case), C.nout(case), P64, False, None, 'ecc.0._fnet'))


def test_the_case_graphs():
    for E in sorted({c['E'] for c in CASES.values()}):
        idxn, degs = C.graph_of(E)
        n = int(degs.numel())
        assert int(degs.sum()) == E == idxn.numel() and int(degs.max()) <= 8 and int(degs.max()) - int(degs.min()) <= 1
        dst = torch.repeat_interleave(torch.arange(n), degs)
        assert bool((idxn != dst).all()) and len({(int(a), int(b)) for a, b in zip(idxn, dst)}) == E      # no self-loop, no repeated edge
        if E >= n:
            assert len(set(idxn.tolist())) == n      # every node has an out-edge


# ---------------------------------------------------------------------------------------------------------------------
# launch forms
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_against_the_headers():
    assert (C.FC_ROWS, C.KC, C.MAX_LAYERS, C.FOLD_SLOTS) == (32, 32, 8, 4)
    assert (C.PRO_IDENT, C.PRO_AFFINE, C.PRO_BNBWD) == (0, 1, 3) and (C.KEY_NO_BN_FOLD, C.KEY_NO_GROUP) == (10, 11)
    src = open(C.os.path.join(C.ROOT, 'superpoint_graph_amd', 'csrc', 'spg_gemm.hip')).read()
    assert 'int target = 512 / tiles;' in src and 'launch_gemm_t<32, 128, 1, 4, WRED, AMODE>' in src      # WGRAD_TARGET, COL_TILE
    assert 'for (; k + 48 < job.nsplit; k += 64)' in src      # the stride E = 1568 / 2080 straddle (49 and 65 splits)


def test_predicates_against_a_hand_table():
    """Written out from the source of wgrad_plan, spg_launch_gemm_impl / launch_gemm_t and launch_wgrad_t, not computed."""
    plan = C.wgrad_plan
    # K <= 32: 128 x 32, one tile per 128 outputs; target 512 / tiles splits, rows rounded up to whole chunks of 32
    assert plan(2, 32, 13) == (128, 32, 32, 1) and plan(65, 128, 32) == (128, 32, 32, 3) and plan(1568, 128, 32) == (128, 32, 32, 49)
    assert plan(2080, 128, 32) == (128, 32, 32, 65) and plan(20000, 128, 32) == (128, 32, 64, 313)
    # K <= 64: 64 x 64 for N <= 64, else 128 x 64; N = 4096: 32 tiles, target 16: 513 / 16 = 33 rows -> 64
    assert plan(65, 32, 64) == (64, 64, 32, 3) and plan(65, 64, 33) == (64, 64, 32, 3) and plan(65, 1024, 64) == (128, 64, 32, 3)
    assert plan(513, 4096, 64) == (128, 64, 64, 9) and plan(544, 4096, 64) == (128, 64, 64, 9) and plan(512, 4096, 64) == (128, 64, 32, 16)
    # K > 64: 128 x 128
    assert plan(65, 64, 128) == (128, 128, 32, 3) and plan(65, 32, 160) == (128, 128, 32, 3)
    I, A, B = C.PRO_IDENT, C.PRO_AFFINE, C.PRO_BNBWD
    gf = C._gemm_form      # (wred, amode, a_ld, a_has_c0, ldw, M, N, K) -> (mode, full, row tiles, column tiles)
    assert gf(False, I, 13, False, 13, 65, 32, 13) == (-1, False, 3, 1)            # 13 floats per row: no aligned quads
    assert gf(False, I, 4, False, 4, 65, 32, 4) == (I, False, 3, 1)                # vector input, K % 32 != 0
    assert gf(False, I, 32, False, 32, 64, 160, 32) == (I, True, 2, 2)
    assert gf(False, A, 32, False, 32, 64, 128, 32) == (A, False, 2, 1)            # no BatchNorm constants: masked
    assert gf(False, A, 64, True, 64, 64, 4096, 64) == (A, True, 2, 32)
    assert gf(False, A, 40, True, 40, 33, 32, 40) == (A, False, 2, 1)
    assert gf(False, A, 30, True, 30, 33, 20, 30) == (-1, False, 2, 1)
    assert gf(True, I, 32, True, 64, 65, 64, 32) == (I, True, 3, 1) and gf(True, I, 8, True, 64, 33, 64, 8) == (I, False, 2, 1)
    assert gf(True, B, 64, True, 128, 65, 128, 64) == (B, True, 3, 1) and gf(True, B, 40, True, 24, 33, 24, 40) == (B, False, 2, 1)
    assert gf(True, I, 20, True, 30, 33, 30, 20) == (-1, False, 2, 1) and gf(True, I, 32, True, 160, 65, 160, 32) == (I, True, 3, 2)
    wf = C._wgrad_form     # (amode, bmode, b_has_c0, M, N, K) -> (IT, JT, rps, nsplit, a, b, full)
    assert wf(I, I, False, 65, 32, 13) == (128, 32, 32, 3, -1, -1, False)
    assert wf(I, I, False, 64, 128, 32) == (128, 32, 32, 2, I, I, True) and wf(I, I, False, 64, 32, 32) == (128, 32, 32, 2, I, I, False)
    assert wf(I, A, True, 64, 128, 32) == (128, 32, 32, 2, I, A, True) and wf(I, A, False, 64, 128, 32) == (128, 32, 32, 2, I, A, False)
    assert wf(I, A, True, 65, 128, 32) == (128, 32, 32, 3, I, A, False)            # a ragged row count is never `full`
    assert wf(I, A, True, 544, 4096, 64) == (128, 64, 64, 9, I, A, True) and wf(I, A, True, 513, 4096, 64) == (128, 64, 64, 9, I, A, False)
    assert wf(I, A, True, 64, 32, 64) == (64, 64, 32, 2, I, A, False)              # the production vector head: 32 is no whole 64-row tile
    assert wf(B, I, False, 96, 128, 32) == (128, 32, 32, 3, B, I, True) and wf(B, A, False, 64, 64, 128) == (128, 128, 32, 2, B, A, False)


def test_launch_form_against_a_hand_table():
    form = lambda **kw: C.launch_form(C._case('x', kw.pop('E'), '', **kw))
    assert form(E=65) == ('slots grouped f0:gm.3x1 w0:128x32.32x3.ggm.rides f1:am.3x1 d1:iF.3x1 w1:128x32.32x3.iam.rides f2:am.3x1 d2:bF.3x1 '
                          'w2:128x128.32x3.bam.zero f3:aF.3x1 d3:iF.3x1 w3:64x64.32x3.iam.none')
    assert form(E=64, fnet=(32, 128, 64), bnidx=0, nc=32, matrix=True, llbias=1, keys={10: 1, 11: 1}) == (
        'finalize direct f0:iF.2x1 w0:128x32.32x2.biF.zero f1:aF.2x1 d1:iF.2x1 w1:128x128.32x2.iam.rides f2:am.2x8 d2:iF.2x1 w2:128x64.32x2.iam.rides')
    assert form(E=33, fnet=(13,), bnidx=-1, training=False) == 'nobn grouped f0:gm.2x1'


@pytest.mark.parametrize('name', list(CASES))
def test_case_reaches_the_forms_it_is_there_for(name):
    case = CASES[name]
    tokens = C.launch_form(case).split()
    assert set(case['reach']) <= set(tokens), set(case['reach']) - set(tokens)
    for keys in C.neutral_keys(case):      # a neutral key changes the header only
        assert C.launch_form(case, {**case['keys'], **keys}).split()[2:] == tokens[2:]


def test_the_table_reaches_every_form():
    """The kinds of launch the predicates can give for a filter network, by (operand modes, full); unreachable:
      * wgrad 'ba' + F: a BNBWD gradient operand means the layer HAS the BatchNorm, `full` with an AFFINE input operand means its
        PRODUCER has it -- create_fnet places one BatchNorm;
      * bias through spg_queue_colsum: see the module docstring of fnet_cases;
      * a BNBWD data gradient of layer 0: the first layer has none."""
    seen = {'f': set(), 'd': set(), 'w': set(), 'bias': set(), 'head': set()}
    for c in CASES.values():
        toks = C.launch_form(c).split()
        seen['head'] |= set(toks[:2])
        for t in toks[2:]:
            body = t.split(':')[1].split('.')
            if t[0] in 'fd':
                seen[t[0]].add(body[0])
            else:
                seen['w'].add(body[2]); seen['bias'].add(body[3])
    assert seen['head'] == {'slots', 'finalize', 'nobn', 'grouped', 'direct'}
    assert seen['f'] == {'gm', 'im', 'iF', 'am', 'aF'}
    assert seen['d'] == {'gm', 'im', 'iF', 'bm', 'bF'}
    assert seen['w'] == {'ggm', 'iim', 'iiF', 'iam', 'iaF', 'bam', 'bim', 'biF'}
    assert seen['bias'] == {'rides', 'zero', 'none'}
    train = [c for c in CASES.values() if c['training']]
    # the lattice of the issue
    assert {c['E'] for c in train} >= {2, 31, 32, 33, 64, 65, 96, 513, 544, 1568, 2080}
    assert {c['fnet'][0] for c in train} >= {1, 4, 13, 32, 33} and {tuple(c['fnet'][1:]) for c in train} >= {C.PROD, (24, 40), (160,), ()}
    assert {(c['matrix'], c['nc']) for c in train} >= {(False, 8), (False, 32), (False, 128), (True, 8), (True, 32), (True, 64)}
    assert {c['bnidx'] for c in train} >= {-1, 0, 1, 2} and {c['llbias'] for c in train} == {0, 1} and {c['update_times'] for c in train} == {1, 2}
    assert {c['edge'] for c in train} >= set(C.EDGES) and any(not c['training'] for c in CASES.values())
    # the splits the batched reduction's 64-stride straddles, and rows_per_split beyond one chunk with a one-row / one-chunk last split
    plans = {(c['E'],) + C.wgrad_plan(c['E'], l['cout'], l['cin'])[2:] for c in train for l in C.layers_of(c)}
    assert {(1568, 32, 49), (2080, 32, 65), (513, 64, 9), (544, 64, 9)} <= plans


# ---------------------------------------------------------------------------------------------------------------------
# admission: the float32 stand-in through the checks of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_case_is_admitted(name):
    case = CASES[name]
    built = C.build(case)
    report = []
    C.check_all(case, built, C.standin(case, built), report)      # every bound and the decision cap hold for the float32 side ...
    worst = max(report, key=lambda r: r[3])
    print(f'{name}: float32 CPU worst ratio {worst[3]:.3f} ({worst[0]} {worst[1]})')
    assert worst[3] <= C.ADMIT, f'{name}: the float32 CPU evaluation stands at {worst[3]:.3f} of the bound on {worst[0]} {worst[1]}'      # ... four times over


# ---------------------------------------------------------------------------------------------------------------------
# knobs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('knob', sorted(C.KNOBS))
def test_knob_fails_its_check_on_its_case(knob):
    switches, check, name = C.KNOBS[knob]
    case = CASES[name]
    built = C.build(case)
    with pytest.raises(AssertionError) as e:
        C.check_all(case, built, C.standin(case, built, **switches))
    assert f': {check}' in str(e.value) and str(e.value).startswith(name), (knob, str(e.value))


def test_every_knob_of_the_issue_is_listed():
    assert len(C.KNOBS) == 11 and {v[1] for v in C.KNOBS.values()} == {'raw', 'bn.mean', 'running_var', 'grad'}
    assert all(v[2] in CASES for v in C.KNOBS.values())
