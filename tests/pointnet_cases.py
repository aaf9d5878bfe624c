"""Cases, float64 references, bounds and launch forms for the BatchNorm PointNet (csrc/spg_gemm.hip, spg_narrow.hip,
spg_pointnet.hip, spg_convstack.hip) judged LAYER BY LAYER at its tile and dispatch edges.  Plain module (no test in it):
tests/test_pointnet_cases.py runs every check on the CPU with a float32 stand-in for the device and plants faults in it,
tests/test_gpu_pointnet_layers.py runs the device.

What a run leaves (`fw`, the same structure from the device's workspace and from `standin_forward`):
    fw['layers'][i]   y (raw output [rows, C] float32) and, behind a BatchNorm, mean / rstd / s / t [C]
    fw['stn'|'main']  pooled [B, C + nglob] (raw extremum per channel, then the global features), aidx [B, C] (int64)
    fw['running']     {BatchNorm key: (running_mean, running_var)} after the forward
    fw['emb']         [B, D]
Layer i is the i-th layer in the library's order (include/spg_hip.h): STN convolutions, STN FC layers, the STN's projection,
the convolutions, the FC layers.

Checks (each assertion message starts with the case, the layer and the NAME of the check -- the CPU test matches on the name):
  raw            every element of y against a @ W^T + b in float64, a formed in float64 from the floats the layer consumed
                 (max(y_prev * s_prev + t_prev, 0): the product of two floats is exact in float64, so the ReLU decision is the
                 run's own); bound 2 (K + 4) 2^-24 (sum_k |a_ik| |w_jk| + |b_j|): the forward error of a length-K fp32 dot product
                 in any order, + 4 for the prologue's fma and the 2 x 2 transform, x 2 for one ulp per accumulation instead of a
                 half.  conftest.assert_elementwise's defaults hold as well.
  bn.mean        |mean - mean64| <= 1e-6 rms, rms = sqrt(E[y^2]), statistics in float64 of the run's own y
  bn.rstd        |rstd / rstd64 - 1| <= 1e-6 kappa, kappa = max(1, rms / sqrt(var + eps)) (the condition number of the variance
                 under one fp32 rounding per element)
  bn.s, bn.t     s = gamma rstd and t = beta - mean s: the two bounds above propagated, plus half an ulp of the stored float
  running_mean   against the float64 update (unbiased variance, `update_times` times): 1e-6 of the terms' magnitudes
  running_var    1e-6 kappa relative
  pool.bitwise   pooled[b, c] is y[b P + aidx[b, c], c] bit for bit
  pool.extremum  ... and the maximum of y over the superpoint's rows where gamma_c >= 0 (-0.0 included: the kernels test
                 gamma < 0), the minimum where gamma_c < 0; any attaining index is admitted
  pool.global    the global-feature columns are the input bit for bit
  emb            the embedding is the last layer's y (the stand-in only: the library writes that layer's output into `emb` itself)
  decisions      (backward) a ReLU decision differs from float64's own only where |v| <= 1e-4 max|v| of the layer, at most
                 10 * 1e-4 * numel of them; a pool winner misses the float64 extremum by at most 1e-4 max|h|
  grad           every element of every gradient against the float64 backward WITH the run's decisions, assert_elementwise
                 defaults; tensors conftest.noise_grad names stay below 1e-5
  constant       (edge c) a channel with an all-zero weight row normalises to beta within rstd ulp(y)
Nothing here is derived from what the device returns.  One figure is an expected failure on the device, with its cause: CONSTANT_XFAIL
below.  Cases marked `ordinary` carry no conditioning of their data and run the forward checks only.

Case data: a BatchNorm over fewer than 32 rows gets small weights (build: FEW_ROWS_SCALE), so that eps bounds |y| / sqrt(var + eps) in
every channel -- otherwise a channel whose few rows lie close together makes the gradients ill-conditioned for any fp32 arithmetic."""
import os
import re
import zlib

import torch
import torch.nn.functional as F

from conftest import ROOT, assert_elementwise, noise_grad

EPS, MOMENTUM = 1e-5, 0.1
U24 = 2.0 ** -24
FEW_ROWS_SCALE = 0.01
TIE = 1e-4                      # tests/test_gpu_baseline_parity.py::_decision_conditioned
PROD = dict(conv=(64, 64, 128, 128, 256), fc=(256, 64, 32), stn_conv=(64, 64, 128), stn_fc=(128, 64))      # oracle.ModelSpec()
ODD = dict(conv=(48, 80, 96), fc=(96, 40, 32), stn_conv=(24, 40), stn_fc=(40, 20))      # test_gpu_model._ODD_SPECS['p64_odd_widths']


def _define(header, name):
    text = open(os.path.join(ROOT, 'superpoint_graph_amd', 'csrc', header)).read()
    return int(re.search(r'#define\s+' + name + r'\s+(\d+)', text).group(1))


GRAM_MAXF = _define('spg_narrow.h', 'SPG_GRAM_MAXF')
FC_ROWS = _define('spg_gemm.h', 'SPG_FC_ROWS')
KC = _define('spg_common.h', 'SPG_KC')
NP_C = 64                       # spg_narrow.hip: SPG_NP_C
CS_KMAX, CS_MAX_LAYERS = 128, 8  # spg_convstack.hip, spg_gemm.h: SPG_CONVSTACK_MAX_LAYERS
KEY_NO_BN_FOLD, KEY_NO_BWD_PAIR, KEY_NO_NARROW_PAIR, KEY_NO_FIRST_CONV_BWD, KEY_NO_PAIR_SPLIT = 10, 14, 17, 18, 22      # spg_common.h


# =====================================================================================================================
# the layer table
# =====================================================================================================================
def has_stn(case):
    return case['nfeat_stn'] > 0


def layers_of(case):
    """One dict per layer in the library's order: seg, kind, k (index inside its stack), cin, cout, bn, w (parameter prefix of
    the Conv1d / Linear), n (prefix of its BatchNorm or None), pooled (last convolution of its segment)."""
    wd, out = case['widths'], []

    def add(seg, kind, k, cin, cout, w, n, pooled=False):
        out.append(dict(i=len(out), seg=seg, kind=kind, k=k, cin=cin, cout=cout, bn=n is not None, w=w, n=n, pooled=pooled))
    if has_stn(case):
        cs, fs = wd['stn_conv'], wd['stn_fc']
        for k, c in enumerate(cs):
            add('stn', 'conv', k, cs[k - 1] if k else case['nfeat_stn'], c, f'ptn.stn.convs.{3 * k}', f'ptn.stn.convs.{3 * k + 1}', k + 1 == len(cs))
        for k, c in enumerate(fs):
            add('stn', 'fc', k, fs[k - 1] if k else cs[-1], c, f'ptn.stn.fcs.{3 * k}', f'ptn.stn.fcs.{3 * k + 1}')
        add('stn', 'fc', len(fs), fs[-1], 4, 'ptn.stn.proj', None)
    cs, fs = wd['conv'], wd['fc']
    for k, c in enumerate(cs):
        add('main', 'conv', k, cs[k - 1] if k else case['nfeat'], c, f'ptn.convs.{3 * k}', f'ptn.convs.{3 * k + 1}', k + 1 == len(cs))
    for k, c in enumerate(fs):
        last = k + 1 == len(fs)
        add('main', 'fc', k, fs[k - 1] if k else cs[-1] + case['nglob'], c, f'ptn.fcs.{3 * k}', None if last else f'ptn.fcs.{3 * k + 1}')
    return out


def oracle_spec(case):
    """The ModelSpec under which oracle.spg_oracle.pointnet_forward is this network."""
    from oracle import spg_oracle as O
    wd = case['widths']
    return O.ModelSpec(node_feats=case['nfeat'], ptn_widths=(tuple(wd['conv']), tuple(wd['fc'])),
                       ptn_widths_stn=(tuple(wd['stn_conv']), tuple(wd['stn_fc'])), ptn_nfeat_stn=case['nfeat_stn'], ptn_npts=case['P'])


# =====================================================================================================================
# which launches serve a shape: the predicates of the library, restated from the shape and the spg_tune keys
# =====================================================================================================================
def narrow_pair_supported(nfeat, c1, c2, P, M, keys):
    """spg_narrow.hip: spg_narrow_pair_supported."""
    return (1 <= nfeat <= GRAM_MAXF and c1 == NP_C and c2 == NP_C and 32 <= P <= 128 and P % 32 == 0 and M > 0 and
            M * NP_C * 4 < 2 ** 32 and M * nfeat * 4 < 2 ** 32 and keys.get(KEY_NO_NARROW_PAIR, 0) != 1)


def first_conv_bwd_supported(nfeat, c1, P, M, keys):
    """spg_narrow.hip: spg_first_conv_bwd_supported."""
    return (2 <= nfeat <= GRAM_MAXF and c1 == NP_C and 32 <= P <= 128 and P % 32 == 0 and M > 0 and M * NP_C * 4 < 2 ** 32 and
            keys.get(KEY_NO_NARROW_PAIR, 0) == 0 and not keys.get(KEY_NO_FIRST_CONV_BWD, 0))


def bwdpair_rows(ci):
    """spg_gemm.hip: spg_bwdpair_rows."""
    return 4096 // ci


def bwdpair_shape_supported(ci, co, M, P, pooled, keys):
    """The shape part of spg_gemm.hip: spg_bwdpair_supported (fp32 mode): the CI / CO pairs, whole tiles of spg_bwdpair_rows(CI)
    rows, 128 points per superpoint for the pooled layer."""
    if keys.get(KEY_NO_BWD_PAIR, 0):
        return False
    if not ((ci == 64 and co in (64, 128)) or (ci == 128 and (co == 128 or (co == 256 and not keys.get(KEY_NO_PAIR_SPLIT, 0))))):
        return False
    it = bwdpair_rows(ci)
    if M < it or M % it != 0:
        return False
    return P == 128 if pooled else True


def bn_fold_allowed(contributions, keys):
    """spg_dense.h: spg_bn_fold_allowed on one rank without synchronised BatchNorm (SPG_FOLD_MAX_CONTRIBUTIONS is far above
    4 B for any batch of this table)."""
    return not keys.get(KEY_NO_BN_FOLD, 0) and contributions <= 2 ** 17


def conv_stack_eval_supported(cin0, couts, P):
    """spg_convstack.hip: spg_conv_stack_eval_supported (the pointer conditions hold for every plan)."""
    if not (1 <= len(couts) <= CS_MAX_LAYERS and 1 <= P <= 128 and 1 <= cin0 <= CS_KMAX):
        return False
    for l, co in enumerate(couts):
        if co < 32 or co > 256:
            return False
        for n0 in range(0, co, 128):
            if min(co - n0, 128) not in (32, 64, 128):
                return False
        if l > 0 and couts[l - 1] > CS_KMAX:
            return False
        if l + 1 < len(couts) and co > 128:
            return False
    return True


def launch_form(case, keys=None):
    """The launches that serve the case, as a string.  Training: 'slots' (the statistics travel in the fixed-point slots) or
    'finalize' (finalize launches), then per segment 'n' (first two convolutions in one pass), 'f' (first convolution's backward in
    one pass) and per later convolution 'p' (fused backward pair) -- '-' where the general launches run.  Inference: per segment
    'stack' (one-kernel convolution stack) or 'layers'."""
    keys = dict(case['keys'] if keys is None else keys)
    B, P = case['B'], case['P']
    M = B * P
    segs = [s for s in ('stn', 'main') if s == 'main' or has_stn(case)]
    convs = {s: [l for l in layers_of(case) if l['seg'] == s and l['kind'] == 'conv'] for s in segs}
    if case['mode'] == 'eval':
        return ' '.join(f"{s}[{'stack' if conv_stack_eval_supported(convs[s][0]['cin'], [l['cout'] for l in convs[s]], P) else 'layers'}]"
                        for s in segs)
    fold = bn_fold_allowed(4 * B, keys)
    parts = ['slots' if fold else 'finalize']
    for s in segs:
        cv = convs[s]
        narrow = fold and len(cv) > 2 and narrow_pair_supported(cv[0]['cin'], cv[0]['cout'], cv[1]['cout'], P, M, keys)
        fcb = narrow and first_conv_bwd_supported(cv[0]['cin'], cv[0]['cout'], P, M, keys)
        pairs = ''.join('p' if fold and bwdpair_shape_supported(l['cin'], l['cout'], M, P, l['pooled'], keys) else '-' for l in cv[1:])
        parts.append(f"{s}[{'n' if narrow else '-'}{'f' if fcb else '-'}{pairs}]")
    return ' '.join(parts)


def neutral_keys(case):
    """spg_tune settings that must leave every output bit unchanged, because the shape already runs the fallback they select:
    only for training cases at the default keys."""
    if case['mode'] != 'train' or case['keys']:
        return []
    form = launch_form(case)
    body = ''.join(re.findall(r'\[(.*?)\]', form))
    out = []
    if 'n' not in body:
        out.append({KEY_NO_NARROW_PAIR: 1})
    if 'f' not in body:
        out.append({KEY_NO_FIRST_CONV_BWD: 1})
    if 'p' not in body:
        out.append({KEY_NO_BWD_PAIR: 1})
    if not any(l['cin'] == 128 and l['cout'] == 256 and bwdpair_shape_supported(128, 256, case['B'] * case['P'], case['P'], l['pooled'], {})
               for l in layers_of(case) if l['kind'] == 'conv'):
        out.append({KEY_NO_PAIR_SPLIT: 1})
    for k in out:
        assert launch_form(case, k) == form, (case['name'], k)
    return out


# =====================================================================================================================
# the cases
# =====================================================================================================================
EDGES = {
    'a': 'pooled layers: negative gamma on a third of the channels, gamma 0 on one, -0.0 on one',
    'b': 'one superpoint of four points repeated 32 times, one of a single point repeated 128 times',
    'c': 'an all-zero weight row in a convolution (beta < 0) and in an FC layer (beta > 0)',
    'd': 'coordinate channels at offset 1e3 with unit spread',
    'e': 'the whole cloud scaled by 1e-4',
}
# Edge d, backward: with coordinates at offset 1e3 the NETWORK is ill-conditioned, for any fp32 evaluation.  The first raw output sits
# at |y| / sigma ~ 1e3 and is stored in fp32, so the next layer's input is known to 1e-4; an error dT of the STN's transform moves every
# coordinate of its superpoint by 1e3 dT; the first convolutions' weight gradient is sum dy x with sum dy = 0 and x ~ 1e3.  Measured
# on the float32 CPU evaluation: one ReLU decision differs from float64's at |v| = 7.2e-4 of a scale of 2.63 (the tie rule admits
# 2.6e-4), and with the decisions held equal the gradients are 3e-2 ... 4e-1 from float64 (3800 x the bound on ptn.stn.convs.0.weight).
# With float32 block partials in the statistics, 5 of the 768 decisions of the first FC layer differ as well (the cap admits none).
# The forward checks are layer-local and hold.  check_backward records these figures for this case instead of asserting them
# (`excess`; the no-signal floor with them: a tensor without signal stands at 1.0e-5 there on the CPU); that every gradient is finite
# and (in its own test) the identical second run are asserted.
ILL_CONDITIONED = {'train B3 P128 edge d': 'coordinates at offset 1e3: the ReLU decisions behind the first layer and the gradients are known to '
                                           '1e-4 / 1e-1 only in any fp32 evaluation (the float32 CPU evaluation misses the same two bounds)'}
# Edge c, forward: every wavefront of a row-GEMM epilogue sums its rows' outputs in fp32, one after the other, and hands (rows, mean, M2)
# to the statistics slots.  A running sum of IDENTICAL floats rounds (3 b, 5 b, ... are not floats), so the batch mean of a constant
# channel is a few ulp off the constant -- inside the 1e-6 rms the mean is held to, but the normalised value is then rstd times
# that from beta.  Exact partial sums (pairwise or compensated) touch every statistics epilogue of the training path and the bits of
# every run: a kernel change of its own, with its own benchmark.
CONSTANT_XFAIL = ('the per-wavefront fp32 running sum of the statistics epilogue leaves the batch mean of a constant channel a few ulp '
                  'off the constant: the normalised value of the 64 -> 128 convolution\'s constant channel is ~4 rstd ulp(y) from beta')
EDGE_C_CONV, EDGE_C_FC, EDGE_C_CH = 'ptn.convs.6', 'ptn.fcs.0', 5      # (the 64 -> 128 convolution, the first FC layer; channel 5)


def _case(name, mode, B, P, form, nfeat=14, nfeat_stn=14, nglob=1, widths=PROD, keys=None, update_times=1, edge=None, ext=False, ordinary=False):
    assert not (ext and nfeat_stn)      # an external transform replaces the inner STN
    return dict(name=name, ext=ext, ordinary=ordinary, mode=mode, B=B, P=P, nfeat=nfeat, nfeat_stn=nfeat_stn, nglob=nglob, widths={k: tuple(v) for k, v in widths.items()},
                keys=dict(keys or {}), update_times=update_times, edge=edge, form=form)


def cases():
    out = []
    # ---- training, production widths, 128 points: every fused form; 2 / 3 / 5 superpoints = 4 / 6 / 10 tiles of 64 rows, 8 / 12 /
    #      20 of 32; 31 / 32 / 33 superpoints: the FC head at and across SPG_FC_ROWS
    full = 'slots stn[nfpp] main[nfpppp]'
    for B in (2, 3, 5, FC_ROWS - 1, FC_ROWS, FC_ROWS + 1):
        out.append(_case(f'train B{B} P128', 'train', B, 128, full))
    out.append(_case('train B2 P128 update_times 2', 'train', 2, 128, full, update_times=2))
    for keys, form in (({17: 1}, 'slots stn[--pp] main[--pppp]'), ({17: 2}, 'slots stn[n-pp] main[n-pppp]'),
                       ({18: 1}, 'slots stn[n-pp] main[n-pppp]'), ({14: 1}, 'slots stn[nf--] main[nf----]'),
                       ({22: 1}, 'slots stn[nfpp] main[nfppp-]'), ({10: 1}, 'finalize stn[----] main[------]')):
        k, v = next(iter(keys.items()))
        out.append(_case(f'train B3 P128 key{k}={v}', 'train', 3, 128, form, keys=keys))
    # ---- 96 / 64 / 32 points: 3 / 2 / 1 blocks of the one-pass kernels per superpoint; M = 288 and 96 rows are no whole tiles of
    #      64 rows (the 64-input pairs fall back), the pooled layer's pair needs 128 points; with and without dT
    for P, stn, main in ((96, '[nf--]', '[nf--p-]'), (64, '[nfp-]', '[nfppp-]'), (32, '[nf--]', '[nf--p-]')):
        out.append(_case(f'train B3 P{P}', 'train', 3, P, f'slots stn{stn} main{main}'))
        out.append(_case(f'train B3 P{P} no stn', 'train', 3, P, f'slots main{main}', nfeat_stn=0))
    # ---- an external 2 x 2 transform in place of the STN (LocalCloudEmbedder): its gradient from the first convolution's one-pass
    #      backward, and from the general launches (xy data gradient + spg_stn_dT)
    out.append(_case('train B3 P64 ext transform', 'train', 3, 64, 'slots main[nfppp-]', nfeat_stn=0, ext=True))
    out.append(_case('train B3 P50 ext transform', 'train', 3, 50, 'slots main[------]', nfeat_stn=0, ext=True))
    out.append(_case('eval B2 P33 ext transform', 'eval', 2, 33, 'main[stack]', nfeat_stn=0, ext=True))
    # ---- partial row tiles: every fused form off
    for P in (100, 50, 33, 1):
        out.append(_case(f'train B3 P{P}', 'train', 3, P, 'slots stn[----] main[------]'))
        out.append(_case(f'train B3 P{P} odd widths', 'train', 3, P, 'slots stn[---] main[----]', nfeat=9, nfeat_stn=9, widths=ODD))
    # ---- feature counts around 16 (two / four reduction groups of the one-pass kernels, the float64-MFMA Gram kernel up to 15) and
    #      at SPG_GRAM_MAXF; the reference's default 2-feature STN
    for nf in (11, 16, 17, 20, GRAM_MAXF):
        out.append(_case(f'train B3 P128 nfeat{nf}', 'train', 3, 128, full, nfeat=nf, nfeat_stn=nf))
    out.append(_case('train B3 P128 nfeat_stn2', 'train', 3, 128, full, nfeat_stn=2))
    # ---- global features: 256 / 257 (padded weight copy) / 259 inputs of the first FC layer
    for ng in (0, 3):
        out.append(_case(f'train B3 P128 nglob{ng}', 'train', 3, 128, full, nglob=ng))
    # ---- inference
    for B in (1, 2, 3):
        for P in (1, 31, 32, 33, 64, 65, 127, 128):
            out.append(_case(f'eval B{B} P{P}', 'eval', B, P, 'stn[stack] main[stack]'))
    for last in (32, 64, 128, 160, 192, 256):      # passes of 32 / 64 / 128 columns (160 = 128 + 32, 192 = 128 + 64); 9 features: K padded to 16
        wd = dict(conv=(64, 64, 128, 128, last), fc=(256, 64, 32), stn_conv=(64, 64, last), stn_fc=(128, 64))
        out.append(_case(f'eval B2 P33 last{last} nfeat9', 'eval', 2, 33, 'stn[stack] main[stack]', nfeat=9, nfeat_stn=9, widths=wd))
    out.append(_case('eval B3 P65 nfeat9', 'eval', 3, 65, 'stn[stack] main[stack]', nfeat=9, nfeat_stn=9))
    out.append(_case('eval B2 P33 mid96', 'eval', 2, 33, 'stn[stack] main[layers]',
                     widths=dict(conv=(64, 96, 128, 256), fc=(256, 64, 32), stn_conv=(64, 64, 128), stn_fc=(128, 64))))
    out.append(_case('eval B2 P64 mid48 odd widths', 'eval', 2, 64, 'stn[layers] main[layers]', nfeat=9, nfeat_stn=9, widths=ODD))
    # ---- forward checks only (layer-local: they need no conditioning of the case data): the FC heads' BatchNorm over 3 rows
    #      at weights of ordinary size
    out.append(_case('train B3 P128 ordinary weights', 'train', 3, 128, full, ordinary=True))
    # ---- value edges
    for e in EDGES:
        out.append(_case(f'train B3 P128 edge {e}', 'train', 3, 128, full, edge=e))
        out.append(_case(f'eval B3 P128 edge {e}', 'eval', 3, 128, 'stn[stack] main[stack]', edge=e))
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    return out


def build(case):
    """-> (state {key: float32 tensor}, clouds [B, nfeat, P], glob [B, nglob] or None, grad_emb [B, D]); seeded by the case's name.
    state['ext_transform'] [B, 4] = T - I where the case has an external transform."""
    g = torch.Generator().manual_seed(zlib.crc32(case['name'].encode()))
    B, P, e = case['B'], case['P'], case['edge']

    def randn(*s):
        return torch.randn(*s, generator=g)

    def rand(*s):
        return torch.rand(*s, generator=g)
    st = {}
    for l in layers_of(case):
        a = l['cin'] ** -0.5
        rows = B * P if l['kind'] == 'conv' else B
        if l['bn'] and rows < 32 and not case['ordinary']:
            # A BatchNorm over a handful of rows: in a channel whose rows happen to lie close together, |y| / sqrt(var) -- the factor by
            # which one rounding of y moves the normalised value, and every gradient behind it -- is unbounded, for any fp32
            # implementation.  Small weights keep |y| / sqrt(var + eps) below ~10 in EVERY channel (eps is the floor); with two rows
            # (xhat = +-1: the gradient passes only in proportion to eps / (var + eps)) var is brought down to the size of eps.
            a *= FEW_ROWS_SCALE
        st[l['w'] + '.weight'] = (2 * rand(l['cout'], l['cin']) - 1) * a
        st[l['w'] + '.bias'] = (2 * rand(l['cout']) - 1) * a
        if l['bn']:
            st[l['n'] + '.weight'] = 1 + 0.2 * randn(l['cout'])
            st[l['n'] + '.bias'] = 0.1 * randn(l['cout'])
            st[l['n'] + '.running_mean'] = 0.1 * randn(l['cout'])
            st[l['n'] + '.running_var'] = 0.5 + rand(l['cout'])
    if has_stn(case):
        st['ptn.stn.proj.weight'] = 0.05 * randn(4, case['widths']['stn_fc'][-1])      # a non-trivial 2 x 2 transform
        st['ptn.stn.proj.bias'] = 0.05 * randn(4)
    if case['ext']:
        st['ext_transform'] = 0.05 * randn(B, 4)      # T - I, as the library takes it
    clouds = 0.5 * randn(B, case['nfeat'], P)
    glob = 0.1 + 2 * rand(B, case['nglob']) if case['nglob'] else None
    w = randn(B, case['widths']['fc'][-1])
    if e == 'a':
        for l in layers_of(case):
            if l['pooled']:
                gm = st[l['n'] + '.weight']
                gm[1::3] = -gm[1::3].abs()
                gm[0], gm[2] = 0.0, -0.0
    elif e == 'b':
        clouds[0] = clouds[0, :, :4].repeat(1, P // 4)
        clouds[1] = clouds[1, :, :1].repeat(1, P)
    elif e == 'c':
        for pre, beta in ((EDGE_C_CONV, -0.3), (EDGE_C_FC, 0.2)):
            st[pre + '.weight'][EDGE_C_CH] = 0.0
            n = pre[:-1] + str(int(pre[-1]) + 1)
            st[n + '.bias'][EDGE_C_CH] = beta
            st[n + '.weight'][EDGE_C_CH] = 1.0
    elif e == 'd':
        clouds[:, :3] = 1e3 + randn(B, 3, P)
    elif e == 'e':
        clouds = clouds * 1e-4
        # var ~ 1e-7 = eps / 100 in the first convolutions.  Their bias is zero and their weights are ten times the usual: next to a
        # bias of ordinary size the fp32 raw output keeps 1e-3 of the signal, and a normalised signal of 0.01 next to beta loses as much
        # again in the second layer -- in any implementation
        for l in layers_of(case):
            if l['kind'] == 'conv' and l['k'] == 0:
                st[l['w'] + '.bias'].zero_()
                st[l['w'] + '.weight'] *= 10
    return {k: v.float().contiguous() for k, v in st.items()}, clouds.float().contiguous(), glob, w.float()


# =====================================================================================================================
# the network in plain torch, rows = points ([M, C], row b P + p): a restatement of oracle.spg_oracle.pointnet_forward that
# exposes every layer (tests/test_pointnet_cases.py pins it to the oracle, values and gradients, free and with decisions)
# =====================================================================================================================
def cloud_rows(clouds):
    B, nf, P = clouds.shape
    return clouds.permute(0, 2, 1).reshape(B * P, nf)


def transform_rows(rows, T4, B, P):
    """[x y] @ (T + I) on the first two columns, T4 [B, 4] = T - I row-major (learning/pointnet.py:123-124)."""
    T = T4.view(B, 2, 2) + torch.eye(2, dtype=T4.dtype).unsqueeze(0)
    xy = torch.bmm(rows[:, :2].reshape(B, P, 2), T).reshape(B * P, 2)
    return torch.cat([xy, rows[:, 2:]], 1)


def net_forward(case, Pm, clouds, glob, training, dec=None, taps=None):
    """Pm: parameters (and running statistics) in the dtype of the evaluation.  dec: {layer index: bool ReLU mask [rows, C]} and
    {'stn' | 'main': winners [B, C] int64}; taps (dict) receives per layer index (a, y, v) -- input, raw output, the value the ReLU
    saw -- and per segment the [B, P, C] values the max-pool saw.  -> embeddings [B, D]"""
    B, P = case['B'], case['P']
    dec = dec or {}
    L = layers_of(case)
    rows = cloud_rows(clouds)

    def layer(l, h):
        y = h @ Pm[l['w'] + '.weight'].t() + Pm[l['w'] + '.bias']
        v = None
        out = y
        if l['bn']:
            n = l['n']
            if training:
                v = F.batch_norm(y, None, None, Pm[n + '.weight'], Pm[n + '.bias'], True, 0.0, EPS)
            else:
                v = (y - Pm[n + '.running_mean']) / torch.sqrt(Pm[n + '.running_var'] + EPS) * Pm[n + '.weight'] + Pm[n + '.bias']
            out = v * dec[l['i']].to(v.dtype) if l['i'] in dec else torch.relu(v)
        if taps is not None:
            taps[l['i']] = (h, y, v)
        return out

    def segment(seg, h, extra):
        for l in L:
            if l['seg'] == seg and l['kind'] == 'conv':
                h = layer(l, h)
        h3 = h.view(B, P, h.shape[1])
        if taps is not None:
            taps[seg] = h3
        h = h3.gather(1, dec[seg].unsqueeze(1)).squeeze(1) if seg in dec else h3.max(1)[0]
        if extra is not None:
            h = torch.cat([h, extra.to(h.dtype)], 1)
        for l in L:
            if l['seg'] == seg and l['kind'] == 'fc':
                h = layer(l, h)
        return h
    if has_stn(case):
        rows = transform_rows(rows, segment('stn', rows[:, :case['nfeat_stn']], None), B, P)
    elif case['ext']:
        rows = transform_rows(rows, Pm['ext_transform'], B, P)
    return segment('main', rows, glob)


def param_keys(case):
    out = []
    for l in layers_of(case):
        out += [l['w'] + '.weight', l['w'] + '.bias'] + ([l['n'] + '.weight', l['n'] + '.bias'] if l['bn'] else [])
    return out


def net_grads(case, state, clouds, glob, w, dtype, dec=None, taps=None):
    """Gradients of sum(emb * w) in `dtype`: {parameter key: tensor} + 'd_glob' + 'd_T' (external transform).  With taps, every raw
    output keeps its gradient."""
    Pm = {k: v.to(dtype).clone().requires_grad_(k in set(param_keys(case)) or k == 'ext_transform') for k, v in state.items()}
    gl = None if glob is None else glob.to(dtype).clone().requires_grad_(True)
    emb = net_forward(case, Pm, clouds.to(dtype), gl, True, dec, taps)
    if taps is not None:
        for k, v in taps.items():
            if isinstance(k, int):
                v[1].retain_grad()
    (emb * w.to(dtype)).sum().backward()
    out = {k: Pm[k].grad.detach() for k in param_keys(case)}
    if gl is not None:
        out['d_glob'] = gl.grad.detach()
    if case['ext']:
        out['d_T'] = Pm['ext_transform'].grad.detach()
    return out


# =====================================================================================================================
# the float32 stand-in for the device (and the faults the CPU test plants in it)
# =====================================================================================================================
FAULTS = {      # fault -> the check that must catch it
    'drop_last_k': 'raw', 'pool_skips_last_row': 'pool.extremum', 'stats_skip_last_row': 'bn.mean', 'max_for_min': 'pool.extremum',
    'no_bias': 'raw', 'biased_running_var': 'running_var', 'wgrad_skips_last_tile': 'grad',
}


def bn_constants(y, gamma, beta, fault=None):
    """mean, rstd, s, t of a layer from its raw output, the way the library takes them: every block of 32 rows gives (rows, mean, M2 =
    sum (y - mean)^2) in float32; the blocks are combined exactly (the fixed-point slots: float64 here) as (sum y, sum y^2)."""
    ys = y[:-1] if fault == 'stats_skip_last_row' and y.shape[0] > 1 else y
    s1 = torch.zeros(y.shape[1], dtype=torch.float64)
    s2 = torch.zeros(y.shape[1], dtype=torch.float64)
    for part in ys.split(32):
        m = part.mean(0)
        m2 = ((part - m) ** 2).sum(0)
        s1 += part.shape[0] * m.double()
        s2 += m2.double() + part.shape[0] * m.double() ** 2
    mean = s1 / ys.shape[0]
    var = (s2 / ys.shape[0] - mean ** 2).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    mean32, rstd32 = mean.float(), rstd.float()
    s32 = gamma * rstd32
    t32 = (beta.double() - mean32.double() * s32.double()).float()      # (one rounding: fmaf(-mean, s, beta))
    return mean32, rstd32, s32, t32, mean, var


def standin_forward(case, state, clouds, glob, fault=None):
    """The training forward the way the device runs it, in float32 on the CPU: y = a W^T + b, the consumer applies max(y s + t, 0),
    the pool keeps the raw extremum by the sign of gamma.  -> fw"""
    B, P = case['B'], case['P']
    L = layers_of(case)
    state = {k: v.clone() for k, v in state.items()}
    fw = dict(layers=[None] * len(L), running={})
    rows = cloud_rows(clouds)

    def layer(l, a):
        W, b = state[l['w'] + '.weight'], state[l['w'] + '.bias']
        if fault == 'drop_last_k' and l['cin'] > 1:
            y = a[:, :-1] @ W[:, :-1].t() + b
        elif fault == 'no_bias':
            y = a @ W.t()
        else:
            y = a @ W.t() + b
        rec = dict(y=y)
        if l['bn']:
            gamma, beta = state[l['n'] + '.weight'], state[l['n'] + '.bias']
            mean32, rstd32, s, t, mean, var = bn_constants(y, gamma, beta, fault)
            rec.update(mean=mean32, rstd=rstd32, s=s, t=t)
            n = y.shape[0]
            uvar = var if fault == 'biased_running_var' else var * (n / max(n - 1, 1))
            rm, rv = state[l['n'] + '.running_mean'].double(), state[l['n'] + '.running_var'].double()
            for _ in range(case['update_times']):
                rm, rv = (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * uvar
            fw['running'][l['n']] = (rm.float(), rv.float())
        fw['layers'][l['i']] = rec
        return rec

    def fma(y, s, t):      # fmaf: the product is exact in float64, one rounding
        return (y.double() * s.double() + t.double()).float()

    def consume(rec):
        return torch.relu(fma(rec['y'], rec['s'], rec['t']))

    def segment(seg, a, extra):
        rec = None
        for l in L:
            if l['seg'] == seg and l['kind'] == 'conv':
                rec = layer(l, a)
                a = consume(rec)
                last = l
        y3 = rec['y'].view(B, P, -1)
        ysel = y3[:, :P - 1] if fault == 'pool_skips_last_row' and P > 1 else y3
        neg = state[last['n'] + '.weight'] < 0
        if fault == 'max_for_min':
            neg = torch.zeros_like(neg)
        aidx = torch.where(neg, ysel.argmin(1), ysel.argmax(1))
        pooled = y3.gather(1, aidx.unsqueeze(1)).squeeze(1)
        fw[seg] = dict(pooled=pooled if extra is None else torch.cat([pooled, extra], 1), aidx=aidx)
        a = torch.relu(fma(pooled, rec['s'], rec['t']))
        if extra is not None:
            a = torch.cat([a, extra], 1)
        for l in L:
            if l['seg'] == seg and l['kind'] == 'fc':
                rec = layer(l, a)
                if l['bn']:
                    a = consume(rec)
        return rec['y']
    if has_stn(case):
        rows = transform_rows(rows, segment('stn', rows[:, :case['nfeat_stn']].contiguous(), None), B, P)
    elif case['ext']:
        rows = transform_rows(rows, state['ext_transform'], B, P)
    fw['emb'] = segment('main', rows, glob).clone()
    return fw


def standin_backward(case, state, clouds, glob, w, fw, fault=None):
    """Float32 gradients with the stand-in's own decisions."""
    taps = {}
    g = net_grads(case, state, clouds, glob, w, torch.float32, decisions(case, fw), taps)
    for l in layers_of(case):      # the library writes exact zeros for a bias in front of a train-mode BatchNorm (analytically zero)
        if l['bn']:
            g[l['w'] + '.bias'] = torch.zeros_like(g[l['w'] + '.bias'])
    if fault == 'wgrad_skips_last_tile':
        for l in layers_of(case):
            if l['kind'] == 'conv' and l['k'] > 0:
                a, y, _ = taps[l['i']]
                tile = min(32, y.shape[0])
                g[l['w'] + '.weight'] = g[l['w'] + '.weight'] - y.grad[-tile:].t() @ a.detach()[-tile:]
    return g


# =====================================================================================================================
# the checks of the forward
# =====================================================================================================================
def _worst(err, bound):
    """max err / bound, a zero bound asking for a zero error."""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def layer_input(case, state, clouds, glob, fw, l):
    """The layer's input as the run consumed it, in float64 from the run's floats."""
    B, P = case['B'], case['P']
    L = layers_of(case)
    if l['kind'] == 'conv' and l['k'] == 0:
        rows = cloud_rows(clouds).double()
        if l['seg'] == 'stn':
            return rows[:, :case['nfeat_stn']]
        if has_stn(case):
            proj = [q for q in L if q['w'] == 'ptn.stn.proj'][0]
            rows = transform_rows(rows, fw['layers'][proj['i']]['y'].double(), B, P)
        elif case['ext']:
            rows = transform_rows(rows, state['ext_transform'].double(), B, P)
        return rows
    if l['kind'] == 'fc' and l['k'] == 0:
        prev = [q for q in L if q['seg'] == l['seg'] and q['pooled']][0]
        rec, C = fw['layers'][prev['i']], prev['cout']
        pooled = fw[l['seg']]['pooled'].double()
        return torch.cat([torch.relu(pooled[:, :C] * rec['s'].double() + rec['t'].double()), pooled[:, C:]], 1)
    rec = fw['layers'][l['i'] - 1]
    return torch.relu(rec['y'].double() * rec['s'].double() + rec['t'].double())


def check_raw(tag, ident, a, W, b, y, report=None):
    """One layer's raw output y against a @ W^T + b in float64 (a: the layer's input as the run consumed it, float64; b may be None):
    the derived dot-product bound of the module docstring, then conftest.assert_elementwise's defaults."""
    W = W.double()
    b = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else b.double()
    K = W.shape[1]
    assert a.shape[1] == K and y.shape == (a.shape[0], W.shape[0]), (tag, a.shape, y.shape)
    ref = a @ W.t() + b
    bound = 2 * (K + 4) * U24 * (a.abs() @ W.abs().t() + b.abs())
    err = (y.double() - ref).abs()
    ratio = _worst(err, bound)
    cpu = _worst(((a.float() @ W.float().t() + b.float()).double() - ref).abs(), bound)
    print(f'{tag}: raw: worst error {float(err.max()) if err.numel() else 0.0:.3e}, {ratio:.3f} of the bound (float32 CPU {cpu:.3f})')
    if report is not None:
        report.append((ident, 'y', float(err.max()) if err.numel() else 0.0, ratio, cpu))
    assert bool(torch.isfinite(y).all()) and ratio <= 1.0, f'{tag}: raw: worst element at {ratio:.3f} of the dot-product bound'
    assert_elementwise(y, ref, what=f'{tag}: raw')


def check_bn(tag, ident, y, gamma, beta, rm0, rv0, update_times, rec, got_running, report=None):
    """The BatchNorm constants a run derived from its OWN raw output y [rows, C] (rec: mean, rstd, s, t) and the running statistics it
    left (got_running: (running_mean, running_var); rm0 / rv0: before the forward) against the float64 statistics of y over exactly
    its rows, with the bounds of the module docstring."""
    y = y.double()
    n = y.shape[0]
    gamma, beta = gamma.double(), beta.double()
    mean, ey2 = y.mean(0), (y * y).mean(0)
    var = ((y - mean) ** 2).mean(0)
    rms, rstd = ey2.sqrt(), 1.0 / torch.sqrt(var + EPS)
    kappa = torch.sqrt(ey2 / (var + EPS)).clamp_min(1.0)
    s64, t64 = gamma * rstd, beta - mean * gamma * rstd
    b_mean, b_rstd = 1e-6 * rms, 1e-6 * kappa
    b_s = gamma.abs() * rstd * b_rstd + U24 * s64.abs()
    b_t = s64.abs() * b_mean + mean.abs() * gamma.abs() * rstd * b_rstd + U24 * t64.abs()
    uvar = var * (n / max(n - 1, 1))
    rm0, rv0 = rm0.double(), rv0.double()
    rm, rv, keep = rm0, rv0, 1.0
    for _ in range(update_times):
        rm, rv, keep = (1 - MOMENTUM) * rm + MOMENTUM * mean, (1 - MOMENTUM) * rv + MOMENTUM * uvar, keep * (1 - MOMENTUM)
    b_rm = 1e-6 * (keep * rm0.abs() + (1 - keep) * rms)
    b_rv = 1e-6 * kappa * rv
    got_rm, got_rv = got_running
    for what, got, want, bnd in (('bn.mean', rec['mean'], mean, b_mean), ('bn.rstd', rec['rstd'].double() / rstd - 1, torch.zeros_like(rstd), b_rstd),
                                 ('bn.s', rec['s'], s64, b_s), ('bn.t', rec['t'], t64, b_t),
                                 ('running_mean', got_rm, rm, b_rm), ('running_var', got_rv, rv, b_rv)):
        e = (got.double() - want).abs()
        r = _worst(e, bnd)
        print(f'{tag}: {what}: worst error {float(e.max()):.3e}, {r:.3f} of the bound')
        if report is not None:
            report.append((ident, what, float(e.max()), r, float('nan')))
        assert bool(torch.isfinite(got).all()) and r <= 1.0, f'{tag}: {what}: worst channel at {r:.3f} of the bound'


def check_forward(case, state, clouds, glob, fw, report=None):
    """Item 1 of the suite on one training run.  state: the parameters and the running statistics BEFORE the forward.
    report: list receiving (layer, tensor, worst error, error / bound, float32 CPU error / bound)."""
    name, B, P = case['name'], case['B'], case['P']
    for l in layers_of(case):
        rec = fw['layers'][l['i']]
        tag = f"{name}: layer {l['i']} ({l['w']})"
        a = layer_input(case, state, clouds, glob, fw, l)
        assert a.shape[1] == l['cin'] and rec['y'].shape == (a.shape[0], l['cout']), (tag, a.shape, rec['y'].shape)
        check_raw(tag, l['i'], a, state[l['w'] + '.weight'], state[l['w'] + '.bias'], rec['y'], report)
        if l['bn']:
            check_bn(tag, l['i'], rec['y'], state[l['n'] + '.weight'], state[l['n'] + '.bias'], state[l['n'] + '.running_mean'],
                     state[l['n'] + '.running_var'], case['update_times'], rec, fw['running'][l['n']], report)
    for seg in ('stn', 'main'):
        if seg == 'stn' and not has_stn(case):
            continue
        last = [l for l in layers_of(case) if l['seg'] == seg and l['pooled']][0]
        C, tag = last['cout'], f'{name}: {seg}'
        y3 = fw['layers'][last['i']]['y'].view(B, P, C)
        pooled, aidx = fw[seg]['pooled'], fw[seg]['aidx']
        assert aidx.shape == (B, C) and int(aidx.min()) >= 0 and int(aidx.max()) < P, f'{tag}: pool.bitwise: winner outside the superpoint'
        at = y3.gather(1, aidx.unsqueeze(1)).squeeze(1)
        assert torch.equal(at.view(torch.int32), pooled[:, :C].contiguous().view(torch.int32)), f'{tag}: pool.bitwise: pooled is not y at the winner'
        neg = state[last['n'] + '.weight'] < 0
        ext = torch.where(neg, y3.min(1)[0], y3.max(1)[0])
        bad = int((at != ext).sum())
        assert bad == 0, f'{tag}: pool.extremum: {bad} pooled values are not the extremum of the run\'s own y'
        ng = case['nglob'] if seg == 'main' else 0
        assert pooled.shape[1] == C + ng
        if ng:
            assert torch.equal(pooled[:, C:].contiguous().view(torch.int32), glob.contiguous().view(torch.int32)), f'{tag}: pool.global: global features changed'
    assert torch.equal(fw['emb'].view(torch.int32), fw['layers'][-1]['y'].view(torch.int32)), f'{name}: emb: not the last layer\'s output'


def constant_ratio(tag, y_col, bias, beta, mean, rstd, s, t):
    """A channel whose raw output is the constant `bias` on every row (asserted, with the batch mean within 1e-6 of it): the distance of
    the normalised value y s + t from beta, in units of rstd ulp(y).  All arguments are the channel's scalars but y_col [rows]."""
    assert bool((y_col == bias).all()), f'{tag}: constant: y is not the bias'
    v = y_col.double() * s.double() + t.double()
    ulp = float(torch.nextafter(bias.abs(), torch.tensor(float('inf'))) - bias.abs())
    allowed = float(rstd) * ulp
    off = float((v - beta.double()).abs().max())
    dmean = abs(float(mean) - float(bias))
    assert dmean <= 1e-6 * abs(float(bias)), f'{tag}: constant: bn.mean {dmean:.3e} from the constant'
    print(f'{tag}: constant: mean {float(mean):.9g} (bias {float(bias):.9g}), normalised value {off:.3e} from beta, '
          f'{off / allowed:.3f} of rstd ulp(y) = {allowed:.3e}')
    return off / allowed


def constant_channel(case, state, fw):
    """Edge c, an all-zero weight row (gamma = 1): y is the bias on every row (asserted), var = 0, and the normalised value y s + t
    should be beta within rstd ulp(y).  -> {layer prefix: distance from beta / (rstd ulp(y))}"""
    out = {}
    for l in layers_of(case):
        if l['w'] in (EDGE_C_CONV, EDGE_C_FC):
            rec, c = fw['layers'][l['i']], EDGE_C_CH
            out[l['w']] = constant_ratio(f"{case['name']}: {l['w']}", rec['y'][:, c], state[l['w'] + '.bias'][c], state[l['n'] + '.bias'][c],
                                         rec['mean'][c], rec['rstd'][c], rec['s'][c], rec['t'][c])
    return out


# =====================================================================================================================
# decisions and the backward
# =====================================================================================================================
def decisions(case, fw):
    """The run's ReLU masks (exact sign of y s + t in float64) and pool winners, as net_forward's dec."""
    dec = {}
    for l in layers_of(case):
        if l['bn']:
            rec = fw['layers'][l['i']]
            dec[l['i']] = (rec['y'].double() * rec['s'].double() + rec['t'].double()) > 0
    for seg in ('stn', 'main'):
        if seg in fw:
            dec[seg] = fw[seg]['aidx'].long()
    return dec


def check_decisions(case, state, clouds, glob, dec, excess=None):
    """The admissibility rules of test_gpu_baseline_parity._decision_conditioned against the float64 network's own decisions.
    excess (dict): the tie rule and the count cap are recorded in excess['tie'] (worst distance / admitted distance) and
    excess['count'] (most differing ReLU decisions of a layer) instead of asserted.
    -> (ReLU decisions that differ, of, winners that are not the float64 maximum, of)"""
    taps = {}
    with torch.no_grad():
        net_forward(case, {k: v.double() for k, v in state.items()}, clouds.double(), None if glob is None else glob.double(), True, None, taps)
    n_relu = d_relu = n_pool = d_pool = 0
    for key, d in dec.items():
        tag = f"{case['name']}: decisions: {key}"
        if isinstance(key, str):
            h = taps[key]
            gap = h.max(1)[0] - h.gather(1, d.unsqueeze(1)).squeeze(1)
            scale = float(h.abs().max())
            n_pool += d.numel(); d_pool += int((gap > 0).sum())
            if excess is not None:
                excess['tie'] = max(excess.get('tie', 0.0), float(gap.max()) / (TIE * scale))
            else:
                assert float(gap.max()) <= TIE * scale, f'{tag}: a winner misses the float64 maximum by {float(gap.max()):.3e} (scale {scale:.3e})'
        else:
            v = taps[key][2]
            differ = (v > 0) != d
            scale = float(v.abs().max())
            worst = float(v[differ].abs().max()) if bool(differ.any()) else 0.0
            n_relu += d.numel(); d_relu += int(differ.sum())
            if excess is not None:
                excess['tie'] = max(excess.get('tie', 0.0), worst / (TIE * scale))
            else:
                assert worst <= TIE * scale, f'{tag}: a ReLU decision differs at |v| = {worst:.3e} (scale {scale:.3e})'
            if excess is not None:
                excess['count'] = max(excess.get('count', 0), int(differ.sum()))
                continue
            assert int(differ.sum()) <= 10 * TIE * d.numel(), f'{tag}: {int(differ.sum())} of {d.numel()} ReLU decisions differ'
    return d_relu, n_relu, d_pool, n_pool


def check_backward(case, state, clouds, glob, w, fw, grads, report=None, excess=None):
    """Item 3: grads {parameter key: tensor} + 'd_glob' of the run whose forward left fw.  excess (dict, for a case of ILL_CONDITIONED
    only): the tie rule, the count cap, the gradient bound and the no-signal floor are recorded there ('tie', 'count', 'grad', 'noise')
    instead of asserted."""
    name = case['name']
    assert excess is None or name in ILL_CONDITIONED
    dec = decisions(case, fw)
    counts = check_decisions(case, state, clouds, glob, dec, excess)
    print(f'{name}: decisions: ReLU {counts[0]} / {counts[1]} differ, max-pool {counts[2]} / {counts[3]} differ')
    ref = net_grads(case, state, clouds, glob, w, torch.float64, dec)
    assert set(grads) == set(ref), (name, set(grads) ^ set(ref))
    params = {k: v for k, v in ref.items() if k not in ('d_glob', 'd_T')}
    for k, r in ref.items():
        g = grads[k].reshape(r.shape)
        assert bool(torch.isfinite(g).all()), f'{name}: grad: {k} is not finite'
        e = (g.double() - r).abs()
        noise = k in params and noise_grad(k, params)
        bound = torch.full_like(r, 1e-5) if noise else 1e-4 * r.abs() + 1e-5 * float(r.abs().max())
        ratio = _worst(e, bound)
        print(f"{name}: grad: {k}: worst error {float(e.max()):.3e}, {ratio:.3f} of the {'noise floor' if noise else 'bound'}")
        if report is not None:
            report.append((k, 'noise' if noise else 'grad', float(e.max()), ratio, float('nan')))
        if noise and excess is not None:
            excess['noise'] = max(excess.get('noise', 0.0), float(g.abs().max()) / 1e-5)
        elif noise:
            assert float(g.abs().max()) < 1e-5, f'{name}: grad: {k} (no signal) holds {float(g.abs().max()):.3e}'
        elif excess is not None:
            excess['grad'] = max(excess.get('grad', 0.0), ratio)
        else:
            assert_elementwise(g, r, what=f'{name}: grad: {k}')
    if case['edge'] == 'c':      # beta < 0 behind a constant channel: the ReLU is closed on every row, nothing passes
        c = EDGE_C_CH
        n = EDGE_C_CONV[:-1] + str(int(EDGE_C_CONV[-1]) + 1)
        nxt = EDGE_C_CONV[:-1] + str(int(EDGE_C_CONV[-1]) + 3)
        for k, t in ((EDGE_C_CONV + '.weight', grads[EDGE_C_CONV + '.weight'][c]), (n + '.weight', grads[n + '.weight'][c]),
                     (n + '.bias', grads[n + '.bias'][c]), (nxt + '.weight', grads[nxt + '.weight'].reshape(ref[nxt + '.weight'].shape)[:, c])):
            assert float(t.abs().max()) == 0.0, f'{name}: grad: edge c: {k} through the closed channel is not exactly zero'
    return counts


# =====================================================================================================================
# inference
# =====================================================================================================================
def eval_reference(case, state, clouds, glob, dtype=torch.float64):
    """-> {'emb', 'stn.pooled', 'main.pooled'}: the embeddings and the pooled rows as the library keeps them (raw extremum of the last
    convolution by the sign of the BatchNorm scale, then the global features)."""
    taps = {}
    Pm = {k: v.to(dtype) for k, v in state.items()}
    with torch.no_grad():
        emb = net_forward(case, Pm, clouds.to(dtype), None if glob is None else glob.to(dtype), False, None, taps)
    out = {'emb': emb}
    for l in layers_of(case):
        if l['pooled']:
            y3 = taps[l['i']][1].view(case['B'], case['P'], l['cout'])
            neg = state[l['n'] + '.weight'] < 0
            pooled = torch.where(neg, y3.min(1)[0], y3.max(1)[0])
            if l['seg'] == 'main' and glob is not None:
                pooled = torch.cat([pooled, glob.to(dtype)], 1)
            out[l['seg'] + '.pooled'] = pooled
    return out


def check_eval(case, state, clouds, glob, got, report=None):
    ref = eval_reference(case, state, clouds, glob)
    cpu = eval_reference(case, state, clouds, glob, torch.float32)
    assert set(got) == set(ref), (case['name'], set(got) ^ set(ref))
    for k, r in ref.items():
        bound = 1e-4 * r.abs() + 1e-5 * float(r.abs().max())
        e = (got[k].double() - r).abs()
        ratio, c = _worst(e, bound), _worst((cpu[k].double() - r).abs(), bound)
        print(f"{case['name']}: eval: {k}: worst error {float(e.max()):.3e}, {ratio:.3f} of the bound (float32 CPU {c:.3f})")
        if report is not None:
            report.append((k, 'eval', float(e.max()), ratio, c))
        assert bool(torch.isfinite(got[k]).all()), f"{case['name']}: eval: {k} is not finite"
        assert_elementwise(got[k], r, what=f"{case['name']}: eval: {k}")
