"""GPU: PointNet above 128 points per superpoint (csrc/spg_segments.hip and the segment plan of spg_pointnet.hip).
A superpoint of P = S x Ps points runs its convolutions as S pseudo-superpoints of Ps points; the cloud layout, the 2 x 2 transform
and the max-pool are translated between the two views.

* whole training steps and eval forwards through the module API against the CPU oracle, on the scenes
  tests/test_pointnet_npts_cases.py admits (tolerances of tests/test_gpu_model.py);
* the segments' view is the existing path bit for bit: the convolutions' outputs and statistics equal a run on the clouds reshaped
  to [B * S, nfeat, Ps], the merged max-pool is the first extremum of that run's per-segment pools;
* winners at cross-segment ties, every element of both stacks, train and eval;
* an external transform with its gradient (LocalCloudEmbedder's form), FusedStep against the module path, the refusals.

`python tests/test_gpu_pointnet_npts.py` prints the measured error figures (profiles/npts_errors.txt)."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import pointnet_cases as C
import pointnet_npts_cases as N
from conftest import assert_elementwise, build_model, maxrel, noise_grad
from oracle import spg_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-4          # tests/test_gpu_model.py: embeddings / logits / loss, max|d| / max|ref|


# =====================================================================================================================
# the module path: training step, eval forward, FusedStep
# =====================================================================================================================
def _gci(batch):
    from superpoint_graph_amd.learning import ecc
    return ecc.GraphConvInfo.from_buffers(batch['idxn'].clone(), batch['degs'].clone(), batch['edgefeats'].clone())


def _run(model, batch, monger):
    from superpoint_graph_amd.learning import pointnet
    model.ecc.set_info([_gci(batch)], 1)
    embedder = pointnet.CloudEmbedder(types.SimpleNamespace(cuda=1, ptn_mem_monger=monger))
    emb = embedder.run(model, None, batch['clouds_flag'], batch['clouds'], batch['clouds_global'])
    return emb, model.ecc(emb), embedder


def train_step_errors(name, monger):
    """-> (forward errors, {parameter: gradient error}, largest no-signal gradient, worst running-statistics error)."""
    spec, batch, state0, cw = N.case(name)
    loss_o, logits_o, emb_o, grads_o, st = N.oracle_step(name, bool(monger))
    model = build_model(spec, state0).to(DEV).train()
    emb, logits, embedder = _run(model, batch, monger)
    loss = F.cross_entropy(logits, batch['label_mode'].to(DEV), weight=cw.to(DEV))
    model.zero_grad()
    loss.backward()
    embedder.bw_hook()
    fwd = dict(emb=maxrel(emb, emb_o), logits=maxrel(logits, logits_o), loss=maxrel(loss, loss_o))
    grads, noise = {}, 0.0
    for k, p in model.named_parameters():
        if noise_grad(k, grads_o):
            noise = max(noise, float(p.grad.abs().max()))
        else:
            grads[k] = maxrel(p.grad, grads_o[k])
    sd = model.state_dict()
    running = max(maxrel(sd[k].double(), v.double()) for k, v in st.items() if 'running' in k)
    return fwd, grads, noise, running


@pytest.mark.parametrize('monger', [1, 0])
@pytest.mark.parametrize('name', sorted(N.SPECS))
def test_train_step_vs_oracle(hip, name, monger):
    """A whole training step at 256 / 512 / 160 / 384 points per superpoint against the fp32 CPU oracle, built exactly as
    tests/test_gpu_model.py::test_odd_shapes_train_step_vs_oracle: embeddings, logits and loss below 1e-4, every gradient with signal
    below 1e-3, the running statistics below 1e-5 (twice updated with ptn_mem_monger)."""
    fwd, grads, noise, running = train_step_errors(name, monger)
    print(f'{name} monger {monger}: emb {fwd["emb"]:.2e} logits {fwd["logits"]:.2e} loss {fwd["loss"]:.2e} worst gradient '
          f'{max(grads.values()):.2e} ({max(grads, key=grads.get)}) running statistics {running:.2e}')
    assert fwd['emb'] < TOL and fwd['logits'] < TOL and fwd['loss'] < TOL, fwd
    bad = {k: e for k, e in grads.items() if not e <= 1e-3}
    assert not bad, bad
    assert noise < 1e-5 and running < 1e-5, (noise, running)


def eval_forward(name):
    spec, batch, state0, _ = N.case(name)
    model = build_model(spec, state0).to(DEV).eval()
    with torch.no_grad():
        emb, logits, _ = _run(model, batch, 1)
        emb2, logits2, _ = _run(model, batch, 0)
    eo, lo = O.model_forward(batch, spec, {k: v.clone() for k, v in state0.items()}, False)
    return batch, emb, logits, emb2, logits2, eo, lo


@pytest.mark.parametrize('name', ['p160_odd', 'p256_prod'])
def test_eval_forward_vs_oracle(hip, name):
    """Inference (the one-kernel convolution stack per segment at 2 x 128 points, the layer launches at 2 x 80) against
    O.model_forward: every element within 1e-4, exactly zero rows for the too-small superpoints, bit-identical on repetition."""
    batch, emb, logits, emb2, logits2, eo, lo = eval_forward(name)
    print(f'{name} eval: emb {maxrel(emb, eo):.2e} logits {maxrel(logits, lo):.2e}')
    assert maxrel(emb, eo) < TOL and maxrel(logits, lo) < TOL
    assert_elementwise(emb, eo, what=f'{name}: eval embeddings')
    assert_elementwise(logits, lo, what=f'{name}: eval logits')
    invalid = (batch['clouds_flag'] != 0).nonzero().reshape(-1)
    assert invalid.numel() > 0 and float(emb[invalid.to(DEV)].abs().max()) == 0.0
    assert torch.equal(emb, emb2) and torch.equal(logits, logits2)


def test_fused_step_is_the_module_path_bit_for_bit_at_256_points(hip):
    """tests/test_gpu_fused.py's contract at npts = 256 on the 21-superpoint scene: spg_train_step with the classifier / cross entropy
    as separate launches (spg_tune key 15) gives the module path's loss, logits, descriptors, gradients and state, two steps."""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.flat import FlatParameters
    from superpoint_graph_amd.fused import FusedStep, supports
    from superpoint_graph_amd.learning import pointnet
    spec, batch, state0, cw = N.case('p256_prod')
    cw = cw.to(DEV)

    def run(fused):
        model = build_model(spec, state0).to(DEV).train()
        arena = FlatParameters(model, lazy_zero=True, host_counters=True)
        assert supports(model)
        step = FusedStep(model, arena, class_weights=cw, reduction='mean', ptn_mem_monger=True) if fused else None
        rec = []
        for _ in range(2):
            gi = _gci(batch)
            model.ecc.set_info([gi], 1)
            arena.zero_grad()
            if fused:
                loss, logits = step(batch['clouds_flag'], batch['clouds'], batch['clouds_global'], gi, batch['label_mode'].to(DEV))
                emb = step.embeddings
            else:
                embedder = pointnet.CloudEmbedder(types.SimpleNamespace(cuda=1, ptn_mem_monger=1))
                emb = embedder.run(model, None, batch['clouds_flag'], batch['clouds'], batch['clouds_global'])
                logits = model.ecc(emb)
                loss = ops.cross_entropy(logits, batch['label_mode'].to(DEV), weight=cw, reduction='mean')
                loss.backward(arena.one)
                embedder.bw_hook()
            torch.cuda.synchronize()
            rec.append(dict(loss=loss.detach().clone(), logits=logits.detach().clone(), emb=emb.detach().clone(),
                            **{'grad ' + k: p.grad.clone() for k, p in model.named_parameters()}))
            arena.adam_step(lr=1e-3, grad_clip=1.0)
        return rec, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    modules, sd_m = run(False)
    old = hip.spg_tune(15, 1)
    try:
        fused, sd_f = run(True)
    finally:
        hip.spg_tune(15, old)
    assert float(modules[0]['loss']) > 0 and bool(torch.isfinite(modules[1]['loss']))
    for it, (a, b) in enumerate(zip(modules, fused)):
        for k in a:
            assert torch.equal(a[k], b[k]), (it, k)
    for k in sd_m:
        assert torch.equal(sd_m[k], sd_f[k]), k


@pytest.mark.parametrize('npts', [131, 4096, 4097])
def test_unsupported_npts_is_refused_before_any_launch(hip, npts):
    """The modules and ops.pointnet_forward raise NotImplementedError with the rule: nothing is allocated or launched (the
    parameters, running statistics and batch counters keep their bits, no workspace is asked for)."""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import pointnet
    ptn = pointnet.PointNet([64, 64, 128], [128, 64, 32], [32, 64], [64, 16], 6, 6, prelast_do=0).to(DEV).train()
    before = {k: v.clone() for k, v in ptn.state_dict().items()}
    clouds = torch.randn(3, 6, npts, device=DEV)
    with pytest.raises(NotImplementedError, match=r'divisor in \[32, 128\]'):
        ptn(clouds, torch.ones(3, 1, device=DEV))
    stn = pointnet.STNkD(6, [32, 64], [64, 16]).to(DEV)
    with pytest.raises(NotImplementedError, match=f'npts = {npts}'):
        stn(clouds)
    assert all(torch.equal(v, before[k]) for k, v in ptn.state_dict().items())
    cfg = ops.make_pointnet_cfg(6, 0, 1, npts, [], [], [64, 64, 128], [128, 64, 32])
    with pytest.raises(NotImplementedError, match=f'npts = {npts}'):
        ops.pointnet_forward(cfg, clouds, torch.ones(3, 1, device=DEV), [], True)


def test_cli_trains_at_256_points(tmp_path):
    """`python -m superpoint_graph_amd.learning.main ... --ptn_npts 256` on the in-memory dataset of tests/main_fixture.py (as
    tests/test_gpu_main.py runs it, in process): two epochs with evaluation, every loss finite, a checkpoint written; 131 is refused
    with the rule before the first step."""
    import json
    import os

    import main_fixture
    from superpoint_graph_amd.learning import datasets
    from superpoint_graph_amd.learning import main as cli
    train, test = main_fixture.make_dataset(0)
    points = {name: pts for name, _, pts in train + test}
    datasets.register_memory_dataset('memtest', [(n, g) for n, g, _ in train], [(n, g) for n, g, _ in test], [], points,
                                     main_fixture.N_CLASSES, 14)
    odir = str(tmp_path / 'out')
    session = cli.main(['--dataset', 'memtest', '--odir', odir] + main_fixture.CLI + ['--ptn_npts', '256'])
    torch.cuda.synchronize()
    losses = [float(x[0]) for x in session.iter_log] + [float(x) for x in session.eval_log]
    assert len(session.iter_log) >= 4 and all(l == l and 0 < l < 10 for l in losses), losses
    with open(os.path.join(odir, 'trainlog.json')) as f:
        assert len(json.load(f)) == 2
    assert os.path.exists(os.path.join(odir, 'model.pth.tar'))
    with pytest.raises(NotImplementedError, match=r'divisor in \[32, 128\]'):
        cli.main(['--dataset', 'memtest', '--odir', str(tmp_path / 'refused')] + main_fixture.CLI + ['--ptn_npts', '131'])


# =====================================================================================================================
# ops level: the workspace of one forward
# =====================================================================================================================
def _cfg(case, npts=None, stn=True):
    from superpoint_graph_amd import ops
    wd = case['widths']
    has = stn and C.has_stn(case)
    return ops.make_pointnet_cfg(case['nfeat'], case['nfeat_stn'] if has else 0, case['nglob'], npts or case['P'],
                                 wd['stn_conv'] if has else [], wd['stn_fc'] if has else [], wd['conv'], wd['fc'], False, C.EPS, C.MOMENTUM)


def _groups(case, state, stn=True):
    """Fresh device copies (a training forward updates the running statistics in place), one row per layer of the library's table."""
    P = {k: v.to(DEV) for k, v in state.items()}
    rows = [(P[l['w'] + '.weight'], P[l['w'] + '.bias']) + (tuple(P[l['n'] + s] for s in ('.weight', '.bias', '.running_mean', '.running_var'))
                                                             if l['bn'] else (None,) * 4)
            for l in C.layers_of(case) if stn or l['seg'] == 'main']
    return P, rows


def _buf(hip, st, training, layer, what, n, dtype=torch.float32):
    off = hip.spg_pointnet_debug_offset(ctypes.byref(st.cfg), st.B, int(training), layer, what)
    assert off >= 0, (layer, what)
    return st.ws[off:off + 4 * n].view(dtype).cpu().clone()


def _pool(hip, st, training, code, Cc, ng=0):
    """-> (pooled [B, Cc + ng] float32, aidx [B, Cc] int64) of the STN (-1) / main (-2) stack as the library keeps them."""
    ld = int(hip.spg_pointnet_debug_offset(ctypes.byref(st.cfg), st.B, int(training), code, 2))
    assert ld >= Cc + ng and ld % 4 == 0
    return (_buf(hip, st, training, code, 0, st.B * ld).view(st.B, ld)[:, :Cc + ng].contiguous(),
            _buf(hip, st, training, code, 1, st.B * ld, torch.int32).view(st.B, ld)[:, :Cc].long().contiguous())


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _stack(case, seg):
    convs = [l for l in C.layers_of(case) if l['seg'] == seg and l['kind'] == 'conv']
    return convs, convs[-1], case['nglob'] if seg == 'main' else 0


def _forward(hip, case, state, clouds, glob, training, npts=None, stn=True, T4=None):
    """One forward on fresh parameter copies -> (PointNetState, device parameters)."""
    from superpoint_graph_amd import ops
    P, rows = _groups(case, state, stn)
    _, st = ops.pointnet_forward(_cfg(case, npts, stn), clouds.to(DEV), None if glob is None else glob.to(DEV), rows, training, 1,
                                 ext_transform=None if T4 is None else T4.to(DEV))
    torch.cuda.synchronize()
    return st, P


def _transform_of(hip, case, st, training):
    """The raw projection [B, 4] = T - I the inner STN left in the workspace."""
    proj = [l for l in C.layers_of(case) if l['w'] == 'ptn.stn.proj'][0]
    return _buf(hip, st, training, proj['i'], 0, st.B * 4).view(st.B, 4)


def _segment_runs(hip, case, state, clouds, glob, training, T4):
    """The existing path at npts = Ps on the clouds in the segments' view: the whole network (its STN stack is the P-point run's: the
    STN convolutions see no transform) and the network without STN under the P-point run's transform, every segment carrying its
    superpoint's (its main stack is the P-point run's).  -> {seg: (PointNetState, layer index offset)}"""
    Ps, S = N.segments(case['P'])
    cs, gs = N.by_segments(clouds, S), None if glob is None else N.by_segments(glob, S)
    n_stn = len([l for l in C.layers_of(case) if l['seg'] == 'stn'])
    return {'stn': (_forward(hip, case, state, cs, gs, training, Ps)[0], 0),
            'main': (_forward(hip, case, state, cs, gs, training, Ps, stn=False, T4=N.by_segments(T4, S))[0], -n_stn)}


@pytest.mark.parametrize('P', [256, 160])
def test_segments_are_the_existing_path_bit_for_bit(hip, P):
    """Train mode, B = 3: every convolution's raw output y_l and BatchNorm mean / rstd / s / t equal those of the existing path on
    the same clouds reshaped to [B * S, nfeat, Ps] at npts = Ps -- the row space is the same and the statistics slots are order-free
    (STN stack: against the whole network at Ps; main stack: against the network without STN under this run's transform).  The
    merged pooled value is the first extremum of that run's S per-segment pooled values, the merged winner s * Ps + its winner."""
    wd, nf = (C.PROD, 14) if P == 256 else (C.ODD, 9)
    case = C._case(f'segments B3 P{P}', 'train', 3, P, None, nfeat=nf, nfeat_stn=nf, widths=wd, edge='a', ordinary=True)
    state, clouds, glob, _ = C.build(case)
    Ps, S = N.segments(P)
    B, M = case['B'], case['B'] * P
    st, _ = _forward(hip, case, state, clouds, glob, True)
    ref = _segment_runs(hip, case, state, clouds, glob, True, _transform_of(hip, case, st, True))
    for seg, code in (('stn', -1), ('main', -2)):
        rs, shift = ref[seg]
        convs, last, ng = _stack(case, seg)
        for l in convs:
            y, yr = _buf(hip, st, 1, l['i'], 0, M * l['cout']), _buf(hip, rs, 1, l['i'] + shift, 0, M * l['cout'])
            assert torch.equal(_bits(y), _bits(yr)), f"{seg}: y of layer {l['i']} ({l['w']})"
            for what, nm in ((1, 's'), (2, 't'), (3, 'mean'), (4, 'rstd')):
                assert torch.equal(_bits(_buf(hip, st, 1, l['i'], what, l['cout'])), _bits(_buf(hip, rs, 1, l['i'] + shift, what, l['cout']))), \
                    f"{seg}: {nm} of layer {l['i']} ({l['w']})"
        Cc = last['cout']
        pooled, aidx = _pool(hip, st, 1, code, Cc, ng)
        pr, ar = _pool(hip, rs, 1, code, Cc)
        neg = state[last['n'] + '.weight'] < 0
        best, win = N.first_extremum(pr.view(B, S, Cc), ar.view(B, S, Cc), neg, Ps)
        assert torch.equal(_bits(pooled[:, :Cc]), _bits(best)), f'{seg}: merged pooled values'
        assert torch.equal(aidx, win), f'{seg}: merged winners'
        assert int(win.max()) >= Ps, f'{seg}: no winner beyond the first segment'
        if ng:
            assert torch.equal(_bits(pooled[:, Cc:]), _bits(glob)), f'{seg}: global features'


@pytest.mark.parametrize('widths', ['prod', 'odd'])
@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_winners_at_cross_segment_ties(hip, mode, widths):
    """B = 2, P = 256 = 2 x 128: a cloud whose second half repeats its first half, a cloud whose extrema lie in the last segment,
    gamma positive, negative, 0.0 and -0.0 in the pooled layers.  Every pooled value and winner of both stacks, none left out.
    Train: the winner is the FIRST index of the maximum (minimum where gamma < 0) of the device's own y over the superpoint's 256
    rows, the pooled value is y there, bit for bit.  Eval: the pooled layer's y is not kept, and the one-kernel convolution stack
    ('prod') keeps no winners: the pooled bits -- and with the layer launches ('odd') the winners -- are the first extremum over the
    segments of the existing path's run at npts = 128 on the same clouds in the segments' view."""
    case, state, clouds, glob = N.tie_case(widths)
    training = mode == 'train'
    B, P = case['B'], case['P']
    Ps, S = N.segments(P)
    st, _ = _forward(hip, case, state, clouds, glob, training)
    ref = None if training else _segment_runs(hip, case, state, clouds, glob, False, _transform_of(hip, case, st, False))
    stacked = not training and C.conv_stack_eval_supported(case['nfeat'], list(case['widths']['conv']), Ps)
    assert stacked == (widths == 'prod' and not training)
    for seg, code in (('stn', -1), ('main', -2)):
        convs, last, ng = _stack(case, seg)
        Cc = last['cout']
        neg = state[last['n'] + '.weight'] < 0
        pooled, aidx = _pool(hip, st, training, code, Cc, ng)
        if training:
            y = _buf(hip, st, 1, last['i'], 0, B * P * Cc).view(B, P, Cc)
            ext = torch.where(neg, y.min(1)[0], y.max(1)[0])
            hits = y == ext.unsqueeze(1)
            first = hits.int().argmax(1)      # (the first True: argmax of a 0 / 1 tensor returns the first maximum on the CPU)
            # the case is what it claims, on the device's own values: ties across the segments, and extrema only in the last one
            both = hits[:, :Ps].any(1) & hits[:, Ps:].any(1)
            assert bool(both[0].all()), f'{seg}: cloud 0 holds channels without a cross-segment tie'
            assert int((first[1] >= Ps).sum()) > Cc // 4, f'{seg}: cloud 1 holds too few extrema in the last segment only'
            for sel, what in ((neg, 'gamma < 0'), (~neg, 'gamma >= 0')):
                assert int((both & sel).sum()) > 0 and int(((first >= Ps) & sel).sum()) > 0, f'{seg}: {what} is not exercised'
            want_v, want_i = y.gather(1, first.unsqueeze(1)).squeeze(1), first
        else:
            pr, ar = _pool(hip, ref[seg][0], False, code, Cc)
            want_v, want_i = N.first_extremum(pr.view(B, S, Cc), ar.view(B, S, Cc), neg, Ps)
            tied = (pr.view(B, S, Cc)[:, 0] == pr.view(B, S, Cc)[:, 1])
            assert bool(tied[0].all()) and int((~tied[1]).sum()) > Cc // 4, f'{seg}: the eval case holds no cross-segment ties'
        assert torch.equal(_bits(pooled[:, :Cc]), _bits(want_v)), f'{seg}: pooled bits'
        if not stacked:
            assert torch.equal(aidx, want_i), f'{seg}: winners: {int((aidx != want_i).sum())} of {aidx.numel()} differ'
            assert int(aidx[0].max()) < Ps, f'{seg}: a tie of cloud 0 went to the second segment'
        if ng:
            assert torch.equal(_bits(pooled[:, Cc:]), _bits(glob)), f'{seg}: global features'


def external_transform_errors(hip):
    from superpoint_graph_amd import ops
    case = N.ext_case()
    state, clouds, glob, w = C.build(case)
    P, rows = _groups(case, state)
    emb, st = ops.pointnet_forward(_cfg(case), clouds.to(DEV), glob.to(DEV), rows, True, 1, ext_transform=P['ext_transform'])
    gg, g_T, g_glob = ops.pointnet_backward(st, rows, w.to(DEV), want_input_grads=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        e64 = C.net_forward(case, {k: v.double() for k, v in state.items()}, clouds.double(), glob.double(), True)
    ref = C.net_grads(case, state, clouds, glob, w, torch.float64)
    got = {'d_T': g_T.cpu(), 'd_glob': g_glob.cpu()}
    for l, row in zip(C.layers_of(case), gg):
        got[l['w'] + '.weight'], got[l['w'] + '.bias'] = row[0].cpu(), row[1].cpu()
        if l['bn']:
            got[l['n'] + '.weight'], got[l['n'] + '.bias'] = row[2].cpu(), row[3].cpu()
    params = {k: v for k, v in ref.items() if k not in ('d_glob', 'd_T')}
    errs = {k: maxrel(got[k].reshape(r.shape), r) for k, r in ref.items() if k in ('d_glob', 'd_T') or not noise_grad(k, params)}
    noise = max(float(got[k].abs().max()) for k in params if noise_grad(k, params))
    return maxrel(emb, e64), errs, noise


def test_external_transform_and_its_gradient_at_256_points(hip):
    """LocalCloudEmbedder's form (no inner STN, an external 2 x 2 transform per superpoint, one global feature), B = 5, P = 256:
    embeddings, the gradients wrt the transform and the global features -- and every parameter gradient -- against float64 autograd
    of the same expression, inside tests/test_gpu_local.py's bounds (embeddings 2e-5, gradients 5e-4 of the largest element)."""
    e_emb, errs, noise = external_transform_errors(hip)
    print(f'external transform, B 5 P 256: emb {e_emb:.2e} d_T {errs["d_T"]:.2e} d_glob {errs["d_glob"]:.2e} worst gradient '
          f'{max(errs.values()):.2e} ({max(errs, key=errs.get)})')
    assert e_emb <= 2e-5
    assert errs['d_T'] < 5e-4 and errs['d_glob'] < 5e-4, errs
    bad = {k: e for k, e in errs.items() if not e < 5e-4}
    assert not bad, bad
    assert noise < 1e-5


if __name__ == '__main__':
    from superpoint_graph_amd import _lib
    hip_ = _lib.lib()
    print('PointNet above 128 points per superpoint: fp32 error figures on the device (max|d| / max|ref|)')
    print('training step against the fp32 CPU oracle (bounds: forward 1e-4, gradients 1e-3, running statistics 1e-5)')
    for name_ in sorted(N.SPECS):
        for monger_ in (1, 0):
            f_, g_, n_, r_ = train_step_errors(name_, monger_)
            print(f'  {name_:15s} monger {monger_}: emb {f_["emb"]:.2e} logits {f_["logits"]:.2e} loss {f_["loss"]:.2e} worst gradient '
                  f'{max(g_.values()):.2e} ({max(g_, key=g_.get)}) no-signal gradients {n_:.1e} running statistics {r_:.2e}')
    print('eval forward against O.model_forward (bound: 1e-4 per element)')
    for name_ in ('p160_odd', 'p256_prod'):
        _, emb_, logits_, _, _, eo_, lo_ = eval_forward(name_)
        print(f'  {name_:15s}: emb {maxrel(emb_, eo_):.2e} logits {maxrel(logits_, lo_):.2e}')
    e_, errs_, n_ = external_transform_errors(hip_)
    print('external transform, B 5 P 256, against float64 autograd (bounds: embeddings 2e-5, gradients 5e-4)')
    print(f'  emb {e_:.2e} d_T {errs_["d_T"]:.2e} d_glob {errs_["d_glob"]:.2e} worst gradient {max(errs_.values()):.2e} ({max(errs_, key=errs_.get)})')
