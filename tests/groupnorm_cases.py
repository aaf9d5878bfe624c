"""Case builders and float64 references for the GroupNorm / LayerNorm local embedder (csrc/spg_groupnorm.hip) at its
shape and value edges.  Plain module (no test in it): tests/test_groupnorm_cases.py checks the cases on the CPU,
tests/test_gpu_groupnorm_edges.py runs the device against the references.

The bound is conftest.assert_elementwise with its defaults on EVERY element of every tensor (tests/op_cases.py: bound_ratio,
measure, ADMIT are imported from there).  A case is admitted only if the float32 CPU evaluation of its reference stays within
ADMIT = 0.25 of the bound.  Nothing here is derived from what the device returns.

Two declared exceptions, named per tensor by `declare` from the shape of the case alone:
* exact_zero: a group of ONE element (Cg = 1 in a head layer; Cg = 1 and npts = 1 in a convolution) has x - mean = 0, so xhat = 0
  and dz = rstd * (dxh - mean(dxh) - 0) = 0 in the kernel's arithmetic: the layer's dW, db, dgamma and every gradient below it
  are exactly zero.  `reference` checks that the float64 reference is below 1e-12 of the case's largest gradient there and sets
  it to exact zero; the device must return zeros (of either sign).
* noise: the bias of a convolution in front of one-channel groups with npts > 1: the normalisation removes the bias, the gradient
  is analytically zero but is a sum of rounded terms on both sides.  Judged against the floor of tests/test_gpu_groupnorm.py,
  1e-5 of the case's largest gradient.

Evaluators: gn_reference (the network the C ABI runs: ops.gn_forward / gn_backward) and composed_reference (what
LocalCloudEmbedder.run_batch composes: STN, T, stn_as_global, PointNet, L2 normalisation).  Both take a dtype (float64: the
reference; float32: the admission figure) and keyword knobs that are all off by default; a knob restates one plausible kernel
mistake (KNOBS)."""
import functools

import torch
import torch.nn.functional as F

from op_cases import ADMIT, bound_ratio, measure, worst  # noqa: F401  (re-exported for the two test modules)

EPS = 1e-5
NOISE_FLOOR = 1e-5                  # tests/test_gpu_groupnorm.py::_grad_check
ZERO_CHECK = 1e-12
RUN, MAX_GRID = 32, 256             # spg_groupnorm.hip: clouds of a run, workgroups of the backward
VALUE_CLASSES = ('unit', 'identical', 'duplicate pairs', 'zero', '1e-3', '1e3', 'offset 100')
KNOBS = ('unbiased', 'no_eps', 'eps_after_root', 'last_max_wins', 'all_maxima', 'whole_layer_stats', 'relu_ge', 'drop_xhat_term',
         'T_transposed_fwd', 'T_transposed_bwd', 'globals_in_front', 'drop_partial_run', 'drop_beyond_grid', 'drop_odd_cin',
         'drop_partial_tile', 'drop_points_32')


# =====================================================================================================================
# the network, in plain torch
# =====================================================================================================================
class _ReluGe(torch.autograd.Function):
    """ReLU whose backward mask is u >= 0 (knob relu_ge)."""

    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return u.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        return g * (ctx.saved_tensors[0] >= 0).to(g.dtype)


class _TransformWrongBackward(torch.autograd.Function):
    """[x y] @ T whose backward applies T where T^T belongs, and returns dT transposed (knob T_transposed_bwd)."""

    @staticmethod
    def forward(ctx, xy, T):
        ctx.save_for_backward(xy, T)
        return torch.bmm(xy, T)

    @staticmethod
    def backward(ctx, g):
        xy, T = ctx.saved_tensors
        return torch.bmm(g, T), torch.bmm(xy.transpose(1, 2), g).transpose(1, 2)


def _norm(x, G, gamma, beta, eps, k):
    """GroupNorm of x [B, C] or [B, C, P]; without knobs torch's own."""
    if not k:
        return F.group_norm(x, G, gamma, beta, eps)
    B, C = x.shape[:2]
    xg = x.reshape(B, 1 if k.get('whole_layer_stats') else G, -1)
    n = xg.shape[2]
    mu = xg.mean(2, keepdim=True)
    var = ((xg - mu) ** 2).sum(2, keepdim=True) / (max(n - 1, 1) if k.get('unbiased') else n)
    if k.get('no_eps'):
        rstd = 1.0 / torch.sqrt(var)
    elif k.get('eps_after_root'):
        rstd = 1.0 / (torch.sqrt(var) + eps)
    else:
        rstd = 1.0 / torch.sqrt(var + eps)
    if k.get('drop_xhat_term'):          # rstd as a constant: dz = rstd * (dxh - mean(dxh))
        rstd = rstd.detach()
    shape = (1, C) + (1,) * (x.dim() - 2)
    return ((xg - mu) * rstd).reshape(x.shape) * gamma.reshape(shape) + beta.reshape(shape)


def _relu(u, k):
    return _ReluGe.apply(u) if k.get('relu_ge') else F.relu(u)


def _affine(x, W, b, k, conv):
    """conv1d (x [B, cin, P]) or linear (x [B, cin])."""
    cout, cin = W.shape
    if k.get('drop_odd_cin') and cin % 2 == 1:
        W = W * torch.cat([torch.ones(cin - 1, dtype=W.dtype), torch.zeros(1, dtype=W.dtype)])
    op = (lambda a, w, bias: F.conv1d(a, w[:, :, None], bias)) if conv else F.linear
    if k.get('drop_points_32') and conv and x.shape[2] > 32:      # dW from the points below 32 only; dx and the value unchanged
        xm = x.detach().clone()
        xm[:, :, 32:] = 0
        part = op(xm, W, None)
        y = op(x, W.detach(), b) + (part - part.detach())
    else:
        y = op(x, W, b)
    if k.get('drop_partial_tile') and cout > 32 and cout % 32:
        keep = (torch.arange(cout) < (cout // 32) * 32).to(y.dtype)
        y = y * keep.reshape((1, cout) + (1,) * (y.dim() - 2))
    return y


class _SameBits(torch.autograd.Function):
    """Values of x [B, C, P] taken from each point's representative (the first point of the cloud with the same input column);
    the gradient passes through unchanged.  Points with equal inputs have equal activations, but the CPU kernels behind conv1d
    and group_norm (vector bodies and remainder loops) do not promise them the same BITS on every machine, and a difference in
    the last place would decide the arg-max below instead of `the first of equals`."""

    @staticmethod
    def forward(ctx, x, rep):
        return x.gather(2, rep[:, None, :].expand_as(x))

    @staticmethod
    def backward(ctx, g):
        return g, None


def representatives(clouds):
    """[B, P]: for every point the index of the first point of its cloud whose input column [nfeat] is equal."""
    same = (clouds[:, :, :, None] == clouds[:, :, None, :]).all(1)
    return same.to(torch.int8).argmax(2)          # (argmax: the first of equal maxima)


def _pool(x, k, rep=None):
    """Max over the points of x [B, C, P]; the FIRST of equal values carries the gradient (torch's max_pool1d, the kernel)."""
    if rep is not None:
        x = _SameBits.apply(x, rep)
    eq = x == x.amax(2, keepdim=True)
    if k.get('all_maxima'):             # the value once, the gradient to every tied point
        v = x.amax(2).detach()
        return (x * eq).sum(2) - (eq.sum(2) - 1) * v
    if k.get('last_max_wins'):
        pick = eq & (eq.flip(2).cumsum(2).flip(2) == 1)
    else:
        pick = eq & (eq.cumsum(2) == 1)
    return (x * pick).sum(2)


def network(spec, P, clouds, glob, T, k):
    """spec: nfeat, nglob, conv, fc, n_group, last_ac.  P: {name: tensor}.  T: [B, 2, 2] (the full matrix) or None."""
    x, rep = clouds, representatives(clouds.detach())
    if T is not None:
        Tm = T.transpose(1, 2) if k.get('T_transposed_fwd') else T
        xy = x[:, :2, :].transpose(1, 2)
        xy = _TransformWrongBackward.apply(xy, Tm) if k.get('T_transposed_bwd') else torch.bmm(xy, Tm)
        x = torch.cat([xy.transpose(1, 2), x[:, 2:, :]], 1)
    G = spec['n_group']
    for l in range(len(spec['conv'])):
        x = _affine(x, P[f'conv{l}.weight'], P[f'conv{l}.bias'], k, True)
        x = _relu(_norm(x, G, P[f'conv{l}.gamma'], P[f'conv{l}.beta'], EPS, k), k)
    x = _pool(x, k, rep)
    if glob is not None:
        x = torch.cat([glob, x], 1) if k.get('globals_in_front') else torch.cat([x, glob], 1)
    nfc = len(spec['fc'])
    for j in range(nfc):
        x = _affine(x, P[f'fc{j}.weight'], P[f'fc{j}.bias'], k, False)
        if j + 1 < nfc or spec['last_ac']:
            x = _relu(_norm(x, G, P[f'fc{j}.gamma'], P[f'fc{j}.beta'], EPS, k), k)
    return x


def _param_weights(case, k):
    """w for the parameter gradients: rows of clouds that a broken run loop would lose are zeroed."""
    w, B = case['w'], case['B']
    if k.get('drop_partial_run') and B % RUN:
        w = w.clone()
        w[(B // RUN) * RUN:] = 0
    if k.get('drop_beyond_grid') and B > RUN * MAX_GRID:
        w = w.clone()
        w[RUN * MAX_GRID:] = 0
    return w


def _leaf(v, dtype):
    return v.detach().to(dtype).clone().requires_grad_(True)


def _finish(case, emb, P, inputs, dtype, k):
    """emb and the gradients of (emb * w).sum() wrt every parameter and every input of `inputs` {name: leaf}."""
    w = case['w'].to(dtype)
    names, leaves = list(inputs), list(inputs.values())
    pn, pl = list(P), list(P.values())
    gi = torch.autograd.grad((emb * w).sum(), leaves, retain_graph=True, allow_unused=True) if leaves else ()
    gp = torch.autograd.grad((emb * _param_weights(case, k).to(dtype)).sum(), pl, allow_unused=True)
    res = {'emb': emb.detach()}
    for n, g, v in list(zip(names, gi, leaves)) + list(zip(pn, gp, pl)):
        res['d_' + n] = torch.zeros_like(v) if g is None else g.detach()
    return res


def _knobs(restate, knobs):
    k = {n: v for n, v in knobs.items() if v}
    assert set(k) <= set(KNOBS), k
    if restate:
        k['restate'] = True
    return k


def gn_reference(case, dtype=torch.float64, restate=False, **knobs):
    """What ops.gn_forward / gn_backward compute for a case: emb [B, D] and the gradients of (emb * w).sum() wrt every
    parameter, the clouds (want_clouds), the global features (nglob > 0) and T (ext: case['T'] holds T - I, as the C ABI).
    restate (or any knob): GroupNorm from its formula, (x - mean) * rstd, instead of torch.nn.functional.group_norm."""
    k = _knobs(restate, knobs)
    P = {n: _leaf(v, dtype) for n, v in case['params'].items()}
    inputs = {}
    clouds = case['clouds'].to(dtype)
    if case['want_clouds']:
        clouds = inputs['clouds'] = _leaf(clouds, dtype)
    glob = None
    if case['nglob']:
        glob = inputs['glob'] = _leaf(case['glob'], dtype)
    T = None
    if case['ext']:
        inputs['T'] = _leaf(case['T'], dtype)
        T = inputs['T'].reshape(-1, 2, 2) + torch.eye(2, dtype=dtype)
    emb = network(case, P, clouds, glob, T, k)
    return _finish(case, emb, P, inputs, dtype, k)


def composed_reference(case, dtype=torch.float64, restate=False, **knobs):
    """LocalCloudEmbedder.run_batch (reference learning/pointnet.py:189-207, ptn_nfeat_stn = 2, stn_as_global = 1): T = STN(xy) + I,
    xy @ T, the global features extended by T's four entries, PointNet, L2 normalisation.  case['params'] holds 'stn.*' and
    'ptn.*'; gradients wrt every parameter, the clouds and the global features."""
    k = _knobs(restate, knobs)
    P = {n: _leaf(v, dtype) for n, v in case['params'].items()}
    sub = lambda pre: {n[len(pre):]: v for n, v in P.items() if n.startswith(pre)}
    inputs = {'clouds': _leaf(case['clouds'], dtype), 'glob': _leaf(case['glob'], dtype)}
    B = case['B']
    T = network(case['stn'], sub('stn.'), inputs['clouds'][:, :2, :], None, None, k).reshape(B, 2, 2) + torch.eye(2, dtype=dtype)
    glob = torch.cat([inputs['glob'], T.reshape(B, 4)], 1)
    emb = F.normalize(network(case['ptn'], sub('ptn.'), inputs['clouds'], glob, T, k))
    return _finish(case, emb, P, inputs, dtype, k)


# =====================================================================================================================
# the declared exceptions
# =====================================================================================================================
def layers_of(spec):
    """[(name, cin, cout, normalised, is_conv)] in the order of the network."""
    out, cin = [], spec['nfeat']
    for l, c in enumerate(spec['conv']):
        out.append((f'conv{l}', cin, c, True, True))
        cin = c
    cin += spec['nglob']
    for j, c in enumerate(spec['fc']):
        out.append((f'fc{j}', cin, c, j + 1 < len(spec['fc']) or bool(spec['last_ac']), False))
        cin = c
    return out


def declare(case):
    """-> (exact_zero, noise): the tensor names of the two exceptions, from the shape of the case alone."""
    L, G, npts = layers_of(case), case['n_group'], case['npts']
    one = [i for i, (_, _, cout, norm, conv) in enumerate(L) if norm and cout == G and (npts == 1 or not conv)]
    zero, noise = set(), set()
    if one:
        top = one[-1]
        zero |= {f'd_{L[top][0]}.{p}' for p in ('weight', 'bias', 'gamma')}
        for name, _, _, norm, _ in L[:top]:
            zero |= {f'd_{name}.{p}' for p in (('weight', 'bias', 'gamma', 'beta') if norm else ('weight', 'bias'))}
        if case['want_clouds']:
            zero.add('d_clouds')
        if case['ext']:
            zero.add('d_T')
        if case['nglob'] and not L[top][4]:
            zero.add('d_glob')
    for name, _, cout, norm, conv in L:
        if conv and cout == G and npts > 1 and f'd_{name}.bias' not in zero:
            noise.add(f'd_{name}.bias')
    return zero, noise


def gradient_scale(ref):
    return max(float(v.abs().max()) for n, v in ref.items() if n != 'emb')


def judge(case, got, ref):
    """{tensor: (worst |got - ref|, worst error / allowance)} under the bound and the two declared exceptions; a ratio above 1
    fails."""
    gmax = gradient_scale(ref)
    out = {}
    for n, r in ref.items():
        g = got[n].detach().double().cpu()
        if n in case['exact_zero']:
            err = float(g.abs().max())
            out[n] = (err, 0.0 if err == 0.0 and g.shape == r.shape else float('inf'))
        elif n in case['noise']:
            err = float(g.abs().max())
            out[n] = (err, err / (NOISE_FLOOR * gmax) if g.shape == r.shape else float('inf'))
        else:
            out[n] = bound_ratio(g, r)
    return out


_REFERENCES = {}


def reference(case):
    """The float64 reference of a case, computed once; the declared zeros checked (below 1e-12 of the largest gradient) and the
    exact_zero tensors set to exact zero."""
    if case['name'] not in _REFERENCES:
        # (one-element groups: from the formula, where x - mean is exactly 0; torch's CPU kernel folds the mean into a shift and
        # leaves rstd = 316 times a float64 rounding error there, more or less of it from one machine to the next)
        ref = (composed_reference if 'stn' in case else gn_reference)(case, torch.float64, restate=bool(case['exact_zero']))
        gmax = gradient_scale(ref)
        for n in case['exact_zero'] | case['noise']:
            assert float(ref[n].abs().max()) <= ZERO_CHECK * gmax, (case['name'], n, float(ref[n].abs().max()), gmax)
        for n in case['exact_zero']:
            ref[n] = torch.zeros_like(ref[n])
        _REFERENCES[case['name']] = ref
    return _REFERENCES[case['name']]


# =====================================================================================================================
# builders
# =====================================================================================================================
def make_params(g, spec, small_bias0=False, prefix=''):
    """float32 parameters: W ~ N(0, 1 / cin), b ~ 0.3 N(0, 1), gamma ~ 1 + 0.3 N(0, 1), beta ~ 0.3 N(0, 1).  Normalised layers of
    8 channels or more: channel 1 mod 4 has a negative gamma, channel 2 gamma = 0, channel 3 beta = -5 (dead at every point),
    channel 6 gamma = beta = 0 (pre-activation exactly 0).  small_bias0: the first convolution's bias is 1e-3 N(0, 1), so that
    a small cloud leaves its layer variance below eps."""
    P = {}
    for i, (name, cin, cout, norm, _) in enumerate(layers_of(spec)):
        P[f'{prefix}{name}.weight'] = torch.randn(cout, cin, generator=g) / cin ** 0.5
        P[f'{prefix}{name}.bias'] = torch.randn(cout, generator=g) * (1e-3 if small_bias0 and i == 0 else 0.3)
        if norm:
            gam, bet = 1 + 0.3 * torch.randn(cout, generator=g), 0.3 * torch.randn(cout, generator=g)
            if cout >= 8:
                gam[1::4] = -gam[1::4].abs()
                gam[2], bet[3] = 0.0, -5.0
                gam[6] = bet[6] = 0.0
            elif cout >= 2:
                gam[1] = -gam[1].abs()
            P[f'{prefix}{name}.gamma'], P[f'{prefix}{name}.beta'] = gam, bet
    return P


def make_clouds(g, B, nfeat, npts, shift, classes):
    """[B, nfeat, npts] float32; cloud b has the value class classes[(b + shift) mod len(classes)]."""
    x = torch.randn(B, nfeat, npts, generator=g)
    cls = []
    for b in range(B):
        c = classes[(b + shift) % len(classes)]
        cls.append(c)
        if c == 'identical':
            x[b] = x[b, :, :1]
        elif c == 'duplicate pairs':
            x[b, :, 1::2] = x[b, :, 0:2 * (npts // 2):2]
        elif c == 'zero':
            x[b] = 0.0
        elif c == '1e-3':
            x[b] *= 1e-3
        elif c == '1e3':
            x[b] *= 1e3
        elif c == 'offset 100':
            x[b, :3] += 100.0
    return x, cls


def _case(name, nfeat, nglob, npts, B, conv, fc, n_group=1, last_ac=0, ext=True, want_clouds=True, shift=0, classes=VALUE_CLASSES,
          small_bias0=True, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    c = dict(name=name, nfeat=nfeat, nglob=nglob, npts=npts, B=B, conv=list(conv), fc=list(fc), n_group=n_group, last_ac=int(last_ac),
             ext=bool(ext), want_clouds=bool(want_clouds), small_bias0=small_bias0)
    c['params'] = make_params(g, c, small_bias0)
    c['clouds'], c['classes'] = make_clouds(g, B, nfeat, npts, shift, classes)
    c['glob'] = torch.rand(B, nglob, generator=g) if nglob else None
    c['T'] = 0.3 * torch.randn(B, 4, generator=g) if ext else None
    c['w'] = torch.randn(B, fc[-1], generator=g)
    if B >= 4:
        c['w'][3::5] = 0.0          # clouds that nothing depends on
    c['exact_zero'], c['noise'] = declare(c)
    return c


DEFAULT = ([32, 128], [34, 32, 32, 4])
SMALL = ([4, 8], [4, 2])
# Groups of ONE channel over the points (n_group = width in the convolutions) remove any per-channel constant: a cloud offset by 100
# is then a true cancellation (x = 100 +- 1 in float32, the normalised value from the +- 1), and a cloud whose points are all equal
# has variance exactly 0 in every group.  Float32 torch on the CPU is 4 ... 2800 times the bound with those clouds, so the case with
# such groups goes without them (the reshaping the admission rule asks for); the other cases keep all seven classes.
PER_CHANNEL = ('unit', 'duplicate pairs', '1e-3', '1e3')


@functools.lru_cache(maxsize=None)
def cases():
    """The case table; every axis value of the issue is reached by at least one case (tests/test_groupnorm_cases.py asserts it)."""
    C = [
        # the default network of the learned partition at the three wave layouts of its backward
        _case('default npts16 B33', 6, 7, 16, 33, *DEFAULT, seed=1),
        _case('default npts33 B31', 6, 7, 33, 31, *DEFAULT, want_clouds=False, shift=1, seed=2),
        _case('default npts64 B2', 6, 7, 64, 2, *DEFAULT, shift=2, seed=3),
        _case('default npts1 B64', 6, 7, 1, 64, *DEFAULT, shift=3, seed=4),
        # one wave in both passes
        _case('wide npts64 B5', 16, 64, 64, 5, [64, 128], [128, 8], n_group=2, shift=4, seed=5),
        # widths that are no multiple of the tile, odd cin in both stacks
        _case('odd npts31 B32', 3, 1, 31, 32, [33, 65], [17, 5], shift=5, seed=6),
        _case('wide odd npts32 B64', 2, 0, 32, 64, [127, 128], [128, 33, 3], shift=6, seed=7),
        _case('thin npts63 B2', 2, 1, 63, 2, [1, 31, 64], [33, 1], ext=False, shift=2, seed=8),
        # the smallest networks; nfeat = 1 goes without the transform
        _case('1+1 npts2 B1', 1, 0, 2, 1, [4], [4], ext=False, shift=0, seed=9),
        _case('1+1 npts2 B1 dup', 1, 0, 2, 1, [4], [4], ext=False, shift=2, seed=10),
        _case('1+1 last_ac npts7 B33', 2, 1, 7, 33, [31], [8], last_ac=1, seed=11),
        _case('8+8 npts7 B33', 3, 1, 7, 33, [16] * 8, [16] * 7 + [3], want_clouds=False, ext=False, seed=12),
        # groups: two per layer; one per convolution channel (noise biases); one-element groups (exact zeros)
        _case('groups 2 npts8 B65', 6, 7, 8, 65, [16, 32], [32, 4], n_group=2, seed=13),
        _case('groups = width npts5 B31', 3, 1, 5, 31, [4, 4], [32, 3], n_group=4, classes=PER_CHANNEL, seed=14),
        _case('head group of 1, G4', 3, 1, 3, 7, [8, 16], [4, 3], n_group=4, seed=15),
        _case('head width 1', 3, 1, 3, 7, [4, 8], [1, 3], seed=16),
        _case('conv group of 1, npts1 B33', 3, 1, 1, 33, [4, 4], [32, 3], n_group=4, seed=17),
        # the backward's grid-stride loop: a second run for workgroup 0; a second run for 33 of them with a partial last one
        _case('small B8193', 2, 0, 3, 8193, *SMALL, seed=18),
        _case('small B8225', 2, 1, 3, 8225, *SMALL, ext=False, want_clouds=False, shift=1, seed=19),
    ]
    assert len({c['name'] for c in C}) == len(C)
    return C


@functools.lru_cache(maxsize=None)
def composed_cases():
    """LocalCloudEmbedder.run_batch: a stand-alone STN and a PointNet (the widths of the record's third model), duplicate points."""
    out = []
    for name, B, npts, G, seed in (('composed npts8 B9', 9, 8, 1, 30), ('composed groups 2 npts33 B33', 33, 33, 2, 32)):
        g = torch.Generator().manual_seed(1000 + seed)
        stn = dict(nfeat=2, nglob=0, conv=[8, 16], fc=[16, 16, 4], n_group=G, last_ac=0)
        ptn = dict(nfeat=3, nglob=6, conv=[16, 32], fc=[16, 16, 4], n_group=G, last_ac=0)
        c = dict(name=name, B=B, npts=npts, nfeat=3, nglob=2, stn=stn, ptn=ptn, n_group=G)
        c['params'] = {**make_params(g, stn, prefix='stn.'), **make_params(g, ptn, True, prefix='ptn.')}
        c['clouds'], c['classes'] = make_clouds(g, B, 3, npts, 2, VALUE_CLASSES)
        c['glob'] = torch.rand(B, 2, generator=g)
        c['w'] = torch.randn(B, 4, generator=g)
        c['w'][3::5] = 0.0
        c['exact_zero'], c['noise'] = set(), set()
        out.append(c)
    return out
