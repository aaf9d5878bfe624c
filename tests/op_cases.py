"""Case builders and float64 references for the small operators of the training step at their edges: the GRU / LSTM cell
(csrc/spg_ecc.hip), the weighted cross entropy (csrc/spg_loss.hip), the clamp + Adam launch (spg_adam_clamp_kernel) and the
dense-layer backward family (spg_linear_dgrad, spg_colsum, spg_linear_wgrad_bias, spg_linear_backward).  Plain module (no test
in it): tests/test_op_cases.py checks the cases on the CPU, tests/test_gpu_op_edges.py runs the device against the references.

The bound is the project's contract, conftest.assert_elementwise with its defaults: |a - ref| <= 1e-4 |ref| + 1e-5 max|ref| for
EVERY element, NaN exactly where the reference has NaN.  A case is admitted only if the float32 CPU evaluation of the same
reference stays within ADMIT = 0.25 of that bound on every compared tensor (tests/test_op_cases.py): what a case demands of the
device, plain float32 arithmetic delivers four times over.  Nothing here is derived from what the device returns.

Every evaluator takes a dtype (float64: the reference; float32: the admission figure) and keyword knobs that are all off by
default.  A knob restates one plausible kernel mistake; tests/test_op_cases.py shows that every one of them leaves the bound on
at least one case, i.e. that the cases can tell a wrong kernel from a right one."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import spg_oracle as O

RTOL, ATOL_FRAC = 1e-4, 1e-5        # conftest.assert_elementwise's defaults
ADMIT = 0.25


def _t64(v):
    return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).detach().double().cpu()


def bound_ratio(a, ref):
    """-> (worst |a - ref|, worst |a - ref| / (RTOL |ref| + ATOL_FRAC max|ref|)) over all elements.  The ratio is inf when the
    shapes or the NaN positions differ, or where an element is off although its bound is 0."""
    a, ref = _t64(a), _t64(ref)
    if a.shape != ref.shape or not torch.equal(torch.isnan(a), torch.isnan(ref)):
        return math.inf, math.inf
    keep = ~torch.isnan(ref)
    if not bool(keep.any()):
        return 0.0, 0.0
    a, ref = a[keep], ref[keep]
    err = (a - ref).abs()
    bound = RTOL * ref.abs() + ATOL_FRAC * float(ref.abs().max())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(err.max()), float(ratio.max())


def assert_bound(a, ref, what):
    """conftest.assert_elementwise on every element; where the reference is NaN the value must be NaN, and nowhere else."""
    from conftest import assert_elementwise
    a, ref = _t64(a), _t64(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(a), nan), f'{what}: NaN positions differ from the reference'
    if bool((~nan).any()):
        assert_elementwise(a[~nan], ref[~nan], what=what)


def worst(figures):
    """The largest ratio of a {tensor: (abs, ratio)} dict."""
    return max(r for _, r in figures.values())


def measure(got, ref):
    """{tensor: bound_ratio} over the tensors of the reference."""
    return {k: bound_ratio(got[k], ref[k]) for k in ref}


# =====================================================================================================================
# GRU / LSTM cell
# =====================================================================================================================
CELL_SIZES = (1, 3, 5, 64)          # 4 nodes per workgroup: a lone wave, a partial group, one group + 1, 16 groups
SAT_SCALE = 10.0                    # the saturating row scale s (the admission rule decides how large it may be)
ROW_CLASSES = ('unit', '1e-2', '1e-3', 'saturating', 'aggregate 0', 'hidden 0', 'both 0')
CX_CLASSES = ('0', 'unit', '+-20')
ROW_PERM = np.random.default_rng(64).permutation(64)        # a case of n < 64 rows takes the first n rows of this order
IG_CLOSED, IG_OPEN = (0, 1), (2, 3)                          # channels whose input-gate bias is -20 / +20


def cell_params(kind, layernorm, ingate):
    """float32 parameters, uniform +-1/sqrt(32) as nn.RNNCellBase.reset_parameters draws them; ig.bias closed / open on 2 + 2 channels."""
    g = torch.Generator().manual_seed(1000 + 100 * (kind == 'lstm') + 10 * layernorm + ingate)
    gw = 96 if kind == 'gru' else 128
    u = lambda *s: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(32)).float()
    P = {'weight_ih': u(gw, 32), 'weight_hh': u(gw, 32), 'bias_ih': u(gw), 'bias_hh': u(gw)}
    if ingate:
        P['ig.weight'], P['ig.bias'] = u(32, 32), u(32)
        P['ig.bias'][list(IG_CLOSED)] = -20.0
        P['ig.bias'][list(IG_OPEN)] = 20.0
    return P


@functools.lru_cache(maxsize=None)
def cell_rows():
    """The 64 float32 rows (already in ROW_PERM order): aggregate, hidden, cx, upstream gradients of hy and cy, and the class of
    every row.  Row r of the unpermuted table has class r mod 7 and cx class r mod 3, so 64 rows hold every pair."""
    g = torch.Generator().manual_seed(7)
    inp, hid, cx, gh, gc = [torch.randn(64, 32, generator=g) for _ in range(5)]
    sign = torch.where(torch.rand(64, 32, generator=g) < 0.5, -1.0, 1.0)
    cls, ccls = [], []
    for r in range(64):
        c, cc = ROW_CLASSES[r % 7], CX_CLASSES[r % 3]
        s = {'unit': 1.0, '1e-2': 1e-2, '1e-3': 1e-3, 'saturating': SAT_SCALE}.get(c, 1.0)
        inp[r] *= 0.0 if c in ('aggregate 0', 'both 0') else s
        hid[r] *= 0.0 if c in ('hidden 0', 'both 0') else s
        cx[r] = {'0': torch.zeros(32), 'unit': cx[r], '+-20': 20.0 * sign[r]}[cc]
        cls.append(c); ccls.append(cc)
    p = torch.from_numpy(ROW_PERM)
    return dict(inp=inp[p].contiguous(), hid=hid[p].contiguous(), cx=cx[p].contiguous(), gh=gh[p].contiguous(), gc=gc[p].contiguous(),
                row_class=[cls[i] for i in ROW_PERM], cx_class=[ccls[i] for i in ROW_PERM])


@functools.lru_cache(maxsize=None)
def cell_cases():
    rows = cell_rows()
    out = []
    for kind in ('gru', 'lstm'):
        for layernorm in (True, False):
            for ingate in (True, False):
                P = cell_params(kind, layernorm, ingate)
                for n in CELL_SIZES:
                    for grad_cy in ((True, False) if kind == 'lstm' else (None,)):
                        name = f'{kind} ln{int(layernorm)} ig{int(ingate)} n{n}' + ('' if grad_cy is None else (' dcy' if grad_cy else ' dcy=None'))
                        out.append(dict(name=name, kind=kind, layernorm=layernorm, ingate=ingate, n=n, grad_cy=grad_cy, params=P,
                                        **{k: rows[k][:n] for k in ('inp', 'hid', 'cx', 'gh', 'gc')}))
    return out


def _row_norm(g, eps, unbiased):
    mu = g.mean(1, keepdim=True)
    var = g.var(1, unbiased=unbiased, keepdim=True)
    return (g - mu) / torch.sqrt(var + eps)


def gru_cell(inp, hidden, P, pfx, layernorm, ingate, eps=O.IN_EPS, unbiased=False, bias_before_norm=False, flip_sign=False):
    """oracle.spg_oracle.gru_cell_ex with knobs (all off: the same expressions in the same order)."""
    dt = inp.dtype
    if ingate:
        inp = torch.sigmoid(hidden @ P[pfx + '.ig.weight'].to(dt).t() + P[pfx + '.ig.bias'].to(dt)) * inp
    gi = inp @ P[pfx + '.weight_ih'].to(dt).t()
    gh = hidden @ P[pfx + '.weight_hh'].to(dt).t()
    bih, bhh = P[pfx + '.bias_ih'].to(dt), P[pfx + '.bias_hh'].to(dt)
    if bias_before_norm:
        gi, gh = gi + bih, gh + bhh
        bih, bhh = torch.zeros_like(bih), torch.zeros_like(bhh)
    if layernorm:
        gi, gh = _row_norm(gi, eps, unbiased), _row_norm(gh, eps, unbiased)
    i_r, i_i, i_n = gi.chunk(3, 1)
    h_r, h_i, h_n = gh.chunk(3, 1)
    bih_r, bih_i, bih_n = bih.chunk(3)
    bhh_r, bhh_i, bhh_n = bhh.chunk(3)
    resetgate = torch.sigmoid(i_r + bih_r + h_r + bhh_r)
    inputgate = torch.sigmoid(i_i + bih_i + h_i + bhh_i)
    newgate = torch.tanh(i_n + bih_n + resetgate * (h_n + bhh_n))
    return newgate + inputgate * ((newgate - hidden) if flip_sign else (hidden - newgate))


def lstm_cell(inp, hidden, P, pfx, layernorm, ingate, eps=O.IN_EPS, unbiased=False, bias_after_norm=False):
    """oracle.spg_oracle.lstm_cell_ex with knobs (all off: the same expressions in the same order)."""
    hx, cx = hidden
    dt = inp.dtype
    if ingate:
        inp = torch.sigmoid(hx @ P[pfx + '.ig.weight'].to(dt).t() + P[pfx + '.ig.bias'].to(dt)) * inp
    if bias_after_norm:
        gi, gh = inp @ P[pfx + '.weight_ih'].to(dt).t(), hx @ P[pfx + '.weight_hh'].to(dt).t()
    else:
        gi = inp @ P[pfx + '.weight_ih'].to(dt).t() + P[pfx + '.bias_ih'].to(dt)
        gh = hx @ P[pfx + '.weight_hh'].to(dt).t() + P[pfx + '.bias_hh'].to(dt)
    if layernorm:
        gi, gh = _row_norm(gi, eps, unbiased), _row_norm(gh, eps, unbiased)
    if bias_after_norm:
        gi, gh = gi + P[pfx + '.bias_ih'].to(dt), gh + P[pfx + '.bias_hh'].to(dt)
    ig_, fg, cg, og = (gi + gh).chunk(4, 1)
    cy = torch.sigmoid(fg) * cx + torch.sigmoid(ig_) * torch.tanh(cg)
    hy = torch.sigmoid(og) * torch.tanh(cy)
    return hy, cy


def cell_eval(case, dtype=torch.float64, **knobs):
    """Outputs, input gradients and every parameter gradient of a cell case in `dtype` on the CPU.  Without knobs: the oracle
    (oracle.spg_oracle.gru_cell_ex / lstm_cell_ex) under torch autograd."""
    P = {'c.' + k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in case['params'].items()}
    inp, hid, cx = [case[k].detach().to(dtype).clone().requires_grad_(True) for k in ('inp', 'hid', 'cx')]
    ln, ig = case['layernorm'], case['ingate']
    if case['kind'] == 'gru':
        hy = gru_cell(inp, hid, P, 'c', ln, ig, **knobs) if knobs else O.gru_cell_ex(inp, hid, P, 'c', ln, ig)
        hy.backward(case['gh'].to(dtype))
        res = {'hy': hy, 'd_input': inp.grad, 'd_hidden': hid.grad}
    else:
        hy, cy = lstm_cell(inp, (hid, cx), P, 'c', ln, ig, **knobs) if knobs else O.lstm_cell_ex(inp, (hid, cx), P, 'c', ln, ig)
        if case['grad_cy']:
            torch.autograd.backward([hy, cy], [case['gh'].to(dtype), case['gc'].to(dtype)])
        else:
            hy.backward(case['gh'].to(dtype))
        res = {'hy': hy, 'cy': cy, 'd_input': inp.grad, 'd_hidden': hid.grad, 'd_cx': cx.grad}
    for k in case['params']:
        res['d_' + k] = P['c.' + k].grad
    return {k: v.detach() for k, v in res.items()}


# =====================================================================================================================
# weighted cross entropy
# =====================================================================================================================
CE_SHAPES = ((1, 1), (1, 13), (63, 13), (64, 13), (65, 13), (1023, 8), (1024, 8), (1025, 8), (130, 64))   # 64-row tiles, 1024-row stride
CE_LOGIT_CLASSES = ('spread 3', 'spread 3 + 1e4', 'spread 100 - 3e4', 'one -inf')
CE_TARGETS = ('10% ignored', 'one labelled', 'all ignored')
CE_WEIGHTS = ('none', 'random', 'zero class')
CE_UPSTREAM = (1.7, 0.0, -2.0)
IGNORE = -100


def _ce_case(N, C, k, targets, weights, reduction, upstream, bad=None):
    g = torch.Generator().manual_seed(31 * N + C + 7 * k)
    zero_class = C - 1 if weights == 'zero class' else None
    t = torch.randint(0, C, (N,), generator=g)
    if zero_class is not None:                      # rows r = 1 mod 3 carry the zero-weight class, no other row does
        t[t == zero_class] = 0
        t[1::3] = zero_class
    if targets == '10% ignored':
        t[torch.rand(N, generator=g) < 0.1] = IGNORE
        t[0] = 0                                   # at least one labelled row with a non-zero weight
    elif targets == 'one labelled':
        keep = N // 2 if zero_class is None else 3 * (N // 6)       # a row that does not carry the zero-weight class
        lab = int(t[keep])
        t[:] = IGNORE
        t[keep] = lab
    else:
        t[:] = IGNORE
    if bad is not None:
        t[N // 3] = t[2 * N // 3] = bad
    w = None
    if weights != 'none':
        w = torch.rand(C, generator=g) + 0.5
        if zero_class is not None:
            w[zero_class] = 0.0
    rc = (torch.arange(N) + k) % 4                   # row r has the logit class CE_LOGIT_CLASSES[(r + k) mod 4]
    x = torch.randn(N, C, generator=g) * torch.tensor([3.0, 3.0, 100.0, 3.0])[rc][:, None] + torch.tensor([0.0, 1e4, -3e4, 0.0])[rc][:, None]
    if C > 1:
        rows = torch.nonzero(rc == 3)[:, 0]
        col = torch.where((t >= 0) & (t < C), (t + 1) % C, torch.zeros_like(t))        # never the target's own entry
        x[rows, col[rows]] = -math.inf
    name = f'N{N} C{C} {targets}, weight {weights}, {reduction}, upstream {upstream:g}' + ('' if bad is None else f', two targets of {bad}')
    return dict(name=name, N=N, C=C, logits=x, target=t, weight=w, reduction=reduction, upstream=upstream, bad=bad is not None)


@functools.lru_cache(maxsize=None)
def ce_cases():
    """Every shape with every (targets, weights, reduction); the upstream gradient and the logit class of row 0 cycle.  A zero
    class weight `among labelled rows of other classes` needs two rows and two classes, so (1, 1) and (1, 13) go without it."""
    out, k = [], 0
    for N, C in CE_SHAPES:
        for targets in CE_TARGETS:
            for weights in CE_WEIGHTS:
                if weights == 'zero class' and (N < 6 or C < 2):
                    continue
                for reduction in ('mean', 'sum'):
                    out.append(_ce_case(N, C, k, targets, weights, reduction, CE_UPSTREAM[k % 3]))
                    k += 1
    # class indices outside [0, C) that are not ignore_index (spg_loss.hip: the loss becomes NaN, their gradient rows are 0)
    out.append(_ce_case(65, 13, k, '10% ignored', 'random', 'mean', 1.7, bad=13))
    out.append(_ce_case(65, 13, k + 1, '10% ignored', 'random', 'mean', 1.7, bad=-1))
    return out


def _ce_valid(case):
    t = case['target']
    return (t != IGNORE) & (t >= 0) & (t < case['C'])


def ce_reference(case, dtype=torch.float64):
    """torch.nn.functional.cross_entropy on the CPU on the float32 logits converted to `dtype`: loss, gradient of
    upstream * loss, normaliser (sum of the class weights of the labelled rows).  Rows with a class index outside [0, C) count
    as ignored for gradient and normaliser; the loss is then NaN (csrc/spg_loss.hip)."""
    x = case['logits'].detach().to(dtype).clone().requires_grad_(True)
    w = None if case['weight'] is None else case['weight'].to(dtype)
    valid = _ce_valid(case)
    t = torch.where(valid, case['target'], torch.full_like(case['target'], IGNORE))
    loss = F.cross_entropy(x, t, weight=w, reduction=case['reduction'])
    (loss * case['upstream']).backward()
    norm = (torch.ones(case['C'], dtype=dtype) if w is None else w)[t[valid]].sum()
    if case['bad']:
        loss = torch.full_like(loss, math.nan)
    return {'loss': loss.detach(), 'grad': x.grad, 'normaliser': norm}


def ce_restatement(case, dtype=torch.float32, max_subtraction=True, normaliser='weights', lse_first=False):
    """The same three results from the formulas, with knobs: max_subtraction=False: log sum exp(x) as it stands;
    normaliser='rows': `mean` divides by the number of labelled rows; lse_first=True: the log-probability as x - (m + log s)
    with the log-sum-exp rounded to `dtype` first, instead of (x - m) - log s."""
    x = case['logits'].to(dtype)
    N, C = x.shape
    valid = _ce_valid(case)
    tc = case['target'].clamp(0, C - 1)
    m = x.max(1, keepdim=True).values if max_subtraction else torch.zeros(N, 1, dtype=dtype)
    s = torch.exp(x - m).sum(1, keepdim=True)
    lp = x - (m + torch.log(s)) if lse_first else (x - m) - torch.log(s)
    w = (torch.ones(C, dtype=dtype) if case['weight'] is None else case['weight'].to(dtype))[tc]
    w = torch.where(valid, w, torch.zeros_like(w))
    nll = -lp.gather(1, tc[:, None])[:, 0]
    num = torch.where(valid, w * nll, torch.zeros_like(nll)).sum()
    wsum = w.sum()
    mean = case['reduction'] == 'mean'
    den = (wsum if normaliser == 'weights' else valid.sum().to(dtype)) if mean else torch.ones((), dtype=dtype)
    loss = num / den
    if case['bad']:
        loss = torch.full_like(loss, math.nan)
    scale = case['upstream'] * w / den
    onehot = F.one_hot(tc, C).to(dtype)
    grad = torch.where(valid[:, None], scale[:, None] * (torch.exp(lp) - onehot), torch.zeros_like(x))
    return {'loss': loss, 'grad': grad, 'normaliser': wsum}


# =====================================================================================================================
# clamp + Adam
# =====================================================================================================================
ADAM_SIZES = (1, 255, 256, 257, 1025)                 # 256 threads per block
ADAM_HYPER = ((0.0, 0.0, None), (1e-3, 0.5, None), (0.0, 1.0, 3.7), (1e-2, 0.5, 0.25))      # (weight_decay, grad_clip, grad_div)
ADAM_STEPS = (1, 1000)
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-2, (0.9, 0.999), 1e-8


@functools.lru_cache(maxsize=None)
def adam_cases():
    """Element i: i = 0 mod 8 has a gradient of magnitude 10^U(-15, 2); the other seven residues hold 0, +-c, +-c d (the clip
    after the division) and two values beyond it (c = grad_clip or 0.5, d = grad_div or 1).  Odd elements have p = 0 exactly (their
    new value IS minus the update), even ones a unit Gaussian p (weight decay enters the moments).  Step 1 starts from zero
    moments, step 1000 from non-zero ones."""
    out = []
    for n in ADAM_SIZES:
        for h, (wd, clip, div) in enumerate(ADAM_HYPER):
            for step in ADAM_STEPS:
                g = torch.Generator().manual_seed(17 * n + 3 * h + step)
                c, d = (clip or 0.5), (div or 1.0)
                grad = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 17 - 15) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
                special = torch.tensor([0.0, c, -c, c * d, -c * d, 3 * c * d, -10 * c * d], dtype=torch.float64)
                idx = torch.arange(n)
                grad = torch.where(idx % 8 == 0, grad, special[(idx % 8 - 1).clamp(min=0)]).float()
                p = torch.randn(n, generator=g)
                p[1::2] = 0.0
                if step == 1:
                    m, v = torch.zeros(n), torch.zeros(n)
                else:
                    m = 0.1 * torch.randn(n, generator=g) * grad.abs().clamp(min=1e-3, max=c)
                    v = m * m * (0.5 + 1.5 * torch.rand(n, generator=g))
                name = f'n{n} wd {wd:g} clip {clip:g} div {div} step {step}'
                out.append(dict(name=name, n=n, wd=wd, clip=clip, div=None if div is None else torch.tensor([div], dtype=torch.float32),
                                step=step, p=p, g=grad, m=m, v=v))
    return out


def adam_eval(case, dtype=torch.float64, wd_before_clamp=False, div_after_clamp=False, eps_inside_sqrt=False, bias_correction=True):
    """One step of the reference loop (learning/main.py: p.grad.clamp_, then torch.optim.Adam.step): the gradient is divided by
    grad_div and clamped (that is what stays in p.grad), weight decay is added to the clamped gradient, exp_avg.lerp_,
    exp_avg_sq.mul_().addcmul_(), denom = sqrt(v) / sqrt(1 - beta2^t) + eps, p -= lr / (1 - beta1^t) * m / denom.  The
    hyper-parameters are Python doubles, as torch.optim holds them.  p is returned in its two halves, so that the exact-zero
    half is judged against its own largest update and not against the Gaussian half's |p|."""
    p, g, m, v = [case[k].to(dtype).clone() for k in ('p', 'g', 'm', 'v')]
    wd, clip, t = case['wd'], case['clip'], case['step']
    b1, b2 = ADAM_BETAS
    div = None if case['div'] is None else case['div'].to(dtype)
    if div is not None and not div_after_clamp:
        g = g / div
    if wd_before_clamp and wd != 0:
        g = g + wd * p
    if clip > 0:
        g = g.clamp(-clip, clip)
    if div is not None and div_after_clamp:
        g = g / div
    stored = g.clone()
    if wd != 0 and not wd_before_clamp:
        g = g + wd * p
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    bc1, bc2 = (1 - b1 ** t, 1 - b2 ** t) if bias_correction else (1.0, 1.0)
    denom = torch.sqrt(v / bc2 + ADAM_EPS) if eps_inside_sqrt else v.sqrt() / math.sqrt(bc2) + ADAM_EPS
    p = p - (ADAM_LR / bc1) * (m / denom)
    return split_adam(p, stored, m, v)


def split_adam(p, g, m, v):
    return {'p (p was 0)': p[1::2], 'p (p Gaussian)': p[0::2], 'g': g, 'm': m, 'v': v}


# =====================================================================================================================
# dense-layer backward
# =====================================================================================================================
DENSE_SHAPES = ((1, 64, 32), (15, 13, 32), (16, 96, 32), (17, 13, 32), (1024, 96, 32), (1025, 96, 32), (129, 352, 64), (300, 1024, 64))   # (M, N, K)


@functools.lru_cache(maxsize=None)
def dense_cases():
    """y = x w^T + b with x [M, K], w [N, K], upstream dy [M, N]; spg_colsum takes M = 1, 15, 16, 17 (one slice, fewer / as many /
    more rows than its 16 row groups) and 1024, 1025 (64 slices of 16, then of 17 rows with a short last slice)."""
    out = []
    for M, N, K in DENSE_SHAPES:
        g = torch.Generator().manual_seed(M + 3 * N + 5 * K)
        out.append(dict(name=f'M{M} N{N} K{K}', M=M, N=N, K=K, dy=torch.randn(M, N, generator=g), x=torch.randn(M, K, generator=g),
                        w=torch.randn(N, K, generator=g) / K ** 0.5))
    return out


def dense_eval(case, dtype=torch.float64, drop_partial_group=False):
    """dx = dy w, dW = dy^T x, dbias = column sums of dy.  drop_partial_group: a column sum that loses the rows behind the last
    full group of 16."""
    dy, x, w = [case[k].to(dtype) for k in ('dy', 'x', 'w')]
    rows = (case['M'] // 16) * 16 if drop_partial_group else case['M']
    return {'dx': dy @ w, 'dW': dy.t() @ x, 'dbias': dy[:rows].sum(0)}
