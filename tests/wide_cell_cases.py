"""Case builders and float64 references for the RNN-ECC kernels at the state widths 8, 16, 64 and 128 (csrc/spg_ecc_wide.hip): the
stand-alone GRU / LSTM cell and the recurrent module.  Plain module (no test in it): tests/test_wide_cell_cases.py admits the cases
and probes the knobs on the CPU, tests/test_gpu_wide_cell.py and tests/test_gpu_wide_eccrnn.py run the device against the references.

REFERENCES are the float64 evaluation of oracle/spg_oracle.py (gru_cell_ex, lstm_cell_ex, graph_network_forward -> rnn_graph_conv)
under torch autograd.  Every evaluator takes a dtype (float64: the reference; float32 on the CPU: the admission figure).  Nothing
here is derived from what the device returns.

BOUND.  conftest.assert_elementwise with its defaults, |a - ref| <= 1e-4 |ref| + 1e-5 max|ref| for every element.  A case is
admitted only if its float32 CPU evaluation stays within ADMIT = 0.25 of that bound on every compared tensor (the rule of
tests/op_cases.py).  The saturating row class has the scale 10 of tests/op_cases.py at 16, 64 and 128; at nc = 8 it did not pass
(GRU, no normalisation, input gate, 15 and 17 rows: the float32 CPU evaluation of d_ig.weight at 0.30 of the bound, a cancelling
sum over few rows) and its scale is 5 there (worst figure at 8 then: 0.05).  The bound is the same everywhere.

CELL CASES.  Both cells x the four widths x the four (layernorm, ingate) combinations x four row counts.  A workgroup of the wide
kernels owns BLOCK_NODES[nc] rows (16 at 8 and 16, 8 at 64, 4 at 128; the library answers the same through spg_cell_block_nodes and
the GPU test asserts that): cell_sizes(nc) = 1 row, one less and one more than a workgroup, and a few workgroups with a partial
last one -- (1, 15, 17, 50) at 8 and 16, (1, 7, 9, 26) at 64, (1, 3, 5, 22) at 128.  Row r has the class ROW_CLASSES[r mod 6] (unit,
1e-3, saturating, aggregate 0, hidden 0, both 0) and the cx class CX_CLASSES[(r div 6) mod 3] (0, unit, +-20), so 18 rows hold every
pair.  The LSTM cases pass an upstream gradient of cy except at the row count "one more than a workgroup" (grad_cy = None).

MODULE CASES.  graphnet.GraphNetwork of one recurrent token on the ladder graph of tests/ecc_cases.py at n = 200 (in- and
out-degrees 0 .. 13, 31 .. 33, 63 .. 65, 100, a self-loop, repeated edges, hubs; E = 1202): MODULE_CASES below.  The filter
network's ReLU near-ties are handled as in tests/ecc_cases.py (`dec` / `rec`).

KNOBS (keyword switches, all off by default; each restates one plausible kernel mistake).  tests/test_wide_cell_cases.py shows that
every one leaves the bound on at least one case."""
import dataclasses
import functools
import math

import torch

import ecc_cases as EC
from oracle import spg_oracle as O
from op_cases import ADMIT, ATOL_FRAC, RTOL, SAT_SCALE, assert_bound, bound_ratio, measure, worst  # noqa: F401  (re-exported for the tests)

WIDTHS = (8, 16, 64, 128)
BLOCK_NODES = {8: 16, 16: 16, 64: 8, 128: 4}          # nodes (rows) per workgroup, csrc/spg_ecc_wide.hip: WideBlock
ROW_CLASSES = ('unit', '1e-3', 'saturating', 'aggregate 0', 'hidden 0', 'both 0')
CX_CLASSES = ('0', 'unit', '+-20')
IG_CLOSED, IG_OPEN = (0, 1), (2, 3)                   # channels whose input-gate bias is -20 / +20
GATES = {'gru': 3, 'lstm': 4}
SAT = {8: 5.0, 16: SAT_SCALE, 64: SAT_SCALE, 128: SAT_SCALE}      # the saturating row scale per width (see BOUND above)

CELL_KNOBS = {
    'bias on the wrong side of the normalisation': dict(bias_wrong_side=True),
    'variance over nc instead of G nc': dict(var_over_nc=True),
    'unbiased variance': dict(unbiased=True),
    'gate chunks 64 apart instead of nc': dict(chunk64=True),
    'the last nc mod 64 channels dropped': dict(drop_tail=True),
}
MODULE_KNOBS = {'mean divided by the out-degree': dict(mean_by_outdeg=True)}


def cell_sizes(nc):
    nb = BLOCK_NODES[nc]
    return (1, nb - 1, nb + 1, max(3 * nb + 2, 22))


# =====================================================================================================================
# the cell
# =====================================================================================================================
def cell_params(kind, nc, layernorm, ingate):
    """float32 parameters, uniform +-1/sqrt(nc) as nn.RNNCellBase.reset_parameters draws them; ig.bias closed / open on 2 + 2 channels."""
    g = torch.Generator().manual_seed(5000 + 1000 * (kind == 'lstm') + 10 * nc + 2 * layernorm + ingate)
    gw = GATES[kind] * nc
    u = lambda *s: ((torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(nc)).float()
    P = {'weight_ih': u(gw, nc), 'weight_hh': u(gw, nc), 'bias_ih': u(gw), 'bias_hh': u(gw)}
    if ingate:
        P['ig.weight'], P['ig.bias'] = u(nc, nc), u(nc)
        P['ig.bias'][list(IG_CLOSED)] = -20.0
        P['ig.bias'][list(IG_OPEN)] = 20.0
    return P


@functools.lru_cache(maxsize=None)
def cell_rows(nc):
    """The 64 float32 rows of width nc: aggregate, hidden, cx, upstream gradients of hy and cy, and the class of every row."""
    g = torch.Generator().manual_seed(70 + nc)
    inp, hid, cx, gh, gc = [torch.randn(64, nc, generator=g) for _ in range(5)]
    sign = torch.where(torch.rand(64, nc, generator=g) < 0.5, -1.0, 1.0)
    cls, ccls = [], []
    for r in range(64):
        c, cc = ROW_CLASSES[r % 6], CX_CLASSES[(r // 6) % 3]
        s = {'unit': 1.0, '1e-3': 1e-3, 'saturating': SAT[nc]}.get(c, 1.0)
        inp[r] *= 0.0 if c in ('aggregate 0', 'both 0') else s
        hid[r] *= 0.0 if c in ('hidden 0', 'both 0') else s
        cx[r] = {'0': torch.zeros(nc), 'unit': cx[r], '+-20': 20.0 * sign[r]}[cc]
        cls.append(c); ccls.append(cc)
    return dict(inp=inp, hid=hid, cx=cx, gh=gh, gc=gc, row_class=cls, cx_class=ccls)


@functools.lru_cache(maxsize=None)
def cell_cases():
    out = []
    for kind in ('gru', 'lstm'):
        for nc in WIDTHS:
            rows = cell_rows(nc)
            for layernorm in (True, False):
                for ingate in (True, False):
                    P = cell_params(kind, nc, layernorm, ingate)
                    for n in cell_sizes(nc):
                        grad_cy = None if kind == 'gru' else n != BLOCK_NODES[nc] + 1
                        name = f'{kind} nc{nc} ln{int(layernorm)} ig{int(ingate)} n{n}' + ('' if grad_cy is None else (' dcy' if grad_cy else ' dcy=None'))
                        out.append(dict(name=name, kind=kind, nc=nc, layernorm=layernorm, ingate=ingate, n=n, grad_cy=grad_cy, params=P,
                                        **{k: rows[k][:n].contiguous() for k in ('inp', 'hid', 'cx', 'gh', 'gc')}))
    return out


def _row_norm(g, nc, unbiased, var_over_nc):
    mu = g.mean(1, keepdim=True)
    var = g.var(1, unbiased=unbiased, keepdim=True)
    if var_over_nc:                                       # the sum of squares divided by nc instead of by the G nc values of the row
        var = var * (g.shape[1] / nc)
    return (g - mu) / torch.sqrt(var + O.IN_EPS)


def _chunks(v, nc, n_gates, chunk64):
    """The gate chunks of [.., G nc]; chunk64: chunk k is read 64 k values in (wrapped into the row) instead of nc k."""
    if not chunk64:
        return v.chunk(n_gates, -1)
    gw = v.shape[-1]
    return [v[..., (torch.arange(nc) + 64 * k) % gw] for k in range(n_gates)]


def _drop_tail(v, nc, drop_tail):
    keep = nc - nc % 64 if drop_tail else nc
    return v if keep == nc else torch.cat([v[:, :keep], torch.zeros_like(v[:, keep:])], 1)


def gru_cell(inp, hidden, P, pfx, layernorm, ingate, bias_wrong_side=False, var_over_nc=False, unbiased=False, chunk64=False,
             drop_tail=False):
    """oracle.spg_oracle.gru_cell_ex with knobs (all off: the same expressions in the same order)."""
    dt, nc = inp.dtype, inp.shape[1]
    if ingate:
        inp = torch.sigmoid(hidden @ P[pfx + '.ig.weight'].to(dt).t() + P[pfx + '.ig.bias'].to(dt)) * inp
    gi = inp @ P[pfx + '.weight_ih'].to(dt).t()
    gh = hidden @ P[pfx + '.weight_hh'].to(dt).t()
    bih, bhh = P[pfx + '.bias_ih'].to(dt), P[pfx + '.bias_hh'].to(dt)
    if bias_wrong_side:                                   # the LSTM's placement: in front of the normalisation
        gi, gh = gi + bih, gh + bhh
        bih, bhh = torch.zeros_like(bih), torch.zeros_like(bhh)
    if layernorm:
        gi, gh = _row_norm(gi, nc, unbiased, var_over_nc), _row_norm(gh, nc, unbiased, var_over_nc)
    i_r, i_i, i_n = _chunks(gi, nc, 3, chunk64)
    h_r, h_i, h_n = _chunks(gh, nc, 3, chunk64)
    bih_r, bih_i, bih_n = _chunks(bih, nc, 3, chunk64)
    bhh_r, bhh_i, bhh_n = _chunks(bhh, nc, 3, chunk64)
    resetgate = torch.sigmoid(i_r + bih_r + h_r + bhh_r)
    inputgate = torch.sigmoid(i_i + bih_i + h_i + bhh_i)
    newgate = torch.tanh(i_n + bih_n + resetgate * (h_n + bhh_n))
    return _drop_tail(newgate + inputgate * (hidden - newgate), nc, drop_tail)


def lstm_cell(inp, hidden, P, pfx, layernorm, ingate, bias_wrong_side=False, var_over_nc=False, unbiased=False, chunk64=False,
              drop_tail=False):
    """oracle.spg_oracle.lstm_cell_ex with knobs (all off: the same expressions in the same order)."""
    hx, cx = hidden
    dt, nc = inp.dtype, inp.shape[1]
    if ingate:
        inp = torch.sigmoid(hx @ P[pfx + '.ig.weight'].to(dt).t() + P[pfx + '.ig.bias'].to(dt)) * inp
    gi, gh = inp @ P[pfx + '.weight_ih'].to(dt).t(), hx @ P[pfx + '.weight_hh'].to(dt).t()
    if not bias_wrong_side:
        gi, gh = gi + P[pfx + '.bias_ih'].to(dt), gh + P[pfx + '.bias_hh'].to(dt)
    if layernorm:
        gi, gh = _row_norm(gi, nc, unbiased, var_over_nc), _row_norm(gh, nc, unbiased, var_over_nc)
    if bias_wrong_side:                                   # the GRU's placement: behind the normalisation
        gi, gh = gi + P[pfx + '.bias_ih'].to(dt), gh + P[pfx + '.bias_hh'].to(dt)
    ig_, fg, cg, og = _chunks(gi + gh, nc, 4, chunk64)
    cy = torch.sigmoid(fg) * cx + torch.sigmoid(ig_) * torch.tanh(cg)
    hy = torch.sigmoid(og) * torch.tanh(cy)
    return _drop_tail(hy, nc, drop_tail), _drop_tail(cy, nc, drop_tail)


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
        g = P['c.' + k].grad
        res['d_' + k] = g if g is not None else torch.zeros_like(P['c.' + k])
    return {k: v.detach() for k, v in res.items()}


# =====================================================================================================================
# the recurrent module
# =====================================================================================================================
FNET = [13, 32, 128, 64]                     # edge features -> filter network widths; orthogonal init, no last-layer bias, BatchNorm at 2
GKEY = 200                                   # the ladder graph of tests/ecc_cases.py at its smallest size
# (cell, nc, matrix filters, nrepeats, cat_all, layernorm, ingate, training): GRU and LSTM; matrix filters at 8 and 64, vector filters
# at 16 and 128; nrepeats 1 and 3; cat_all on and off; one plain cell (no normalisation, no input gate); training and evaluation mode
MODULE_CASES = (
    ('gru', 8, True, 3, True, True, True, True),
    ('lstm', 8, True, 1, False, True, True, True),
    ('gru', 64, True, 1, False, True, True, True),
    ('lstm', 64, True, 3, True, True, True, True),
    ('gru', 16, False, 3, False, True, True, True),
    ('lstm', 16, False, 1, True, False, False, True),
    ('gru', 128, False, 3, True, True, True, True),
    ('lstm', 128, False, 3, False, True, True, True),
    ('gru', 64, True, 3, True, False, False, True),
    ('gru', 64, True, 3, True, True, True, False),
    ('lstm', 8, True, 3, False, True, True, False),
    ('gru', 16, False, 1, True, True, True, False),
    ('lstm', 128, False, 1, True, True, True, False),
)
NETWORK_CASE = ('gru_3_0,f_13', 64)          # GraphNetwork with the classifier behind the recurrence (HipLinear), training mode


def config_of(cell, nc, matrix, R, cat_all, layernorm, ingate):
    return f'{cell}_{R}_{int(not matrix)}_{int(layernorm)}_{int(ingate)}_{int(cat_all)}'


def module_spec(config, nc):
    base = O.ModelSpec()
    return dataclasses.replace(base, model_config=config, ptn_widths=(tuple(base.ptn_widths[0]), tuple(base.ptn_widths[1][:-1]) + (nc,)),
                               edge_feats=FNET[0], fnet_widths=tuple(FNET[1:]), fnet_llbias=0, fnet_orthoinit=1, fnet_bnidx=2)


@functools.lru_cache(maxsize=None)
def module_state(config, nc):
    """The float32 state_dict of graphnet.GraphNetwork for a configuration (its own initialisation, seed 7), keys prefixed 'ecc.'."""
    from superpoint_graph_amd.learning import graphnet
    with torch.random.fork_rng():
        torch.manual_seed(7)
        net = graphnet.GraphNetwork(config, nc, list(FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    return {'ecc.' + k: v.detach().clone() for k, v in net.state_dict().items()}


def out_width(config, nc):
    w = nc
    for _, kind, payload in O.parse_model_config(config, nc):
        if kind in ('gru', 'lstm') and payload[1].cat_all:
            w = payload[0] * (payload[1].nrepeats + 1)
        elif kind in ('gru', 'lstm'):
            w = payload[0]
        elif kind == 'f':
            w = payload[1]
    return w


@functools.lru_cache(maxsize=None)
def network_case(config, nc, training=True, gkey=GKEY):
    idxn, degs, _ = EC.graph(gkey)
    n, E = int(degs.numel()), int(idxn.numel())
    g = torch.Generator().manual_seed(29 + n + nc)
    x = torch.randn(n, nc, generator=g)
    ef = torch.randn(E, FNET[0], generator=g)
    go = torch.randn(n, out_width(config, nc), generator=g)
    return dict(name=f'{config} at width {nc}, graph {gkey}, ' + ('train' if training else 'eval'), config=config, nc=nc, gkey=gkey,
                training=training, x=x, edgefeats=ef, go=go)


def module_case(cell, nc, matrix, R, cat_all, layernorm, ingate, training):
    return network_case(config_of(cell, nc, matrix, R, cat_all, layernorm, ingate), nc, training)


def _mean_aggregate(hx, w, idxn, degs, divisor):
    """The in-edge mean of oracle.spg_oracle.ecc_forward with another divisor, plain autograd."""
    n = degs.numel()
    dst = torch.repeat_interleave(torch.arange(n), degs)
    sel = hx.index_select(0, idxn)
    prod = torch.bmm(sel.unsqueeze(1), w).squeeze(1) if w.dim() == 3 else sel * w
    out = torch.zeros(n, prod.shape[1], dtype=hx.dtype).index_add(0, dst, prod)
    return out / divisor.to(hx.dtype).unsqueeze(1)


def _forward_knobs(x, ef, idxn, degs, spec, P, training, dec, rec, nc, mean_by_outdeg=False):
    """oracle.spg_oracle.graph_network_forward for a single gru / lstm token with the aggregation restated."""
    (d, kind, payload), = O.parse_model_config(spec.model_config, nc)
    rs, pfx = payload[1], f'ecc.{d}'
    w = O.fnet_forward(ef.to(x.dtype), spec, nc if rs.vv else nc * nc, P, training, None, pfx + '._fnet', dec, rec)
    if not rs.vv:
        w = w.view(-1, nc, nc)
    outdeg = torch.bincount(idxn, minlength=degs.numel())
    div = (outdeg if mean_by_outdeg else degs).clamp(min=1)
    hx, hxs = x, [x]
    cx = torch.zeros_like(x) if rs.kind == 'lstm' else None
    for _ in range(rs.nrepeats):
        inp = _mean_aggregate(hx, w, idxn, degs, div)
        if rs.kind == 'lstm':
            hx, cx = O.lstm_cell_ex(inp, (hx, cx), P, pfx + '._cell', rs.layernorm, rs.ingate)
        else:
            hx = O.gru_cell_ex(inp, hx, P, pfx + '._cell', rs.layernorm, rs.ingate)
        hxs.append(hx)
    return torch.cat(hxs, 1) if rs.cat_all else hx


def module_eval(case, dtype=torch.float64, dec=None, rec=None, restated=False, **knobs):
    """-> {out, 'grad x', 'grad <parameter>' ...} in `dtype` on the CPU (evaluation mode: out only).  Without knobs:
    oracle.spg_oracle.graph_network_forward under torch autograd (restated=True: the knob path with every knob off).
    dec / rec: the ReLU decision hooks of the filter network."""
    idxn, degs, _ = EC.graph(case['gkey'])
    spec = module_spec(case['config'], case['nc'])
    P = {k: (v.to(dtype).clone().requires_grad_(True) if (O.is_param_key(k) and v.is_floating_point()) else v.clone())
         for k, v in module_state(case['config'], case['nc']).items()}
    x = case['x'].to(dtype).clone().requires_grad_(case['training'])
    ef = case['edgefeats'].to(dtype)
    if knobs or restated:
        out = _forward_knobs(x, ef, idxn, degs, spec, P, case['training'], dec, rec, case['nc'], **knobs)
    else:
        out = O.graph_network_forward(x, ef, idxn, degs, spec, P, case['training'], dec=dec, rec=rec)
    res = {'out': out.detach()}
    if case['training']:
        out.backward(case['go'].to(dtype))
        res['grad x'] = x.grad
        for k, v in P.items():
            if v.requires_grad:
                res['grad ' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return res


def compared(ref):
    """The tensors of a module result that are judged: out, grad x and every parameter gradient that conftest.noise_grad does not
    exclude on the float64 reference (the bias in front of the filter network's train-mode BatchNorm)."""
    from conftest import noise_grad
    pg = EC.param_grads(ref)
    return [k for k in ref if not (k.startswith('grad ecc.') and noise_grad(k[5:], pg))]


@functools.lru_cache(maxsize=None)
def module_reference(config, nc, training=True, gkey=GKEY):
    """The float64 reference of a module case with its own decisions, computed once: (results, recorded ReLU pre-activations)."""
    rec = {}
    return module_eval(network_case(config, nc, training, gkey), torch.float64, rec=rec), rec


def module_refs(case, dec):
    """The reference of every judged tensor: out from the unconditioned float64 reference, the gradients from the float64 backward
    with the ReLU decisions `dec` of the side under test (which may differ from the reference's own only on near-ties,
    ecc_cases.check_near_ties).  -> ({tensor: reference}, number of decisions that differ)."""
    free, rec = module_reference(case['config'], case['nc'], case['training'], case['gkey'])
    if not case['training']:
        return {'out': free['out']}, 0
    n_diff = EC.check_near_ties(dec, rec)
    cond = free if n_diff == 0 else module_eval(case, torch.float64, dec=dec)
    return {k: (free if k == 'out' else cond)[k] for k in compared(cond)}, n_diff
