"""GPU: the recurrent graph convolution at the state widths 8, 16, 64 and 128 (csrc/spg_ecc_wide.hip behind spg_eccrnn_forward /
spg_eccrnn_backward), element by element against oracle.spg_oracle.rnn_graph_conv in float64 (tests/wide_cell_cases.py, whose cases
tests/test_wide_cell_cases.py admits on the CPU):

a. graphnet.GraphNetwork of one recurrent token on the ladder graph of tests/ecc_cases.py at n = 200 (in- and out-degrees 0 .. 13,
   31 .. 33, 63 .. 65, 100, a self-loop, repeated edges, hubs): GRU and LSTM, matrix filters at 8 and 64, vector filters at 16 and 128,
   nrepeats 1 and 3, cat_all on and off, training mode (filter-network BatchNorm over E) and evaluation mode
   (wide_cell_cases.MODULE_CASES).  Compared under conftest.assert_elementwise: the output (against the reference with its own
   decisions), grad_h0 and every filter-network and cell parameter gradient that conftest.noise_grad does not exclude (against the
   float64 backward with the DEVICE's filter-network ReLU decisions, which may differ from the reference's own only on near-ties).
   A second run is bit-identical.
b. an edge-less graph: zero aggregates (the output is the cell iterated on a zero input) and exactly zero filter-network gradients.
c. GraphNetwork('gru_3_0,f_13', 64, ...): the classifier behind the recurrence runs on HipLinear.
d. one FlatParameters training step of PointNet + 'gru_3_1,f_8' at width 16: fused.supports(model) is False, the loss and all
   gradients match oracle.train_step in float64 (with the device's ReLU / max-pool decisions) inside the contract, and the gradients
   are views of the arena.
e. refusals, each a NotImplementedError before any launch: width 24, matrix filters at 128, GRUCellEx(64, 32).

`python tests/test_gpu_wide_eccrnn.py` prints the measured figures (profiles/wide_cell_errors.txt)."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the repository root on sys.path when this file is run as a script)
import ecc_cases as EC
import wide_cell_cases as C
from oracle import spg_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def run_network(case):
    """-> ({out, 'grad x', 'grad ecc.<parameter>'} on the host, the device's filter-network ReLU decisions or None in evaluation mode)."""
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import ecc, graphnet
    from test_gpu_baseline_parity import _hip_fnet_decisions
    idxn, degs, _ = EC.graph(case['gkey'])
    net = graphnet.GraphNetwork(case['config'], case['nc'], list(C.FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    net.load_state_dict({k[4:]: v for k, v in C.module_state(case['config'], case['nc']).items()})
    net = net.to(DEV)
    net.train(case['training'])
    gi = ecc.GraphConvInfo.from_buffers(idxn.clone(), degs.clone(), case['edgefeats'].clone(), None, None)
    captured = {}
    real = ops.eccrnn_forward

    def spy(*a, **kw):
        out = real(*a, **kw)
        captured['ecc'] = out[1]
        return out
    ops.eccrnn_forward = spy
    try:
        net.set_info([gi], 1)
        if not case['training']:
            with torch.no_grad():
                res, dec = {'out': net(case['x'].to(DEV))}, None
        else:
            xg = case['x'].to(DEV).requires_grad_(True)
            out = net(xg)
            out.backward(case['go'].to(DEV))
            res = {'out': out.detach(), 'grad x': xg.grad}
            res.update({'grad ecc.' + k: p.grad for k, p in net.named_parameters()})
        torch.cuda.synchronize()
        if case['training']:
            dec = _hip_fnet_decisions(captured['ecc'], C.module_spec(case['config'], case['nc']))
    finally:
        ops.eccrnn_forward = real
    return {k: v.detach().cpu() for k, v in res.items()}, dec


def judge(case):
    got, dec = run_network(case)
    refs, n_diff = C.module_refs(case, dec)
    fig = {k: C.bound_ratio(got[k], r) for k, r in refs.items()}
    for k, (err, ratio) in fig.items():
        print(f"{case['name']}: {k}: worst error {err:.3e}, {ratio:.3f} of the bound")
    print(f"{case['name']}: {n_diff} ReLU decisions differ from the float64 reference")
    for k, r in refs.items():
        C.assert_bound(got[k], r, f"{case['name']}: {k}")
    if case['training']:
        assert 'grad x' in refs and len(refs) >= len(got) - 1
        for k in set(got) - set(refs):              # the bias in front of the filter network's train-mode BatchNorm
            assert k == 'grad ecc.0._fnet.4.bias' and float(got[k].abs().max()) < 1e-5, k
    again, _ = run_network(case)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{case['name']}: {k} differs between two runs"
    return fig, n_diff


@pytest.mark.parametrize('args', C.MODULE_CASES, ids=lambda a: '-'.join(str(v) for v in a))
def test_module_on_the_ladder_graph(hip, args):
    judge(C.module_case(*args))


def test_network_with_classifier_at_64(hip):
    """GraphNetwork('gru_3_0,f_13', 64, ...): the recurrence (matrix filters, all states concatenated: 256 columns) feeds HipLinear."""
    from superpoint_graph_amd.learning import graphnet
    from superpoint_graph_amd.learning.modules import HipLinear
    config, nc = C.NETWORK_CASE
    net = graphnet.GraphNetwork(config, nc, list(C.FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    fc = list(net.children())[1]
    assert isinstance(fc, HipLinear) and fc.in_features == 4 * nc and fc._kernel_shape_ok()
    fig, _ = judge(C.network_case(config, nc, True))
    assert 'grad ecc.1.weight' in fig and 'grad ecc.1.bias' in fig


def test_edge_less_graph(hip):
    """No edges: every aggregate is zero (the output is the cell iterated on a zero input), the filter network receives exactly zero."""
    from superpoint_graph_amd.learning import ecc, graphnet
    nc, n, config = 16, 19, 'gru_3_1_1_1_1'
    state = C.module_state(config, nc)
    net = graphnet.GraphNetwork(config, nc, list(C.FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1)
    net.load_state_dict({k[4:]: v for k, v in state.items()})
    net = net.to(DEV).train()
    g = torch.Generator().manual_seed(3)
    x, go = torch.randn(n, nc, generator=g), torch.randn(n, 4 * nc, generator=g)
    gi = ecc.GraphConvInfo.from_buffers(torch.zeros(0, dtype=torch.int64), torch.zeros(n, dtype=torch.int64), torch.zeros(0, C.FNET[0]), None, None)
    net.set_info([gi], 1)
    xg = x.to(DEV).requires_grad_(True)
    out = net(xg)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    P = {k: (v.double().clone().requires_grad_(True) if O.is_param_key(k) else v.clone()) for k, v in state.items()}
    x64 = x.double().clone().requires_grad_(True)
    hx, hxs = x64, [x64]
    for _ in range(3):
        hx = O.gru_cell_ex(torch.zeros_like(hx), hx, P, 'ecc.0._cell', True, True)
        hxs.append(hx)
    ref = torch.cat(hxs, 1)
    ref.backward(go.double())
    C.assert_bound(out, ref, 'edge-less: out')
    C.assert_bound(xg.grad, x64.grad, 'edge-less: grad x')
    for k, p in net.named_parameters():
        if '_fnet' in k:
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k
        elif k.endswith('weight_ih'):               # the gated input is zero: so is the gradient of W_ih
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            C.assert_bound(p.grad, P['ecc.' + k].grad, 'edge-less: grad ' + k)


def test_flat_parameters_training_step_at_16(hip, monkeypatch):
    """learning/main.py's module path with the flat arena at a width the fused step does not serve."""
    from conftest import build_model, load_golden, noise_grad
    from superpoint_graph_amd import fused, ops
    from superpoint_graph_amd.flat import FlatParameters
    from test_gpu_baseline_parity import _hip_decisions, _hip_fnet_decisions
    from test_gpu_model import _run
    spec0, batch, _, g = load_golden('vector_gru4_small')
    spec = dataclasses.replace(spec0, model_config='gru_3_1,f_8', ptn_widths=(tuple(spec0.ptn_widths[0]), tuple(spec0.ptn_widths[1][:-1]) + (16,)))
    with torch.random.fork_rng():
        torch.manual_seed(11)
        state0 = {k: v.detach().clone() for k, v in build_model(spec).state_dict().items()}
    model = build_model(spec, state0).to(DEV).train()
    assert model.ecc.gconvs[0]._cell.hidden_size == 16
    assert fused.supports(model) is False
    arena = FlatParameters(model, lazy_zero=True, host_counters=True)
    captured = {}
    real_ptn, real_ecc = ops.pointnet_forward, ops.eccrnn_forward

    def spy_ptn(*a, **kw):
        out = real_ptn(*a, **kw)
        captured['state'] = out[1]
        return out

    def spy_ecc(*a, **kw):
        out = real_ecc(*a, **kw)
        captured['ecc'] = out[1]
        return out
    monkeypatch.setattr(ops, 'pointnet_forward', spy_ptn)
    monkeypatch.setattr(ops, 'eccrnn_forward', spy_ecc)
    cw = torch.from_numpy(g['class_weights'])
    arena.zero_grad()
    emb, logits, embedder = _run(model, batch)
    loss = F.cross_entropy(logits, batch['label_mode'].to(DEV), weight=cw.to(DEV))
    loss.backward()
    embedder.bw_hook()
    torch.cuda.synchronize()
    dec = _hip_decisions(model.ptn, captured['state'])
    dec.update(_hip_fnet_decisions(captured['ecc'], spec))
    st = {k: v.clone() for k, v in state0.items()}
    rec = {}
    loss_ref, logits_ref, _, grads_ref = O.train_step(batch, spec, st, cw, dtype=torch.float64, update_running_stats=False, dec=dec, rec=rec)
    for key, d in dec.items():                      # the device's decisions differ from float64's own only on near-ties
        if key.endswith('.pool'):
            h = rec[key]
            gap = h.max(1)[0] - h.gather(1, d.unsqueeze(1)).squeeze(1)
            assert float(gap.max()) <= 1e-4 * float(h.abs().max()), key
        else:
            v = rec[key].reshape(d.shape)
            differ = (v > 0) != d
            assert (float(v[differ].abs().max()) if bool(differ.any()) else 0.0) <= 1e-4 * float(v.abs().max()), key
    C.assert_bound(loss, loss_ref, 'loss')
    C.assert_bound(logits, logits_ref, 'logits')
    lo, hi = arena.flat.grad.data_ptr(), arena.flat.grad.data_ptr() + 4 * arena.flat.grad.numel()
    for k, p in model.named_parameters():
        assert p.grad is not None and lo <= p.grad.data_ptr() < hi, f'{k}: the gradient is not a view of the arena'
        if noise_grad(k, grads_ref):
            assert float(p.grad.abs().max()) < 1e-5, k
        else:
            print(f'{k}: {C.bound_ratio(p.grad, grads_ref[k])[1]:.3f} of the bound')
            C.assert_bound(p.grad, grads_ref[k], 'grad ' + k)


def test_refusals(hip, monkeypatch):
    """Width 24, matrix filters at 128 and GRUCellEx(64, 32) raise NotImplementedError before anything is launched."""
    from superpoint_graph_amd import _lib, ops
    from superpoint_graph_amd.learning import ecc, graphnet
    from superpoint_graph_amd.learning.modules import GRUCellEx, LSTMCellEx
    L = _lib.lib()
    launched = []
    for name in ('spg_eccrnn_forward', 'spg_cell_fwd', 'spg_gru_cell_fwd', 'spg_lstm_cell_fwd', 'spg_eccrnn_workspace_bytes'):
        real = getattr(L, name)
        monkeypatch.setattr(L, name, (lambda *a, _n=name, _r=real: (launched.append(_n), _r(*a))[1]))
    idxn, degs, _ = EC.graph(5)
    E = int(idxn.numel())

    def forward(config, nc):
        net = graphnet.GraphNetwork(config, nc, list(C.FNET), 1, 0, 2, 30000, use_pyg=0, cuda=1).to(DEV)
        net.set_info([ecc.GraphConvInfo.from_buffers(idxn.clone(), degs.clone(), torch.randn(E, C.FNET[0]), None, None)], 1)
        return net(torch.randn(5, nc, device=DEV))
    with pytest.raises(NotImplementedError, match='8, 16, 32, 64'):
        forward('gru_2_1', 24)
    with pytest.raises(NotImplementedError, match='8, 16, 32, 64'):
        forward('lstm_2_0', 24)
    with pytest.raises(NotImplementedError, match='matrix filters'):
        forward('gru_2_0', 128)
    with pytest.raises(NotImplementedError, match='input_size == hidden_size'):
        GRUCellEx(64, 32).to(DEV)(torch.randn(3, 64, device=DEV), torch.randn(3, 32, device=DEV))
    with pytest.raises(NotImplementedError, match='8, 16, 32, 64'):
        LSTMCellEx(24, 24).to(DEV)(torch.randn(3, 24, device=DEV), (torch.randn(3, 24, device=DEV), torch.randn(3, 24, device=DEV)))
    with pytest.raises(NotImplementedError, match='bias'):
        GRUCellEx(16, 16, bias=False).to(DEV)(torch.randn(3, 16, device=DEV), torch.randn(3, 16, device=DEV))
    assert launched == []
    # the library refuses the same on its own: -2 / 0 and a message that names the supported set
    cfg = ops.model.EccRnnCfg()
    cfg.nc, cfg.nrepeats, cfg.matrix, cfg.n_fnet, cfg.bnidx = 24, 1, 0, 1, -1
    cfg.fnet_widths[0], cfg.fnet_widths[1] = 13, 24
    assert L.spg_eccrnn_workspace_bytes(cfg, 5, E, 1) == 0 and b'8, 16, 32, 64 and 128' in L.spg_last_error()
    cfg.nc, cfg.matrix, cfg.fnet_widths[1] = 128, 1, 128 * 128
    assert L.spg_eccrnn_workspace_bytes(cfg, 5, E, 1) == 0 and b'matrix filters' in L.spg_last_error()
    assert L.spg_cell_scratch_floats(0, 24, 3) == 0 and b'8, 16, 32, 64 and 128' in L.spg_last_error()


def report():
    from superpoint_graph_amd import _lib
    _lib.lib()
    lines = ['# python tests/test_gpu_wide_eccrnn.py: worst error / bound (1e-4 |ref| + 1e-5 max|ref| per element, float64 reference) per module',
             '# case over out, grad x and every judged parameter gradient: the device, and the float32 CPU evaluation of the same reference',
             f"{'case':60s} {'device':>8s} {'cpu f32':>8s}  worst device tensor; ReLU decisions that differ"]
    for args in C.MODULE_CASES + (C.NETWORK_CASE,):
        case = C.module_case(*args) if len(args) == 8 else C.network_case(*args)
        got, dec = run_network(case)
        refs, n_diff = C.module_refs(case, dec)
        rec32 = {}
        cpu = C.module_eval(case, torch.float32, rec=rec32)
        refs32, _ = C.module_refs(case, EC.decisions(rec32))
        dev_f = {k: C.bound_ratio(got[k], r) for k, r in refs.items()}
        k = max(dev_f, key=lambda t: dev_f[t][1])
        lines.append(f"{case['name']:60s} {dev_f[k][1]:8.3f} {max(C.bound_ratio(cpu[t], r)[1] for t, r in refs32.items()):8.3f}  {k}; {n_diff}")
    return '\n'.join(lines)


if __name__ == '__main__':
    print(report())
