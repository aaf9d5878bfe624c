"""The training step's network: graph structure, generic ECC, GRU / LSTM cells, dense layers, PointNet, GroupNorm PointNet and the
RNN-ECC module with its persistent-launch status (csrc/spg_api.hip for the stand-alone operators, spg_pointnet.hip,
spg_groupnorm.hip, spg_eccnet.hip, spg_ecc.hip)."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from .. import _lib
from .._lib import EccRnnCfg, GnCfg, PointNetCfg, check, lib
from ._core import _ptr, _ptr_array, _req, _stream


# --------------------------------------------------------------------------------------------------
# graph structure
# --------------------------------------------------------------------------------------------------
class DeviceGraph:
    """CSR-by-target + reverse CSR built on the device from GraphConvInfo's (idxn, degs)."""

    def __init__(self, idxn: torch.Tensor, degs: torch.Tensor, n_src: Optional[int] = None):
        """n_src: number of rows of the input feature matrix (>= number of output nodes; equal for superpoint graphs)."""
        _req(idxn, torch.int64, 'idxn'); _req(degs, torch.int64, 'degs')
        self.N, self.E = int(degs.numel()), int(idxn.numel())
        self.n_src = max(self.N, int(n_src) if n_src is not None else self.N)
        nbytes = lib().spg_graph_workspace_bytes(self.N, self.n_src, self.E)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=idxn.device)
        self.idxn, self.degs = idxn, degs
        check(lib().spg_graph_build(_ptr(idxn) if self.E else None, _ptr(degs), self.N, self.n_src, self.E, _ptr(self.ws),
                                    _stream()), 'spg_graph_build')

    @classmethod
    def from_workspace(cls, ws: torch.Tensor, idxn: torch.Tensor, degs: torch.Tensor):
        """A graph whose workspace was already filled on the device (ops.batch_graph_build)."""
        g = cls.__new__(cls)
        g.N, g.E = int(degs.numel()), int(idxn.numel())
        g.n_src = g.N
        g.ws, g.idxn, g.degs = ws, idxn, degs
        return g

    def export(self):
        dev = self.ws.device
        rowptr = torch.empty(self.N + 1, dtype=torch.int32, device=dev)
        rev_rowptr = torch.empty(self.n_src + 1, dtype=torch.int32, device=dev)
        src = torch.empty(self.E, dtype=torch.int32, device=dev)
        dst = torch.empty(self.E, dtype=torch.int32, device=dev)
        rev = torch.empty(self.E, dtype=torch.int32, device=dev)
        self.hdr = torch.empty(4, dtype=torch.int32, device=dev)
        check(lib().spg_graph_export(_ptr(self.ws), self.N, self.n_src, self.E, _ptr(rowptr), _ptr(src), _ptr(dst),
                                     _ptr(rev_rowptr), _ptr(rev), _ptr(self.hdr), _stream()), 'spg_graph_export')
        return rowptr, src, dst, rev_rowptr, rev


# --------------------------------------------------------------------------------------------------
# generic ECC operator
# --------------------------------------------------------------------------------------------------
_DT = {torch.float32: 0, torch.float64: 1}


def ecc_aggregate_fwd(x, w, graph: DeviceGraph, idxe=None, cin=None, cout=None):
    _req(x, name='input'); _req(w, x.dtype, 'weights')
    if x.shape[0] > graph.n_src:
        raise ValueError(f'graph was built for {graph.n_src} input rows, input has {x.shape[0]}')
    matrix = w.dim() == 3
    cin = x.shape[1] if cin is None else cin
    cout = (w.shape[2] if matrix else w.shape[1]) if cout is None else cout
    out = torch.empty(graph.N, cout, dtype=x.dtype, device=x.device)
    check(lib().spg_ecc_aggregate_fwd(_DT[x.dtype], _ptr(x), _ptr(w), _ptr(idxe), _ptr(graph.ws), graph.N, graph.E, cin, cout,
                                      int(matrix), _ptr(out), _stream()), 'spg_ecc_aggregate_fwd')
    return out


def ecc_aggregate_bwd(x, w, grad_out, graph: DeviceGraph, idxe=None, need_x=True, need_w=True):
    matrix = w.dim() == 3
    cin = x.shape[1]
    cout = w.shape[2] if matrix else w.shape[1]
    grad_out = grad_out.contiguous()
    gx = torch.empty_like(x) if need_x else None
    gw = torch.empty_like(w) if need_w else None
    check(lib().spg_ecc_aggregate_bwd(_DT[x.dtype], _ptr(x), _ptr(w), _ptr(idxe), _ptr(graph.ws), graph.N, graph.E,
                                      x.shape[0], w.shape[0], cin, cout, int(matrix), _ptr(grad_out), _ptr(gx), _ptr(gw),
                                      _stream()), 'spg_ecc_aggregate_bwd')
    return gx, gw


# --------------------------------------------------------------------------------------------------
# GRU / LSTM cell at any supported width (spg_cell_fwd / spg_cell_bwd)
# --------------------------------------------------------------------------------------------------
CELL_KINDS = {'gru': 0, 'lstm': 1}
CELL_WIDTHS = (8, 16, 32, 64, 128)            # state widths the HIP cells and the RNN-ECC recurrence serve
MATRIX_FILTER_MAX_WIDTH = 64                  # [E, nc, nc] filters: 64 KB per edge at 128 are refused


def check_cell_width(nc, matrix=False, what='the HIP RNN-ECC kernels'):
    """NotImplementedError that names the supported set, before anything is launched (the library refuses the same with -2)."""
    if nc not in CELL_WIDTHS:
        raise NotImplementedError(f'{what}: state width {nc} is not supported; supported widths: {", ".join(map(str, CELL_WIDTHS))}')
    if matrix and nc > MATRIX_FILTER_MAX_WIDTH:
        raise NotImplementedError(f'{what}: matrix filters at state width {nc} ({nc * nc * 4 // 1024} KB of filter per edge) are not supported; '
                                  f'matrix filters are limited to widths up to {MATRIX_FILTER_MAX_WIDTH} (use vector filters at {nc})')


def _cell_check(rc, what):
    if rc == -2:
        raise NotImplementedError(lib().spg_last_error().decode())
    check(rc, what)


def _cell_scratch(kind, nc, n, device):
    floats = lib().spg_cell_scratch_floats(CELL_KINDS[kind], nc, n)
    if floats == 0:
        _cell_check(-2, 'spg_cell_scratch_floats')
    return torch.empty(floats, dtype=torch.float32, device=device)


def cell_block_nodes(nc: int) -> int:
    """Rows (nodes) per workgroup of the cell / step kernels at width nc."""
    return int(lib().spg_cell_block_nodes(nc))


def cell_fwd(kind, inp, h, c, params: Sequence[Optional[torch.Tensor]], layernorm: bool, ingate: bool):
    """GRUCellEx / LSTMCellEx forward at width nc = inp.shape[1]: -> (hy, cy); c and cy are None for the GRU."""
    _req(inp, torch.float32, 'input'); _req(h, torch.float32, 'hidden')
    n, nc = inp.shape
    check_cell_width(nc, what=f'the HIP {kind.upper()} cell')
    if tuple(h.shape) != (n, nc):
        raise ValueError(f'hidden must be [{n}, {nc}], got {tuple(h.shape)}')
    lstm = kind == 'lstm'
    if lstm:
        _req(c, torch.float32, 'hidden[1]')
    hy = torch.empty_like(h)
    cy = torch.empty_like(h) if lstm else None
    _cell_check(lib().spg_cell_fwd(CELL_KINDS[kind], nc, _ptr(inp), _ptr(h), _ptr(c) if lstm else None, n, _ptr_array(params),
                                   int(layernorm), int(ingate), _ptr(hy), _ptr(cy), None, _stream()), 'spg_cell_fwd')      # (no scratch)
    return hy, cy


def cell_bwd(kind, inp, h, c, grad_hy, grad_cy, params, layernorm: bool, ingate: bool):
    """-> (grad input, grad h, grad c or None, parameter gradients like `params`)."""
    n, nc = inp.shape
    check_cell_width(nc, what=f'the HIP {kind.upper()} cell')
    lstm = kind == 'lstm'
    grad_hy = None if grad_hy is None else _req(grad_hy.contiguous(), torch.float32, 'grad_hy')
    grad_cy = None if (grad_cy is None or not lstm) else _req(grad_cy.contiguous(), torch.float32, 'grad_cy')
    gi, gh = torch.empty_like(inp), torch.empty_like(h)
    gc = torch.empty_like(h) if lstm else None
    grads = [None if p is None else torch.empty_like(p) for p in params]
    scratch = _cell_scratch(kind, nc, n, inp.device)
    _cell_check(lib().spg_cell_bwd(CELL_KINDS[kind], nc, _ptr(inp), _ptr(h), _ptr(c) if lstm else None, _ptr(grad_hy), _ptr(grad_cy), n,
                                   _ptr_array(params), int(layernorm), int(ingate), _ptr(gi), _ptr(gh), _ptr(gc), _ptr_array(grads),
                                   _ptr(scratch), _stream()), 'spg_cell_bwd')
    return gi, gh, gc, grads


# the per-kind names of the API: the same calls with `kind` fixed and the other cell's slots dropped
def gru_cell_fwd(inp, hidden, params: Sequence[Optional[torch.Tensor]], layernorm: bool, ingate: bool):
    return cell_fwd('gru', inp, hidden, None, params, layernorm, ingate)[0]


def gru_cell_bwd(inp, hidden, grad_out, params, layernorm: bool, ingate: bool):
    gi, gh, _, grads = cell_bwd('gru', inp, hidden, None, grad_out, None, params, layernorm, ingate)
    return gi, gh, grads


def lstm_cell_fwd(inp, h, c, params: Sequence[Optional[torch.Tensor]], layernorm: bool, ingate: bool):
    return cell_fwd('lstm', inp, h, c, params, layernorm, ingate)


def lstm_cell_bwd(inp, h, c, grad_hy, grad_cy, params, layernorm: bool, ingate: bool):
    return cell_bwd('lstm', inp, h, c, grad_hy, grad_cy, params, layernorm, ingate)


# --------------------------------------------------------------------------------------------------
# dense layer
# --------------------------------------------------------------------------------------------------
def linear_fwd(x, w, bias=None, in_scale=None, in_shift=None, in_relu=False):
    _req(x, torch.float32, 'x'); _req(w, torch.float32, 'w')
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    check(lib().spg_linear_fwd(_ptr(x), K, M, K, _ptr(w), _ptr(bias), N, _ptr(in_scale), _ptr(in_shift), int(in_relu), _ptr(y),
                               N, _stream()), 'spg_linear_fwd')
    return y


def linear_dgrad(dy, w):
    """dx [M, K] = dy [M, N] @ w [N, K]."""
    _req(dy, torch.float32, 'dy'); _req(w, torch.float32, 'w')
    M, N = dy.shape
    K = w.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
    check(lib().spg_linear_dgrad(_ptr(dy), N, M, N, _ptr(w), K, _ptr(dx), K, _stream()), 'spg_linear_dgrad')
    return dx


def colsum(x, out=None):
    _req(x, torch.float32, 'x')
    M, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=x.device) if out is None else out
    work = torch.empty(64 * N, dtype=torch.float32, device=x.device)
    check(lib().spg_colsum(_ptr(x), N, M, N, _ptr(out), _ptr(work), _stream()), 'spg_colsum')
    return out


def linear_wgrad(dy, x, in_scale=None, in_shift=None, in_relu=False, out=None):
    M, N = dy.shape
    K = x.shape[1]
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device) if out is None else out
    work = torch.empty(max(1, lib().spg_linear_wgrad_work_floats(M, N, K)), dtype=torch.float32, device=x.device)
    check(lib().spg_linear_wgrad(_ptr(dy), N, _ptr(x), K, M, N, K, _ptr(in_scale), _ptr(in_shift), int(in_relu), _ptr(dw),
                                 _ptr(work), _stream()), 'spg_linear_wgrad')
    return dw


def linear_wgrad_bias(dy, x, out_w=None, out_b=None):
    """dW [N, K] and dbias [N] of a dense layer in two launches (spg_linear_wgrad_bias)."""
    _req(dy, torch.float32, 'dy'); _req(x, torch.float32, 'x')
    M, N = dy.shape
    K = x.shape[1]
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device) if out_w is None else out_w
    db = torch.empty(N, dtype=torch.float32, device=x.device) if out_b is None else out_b
    work = torch.empty(max(1, lib().spg_linear_wgrad_bias_work_floats(M, N, K)), dtype=torch.float32, device=x.device)
    check(lib().spg_linear_wgrad_bias(_ptr(dy), N, _ptr(x), K, M, N, K, None, None, 0, _ptr(dw), _ptr(db), _ptr(work), _stream()),
          'spg_linear_wgrad_bias')
    return dw, db


def linear_backward(dy, x, w, need_dx=True, has_bias=True, out_w=None, out_b=None):
    """The whole backward of y = x w^T + b: (dx or None, dW, dbias or None) -- ONE grouped launch + one batched reduction
    (spg_linear_backward) instead of three launches."""
    _req(dy, torch.float32, 'dy'); _req(x, torch.float32, 'x'); _req(w, torch.float32, 'w')
    M, N = dy.shape
    K = x.shape[1]
    dx = torch.empty(M, K, dtype=torch.float32, device=x.device) if need_dx else None
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device) if out_w is None else out_w
    db = (torch.empty(N, dtype=torch.float32, device=x.device) if out_b is None else out_b) if has_bias else None
    work = torch.empty(max(1, lib().spg_linear_wgrad_bias_work_floats(M, N, K)), dtype=torch.float32, device=x.device)
    check(lib().spg_linear_backward(_ptr(dy), N, _ptr(x), K, _ptr(w), M, N, K, _ptr(dx), K, _ptr(dw), _ptr(db), _ptr(work), _stream()),
          'spg_linear_backward')
    return dx, dw, db


# --------------------------------------------------------------------------------------------------
# PointNet
# --------------------------------------------------------------------------------------------------
POINTNET_MAX_TILE = 128          # points of one row tile of the convolutions
POINTNET_MIN_SEGMENT = 32        # shortest segment a superpoint of more than 128 points may be cut into
POINTNET_NPTS_END = 4096         # from this size on nothing is served (the library's size queries have always refused 4096)
POINTNET_NPTS_RULE = (f'npts must be in [1, {POINTNET_MAX_TILE}], or in ({POINTNET_MAX_TILE}, {POINTNET_NPTS_END}) with a divisor in '
                      f'[{POINTNET_MIN_SEGMENT}, {POINTNET_MAX_TILE}] (the largest one is the segment length: 256 = 2 x 128, '
                      '160 = 2 x 80, 1000 = 8 x 125; 131 and 262 have none)')


def pointnet_segments(npts):
    """(Ps, S): the BatchNorm PointNet runs its convolutions on S = npts / Ps segments of Ps points per superpoint -- one segment up
    to 128 points, else (below 4096) Ps is the largest divisor of npts that is <= 128 and must be >= 32 (the library
    refuses the same with -2).  NotImplementedError that states the rule: pointnet_forward and the modules call this before anything is
    allocated or launched (make_pointnet_cfg fills any npts in, as it always did)."""
    npts = int(npts)
    if 1 <= npts <= POINTNET_MAX_TILE:
        return npts, 1
    if POINTNET_MAX_TILE < npts < POINTNET_NPTS_END:
        for ps in range(POINTNET_MAX_TILE, POINTNET_MIN_SEGMENT - 1, -1):
            if npts % ps == 0:
                return ps, npts // ps
    raise NotImplementedError(f'PointNet: npts = {npts} is not supported: {POINTNET_NPTS_RULE}')


def make_pointnet_cfg(nfeat, nfeat_stn, nfeat_global, npts, stn_conv, stn_fc, conv, fc, last_ac=False,
                      bn_eps=1e-5, bn_momentum=0.1) -> PointNetCfg:
    c = PointNetCfg()
    c.nfeat, c.nfeat_stn, c.nfeat_global, c.npts = nfeat, nfeat_stn, nfeat_global, npts
    c.n_stn_conv, c.n_stn_fc, c.n_conv, c.n_fc = len(stn_conv), len(stn_fc), len(conv), len(fc)
    for dst, src in ((c.stn_conv, stn_conv), (c.stn_fc, stn_fc), (c.conv, conv), (c.fc, fc)):
        if len(src) > _lib.SPG_MAX_LAYERS:
            raise ValueError('too many layers')
        for i, v in enumerate(src):
            dst[i] = int(v)
    c.last_ac, c.bn_eps, c.bn_momentum = int(last_ac), bn_eps, bn_momentum
    return c


def _require_training_state(state, what):
    """The backward kernels read the batch-statistics workspace layout of a TRAINING-mode forward (saved aggregates,
    BatchNorm mean / rstd).  After an eval-mode forward that layout does not exist: fail loudly instead of reading
    out of bounds (frozen-BatchNorm fine-tuning is not implemented on the HIP path)."""
    if not state.training:
        raise RuntimeError(f'{what}: backward() after an eval-mode forward is not supported by the HIP path '
                           '(the backward implements batch-statistics BatchNorm); call model.train() before the forward, '
                           'or wrap the eval-mode forward in torch.no_grad()')


def rows6(rows):
    """Every row padded with None to the six pointers per layer of the library's tables."""
    return [tuple(r) + (None,) * (6 - len(r)) for r in rows]


def _grad_rows(groups, live, out_grads=None):
    """Six gradient destinations per row of `groups`: the first `live[li]` are `out_grads[li]`'s (written, not accumulated; a
    None entry is skipped by the library) or fresh tensors shaped like the parameters; the running statistics have none."""
    if out_grads is not None:
        if len(out_grads) != len(groups):
            raise ValueError(f'out_grads: {len(groups)} rows expected, got {len(out_grads)}')
        return rows6(tuple(d[:n]) for d, n in zip(out_grads, live))
    return rows6(tuple(None if t is None else torch.empty_like(t) for t in g[:n]) for g, n in zip(groups, live))


class PointNetState:
    """Saved forward state (workspace with the raw layer outputs and BatchNorm constants)."""

    def __init__(self, cfg, B, clouds, clouds_global, ws, training, ext_transform=None):
        self.cfg, self.B, self.clouds, self.clouds_global, self.ws = cfg, B, clouds, clouds_global, ws
        self.training = bool(training)
        self.ext_transform = ext_transform


def pointnet_forward(cfg: PointNetCfg, clouds, clouds_global, groups: List[Sequence[Optional[torch.Tensor]]],
                     training: bool, bn_update_times: int = 1, ext_transform=None):
    """groups: one 6-tuple (weight, bias, bn.weight, bn.bias, running_mean, running_var) per layer in the order
    of include/spg_hip.h.  ext_transform: [B, 4] = T - I of an externally evaluated STN (PointNet without inner STN).
    Returns (emb [B, D], PointNetState)."""
    _req(clouds, torch.float32, 'clouds')
    pointnet_segments(cfg.npts)      # an unsupported npts: NotImplementedError with the rule, before any allocation or launch
    B = clouds.shape[0]
    if clouds.shape[1] != cfg.nfeat or clouds.shape[2] != cfg.npts:
        raise ValueError(f'clouds must be [B, {cfg.nfeat}, {cfg.npts}], got {tuple(clouds.shape)}')
    if training and B <= 1:
        # torch.nn.BatchNorm1d raises for the FC layers ([1, C] / empty input) in training mode; so do we
        raise ValueError(f'Expected more than 1 value per channel when training, got input size [{B}, C]')
    if B == 0:      # inference on a batch without a single embeddable superpoint: nothing to launch
        return (torch.zeros(0, cfg.fc[cfg.n_fc - 1], dtype=torch.float32, device=clouds.device),
                PointNetState(cfg, 0, clouds, clouds_global, None, training, ext_transform))
    if clouds_global is not None:
        clouds_global = _req(clouds_global.reshape(B, -1).contiguous(), torch.float32, 'clouds_global')
        if clouds_global.shape[1] != cfg.nfeat_global:
            raise ValueError('clouds_global width does not match nfeat_global')
    nbytes = lib().spg_pointnet_workspace_bytes(ctypes.byref(cfg), B, int(training))
    if nbytes == 0:
        raise RuntimeError('spg_pointnet_workspace_bytes: ' + lib().spg_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=clouds.device)
    D = cfg.fc[cfg.n_fc - 1]
    emb = torch.empty(B, D, dtype=torch.float32, device=clouds.device)
    flat = [t for g in groups for t in g]
    if ext_transform is not None:
        ext_transform = _req(ext_transform.reshape(B, 4).contiguous(), torch.float32, 'ext_transform')
    check(lib().spg_pointnet_forward_ext(ctypes.byref(cfg), B, _ptr(clouds), _ptr(clouds_global), _ptr(ext_transform), _ptr_array(flat),
                                         _ptr(emb), _ptr(ws), int(training), int(bn_update_times), _stream()), 'spg_pointnet_forward')
    return emb, PointNetState(cfg, B, clouds, clouds_global, ws, training, ext_transform)


def pointnet_backward(state: PointNetState, groups, grad_emb, out_grads=None, want_input_grads=False):
    """Returns a list of 4-tuples (d weight, d bias, d bn.weight, d bn.bias) per layer.
    out_grads: optional pre-allocated destination tensors in the same structure (written, not accumulated); a
    `None` entry is skipped by the library (used for the analytically-zero biases in front of a BatchNorm when the
    destination is a pre-zeroed flat gradient buffer)."""
    cfg, B = state.cfg, state.B
    _require_training_state(state, 'PointNet')
    if getattr(state, 'backward_done', False):
        # the BatchNorm-backward sums are accumulated into slots of the forward workspace that the forward cleared (spg_gemm.h):
        # a second backward pass over the same forward would add to them again
        raise RuntimeError('PointNet: a second backward() through the same forward is not supported by the HIP path '
                           '(run the forward again)')
    state.backward_done = True
    grad_emb = _req(grad_emb.contiguous(), torch.float32, 'grad_emb')
    nbytes = lib().spg_pointnet_bwd_workspace_bytes(ctypes.byref(cfg), B)
    bws = torch.empty(nbytes, dtype=torch.uint8, device=grad_emb.device)
    grows = _grad_rows(groups, [4] * len(groups), out_grads)
    gg, flatg = [r[:4] for r in grows], [t for r in grows for t in r]
    flat = [t for g in groups for t in g]
    g_T = g_glob = None
    if want_input_grads:          # gradients wrt the external transform and the global features (LocalCloudEmbedder)
        if state.ext_transform is not None:
            g_T = torch.empty(B, 4, dtype=torch.float32, device=grad_emb.device)
        if state.clouds_global is not None:
            g_glob = torch.empty_like(state.clouds_global)
    check(lib().spg_pointnet_backward_ext(ctypes.byref(cfg), B, _ptr(state.clouds), _ptr(state.clouds_global), _ptr(state.ext_transform),
                                          _ptr_array(flat), _ptr(grad_emb), _ptr_array(flatg), _ptr(g_T), _ptr(g_glob), _ptr(state.ws),
                                          _ptr(bws), _stream()), 'spg_pointnet_backward')
    if want_input_grads:
        return gg, g_T, g_glob
    return gg


# --------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm PointNet (the learned partition's local embedder with --ptn_norm layer|group)
# --------------------------------------------------------------------------------------------------
def _gn_check(rc: int, what: str):
    """-2 is the library's "outside the supported range": a NotImplementedError that names the limit."""
    if rc == -2:
        raise NotImplementedError(lib().spg_last_error().decode())
    check(rc, what)


def make_gn_cfg(nfeat, nfeat_global, npts, conv, fc, n_group, eps=1e-5, last_ac=False) -> GnCfg:
    """spg_gn_cfg of a PointNet without inner STN (a stand-alone STN: nfeat_global = 0, fc = [..., K * K]); raises
    NotImplementedError for what the kernels do not cover, before anything is launched."""
    if len(conv) > _lib.SPG_MAX_LAYERS or len(fc) > _lib.SPG_MAX_LAYERS:
        raise NotImplementedError(f'GroupNorm PointNet: at most SPG_MAX_LAYERS = {_lib.SPG_MAX_LAYERS} layers per stack')
    c = GnCfg()
    c.net = make_pointnet_cfg(nfeat, 0, nfeat_global, npts, [], [], conv, fc, last_ac, eps, 0.0)
    c.n_group, c.eps = int(n_group), float(eps)
    _gn_check(lib().spg_gn_check(ctypes.byref(c)), 'spg_gn_check')
    return c


class GroupNormState:
    """What a forward leaves for its backward: per cloud only (statistics, pooled values, arg-max points)."""

    def __init__(self, cfg, B, clouds, clouds_global, ws, ext_transform):
        self.cfg, self.B, self.clouds, self.clouds_global, self.ws, self.ext_transform = cfg, B, clouds, clouds_global, ws, ext_transform


def gn_forward(cfg: GnCfg, clouds, clouds_global, groups, ext_transform=None):
    """groups: one 6-tuple (weight, bias, norm.weight, norm.bias, None, None) per layer, convolutions then FCs.
    ext_transform: [B, 4] = T - I or None.  Returns (out [B, D], GroupNormState); train and eval are the same function."""
    _req(clouds, torch.float32, 'clouds')
    net, B = cfg.net, clouds.shape[0]
    if clouds.shape[1] != net.nfeat or clouds.shape[2] != net.npts:
        raise ValueError(f'clouds must be [B, {net.nfeat}, {net.npts}], got {tuple(clouds.shape)}')
    D = net.fc[net.n_fc - 1]
    if clouds_global is not None:
        clouds_global = _req(clouds_global.reshape(B, -1).contiguous(), torch.float32, 'clouds_global')
        if clouds_global.shape[1] != net.nfeat_global:
            raise ValueError('clouds_global width does not match nfeat_global')
    elif net.nfeat_global != 0:
        raise ValueError('clouds_global is required')
    if ext_transform is not None:
        ext_transform = _req(ext_transform.reshape(B, 4).contiguous(), torch.float32, 'ext_transform')
    if B == 0:
        return torch.zeros(0, D, dtype=torch.float32, device=clouds.device), GroupNormState(cfg, 0, clouds, clouds_global, None, ext_transform)
    nbytes = lib().spg_gn_workspace_bytes(ctypes.byref(cfg), B)
    if nbytes == 0:
        _gn_check(lib().spg_gn_check(ctypes.byref(cfg)), 'spg_gn_workspace_bytes')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=clouds.device)
    emb = torch.empty(B, D, dtype=torch.float32, device=clouds.device)
    flat = [t for g in groups for t in g]
    _gn_check(lib().spg_gn_forward_ext(ctypes.byref(cfg), B, _ptr(clouds), _ptr(clouds_global), _ptr(ext_transform), _ptr_array(flat),
                                       _ptr(emb), _ptr(ws), _stream()), 'spg_gn_forward_ext')
    return emb, GroupNormState(cfg, B, clouds, clouds_global, ws, ext_transform)


def gn_backward(state: GroupNormState, groups, grad_emb, want_clouds=False):
    """-> (list of (d weight, d bias, d norm.weight, d norm.bias) per layer, grad wrt the transform [B, 4] or None, grad wrt the
    global features or None, grad wrt the clouds or None).  Bit-reproducible: partials in a fixed layout, summed in a fixed order."""
    cfg, B = state.cfg, state.B
    grad_emb = _req(grad_emb.contiguous(), torch.float32, 'grad_emb')
    dev = grad_emb.device
    grows = _grad_rows(groups, [4] * len(groups))
    gg = [r[:4] for r in grows]
    g_T = torch.empty(B, 4, dtype=torch.float32, device=dev) if state.ext_transform is not None else None
    g_glob = torch.empty_like(state.clouds_global) if state.clouds_global is not None else None
    g_clouds = torch.empty_like(state.clouds) if want_clouds else None
    if B == 0:
        return [tuple(None if t is None else t.zero_() for t in row) for row in gg], g_T, g_glob, g_clouds
    nbytes = lib().spg_gn_bwd_workspace_bytes(ctypes.byref(cfg), B)
    bws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flat = [t for g in groups for t in g]
    flatg = [t for r in grows for t in r]
    _gn_check(lib().spg_gn_backward_ext(ctypes.byref(cfg), B, _ptr(state.clouds), _ptr(state.clouds_global), _ptr(state.ext_transform),
                                        _ptr_array(flat), _ptr(grad_emb), _ptr_array(flatg), _ptr(g_T), _ptr(g_glob), _ptr(g_clouds),
                                        _ptr(state.ws), _ptr(bws), _stream()), 'spg_gn_backward_ext')
    return gg, g_T, g_glob, g_clouds


# --------------------------------------------------------------------------------------------------
# RNN-ECC module
# --------------------------------------------------------------------------------------------------
def make_eccrnn_cfg(nc, nrepeats, matrix, layernorm, ingate, cat_all, fnet_widths, bnidx, llbias, bn_eps=1e-5,
                    bn_momentum=0.1, cell='gru') -> EccRnnCfg:
    check_cell_width(nc, bool(matrix), 'the fused RNN-ECC path')
    c = EccRnnCfg()
    c.nc, c.nrepeats, c.matrix, c.layernorm, c.ingate, c.cat_all = nc, nrepeats, int(matrix), int(layernorm), int(ingate), int(cat_all)
    c.n_fnet = len(fnet_widths) - 1
    if c.n_fnet > _lib.SPG_MAX_LAYERS:
        raise ValueError('filter network too deep')
    for i, v in enumerate(fnet_widths):
        c.fnet_widths[i] = int(v)
    c.bnidx, c.llbias, c.bn_eps, c.bn_momentum = bnidx, int(llbias), bn_eps, bn_momentum
    c.cell = {'gru': 0, 'lstm': 1}[cell]
    return c


class EccRnnState:
    def __init__(self, cfg, graph, edgefeats, ws, training):
        self.cfg, self.graph, self.edgefeats, self.ws = cfg, graph, edgefeats, ws
        self.training = bool(training)


def eccrnn_forward(cfg: EccRnnCfg, graph: DeviceGraph, h0, edgefeats, groups, training: bool, bn_update_times: int = 1):
    _req(h0, torch.float32, 'input'); _req(edgefeats, torch.float32, 'edgefeats')
    N, E = graph.N, graph.E
    if h0.shape[0] != N or h0.shape[1] != cfg.nc:
        raise ValueError(f'input must be [{N}, {cfg.nc}], got {tuple(h0.shape)}')
    if edgefeats.dim() != 2 or edgefeats.shape[0] != E or edgefeats.shape[1] != cfg.fnet_widths[0]:
        raise ValueError(f'edgefeats must be [{E}, {cfg.fnet_widths[0]}], got {tuple(edgefeats.shape)}')
    if training and cfg.bnidx >= 0 and E == 1:
        raise ValueError('Expected more than 1 value per channel when training (filter-network BatchNorm over one edge)')
    nbytes = lib().spg_eccrnn_workspace_bytes(ctypes.byref(cfg), N, E, int(training))
    if nbytes == 0:
        raise RuntimeError('spg_eccrnn_workspace_bytes: ' + lib().spg_last_error().decode())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=h0.device)
    width = cfg.nc * (cfg.nrepeats + 1) if cfg.cat_all else cfg.nc
    out = torch.empty(N, width, dtype=torch.float32, device=h0.device)
    flat = [t for g in groups for t in g]
    check(lib().spg_eccrnn_forward(ctypes.byref(cfg), N, E, _ptr(graph.ws), _ptr(h0), _ptr(edgefeats), _ptr_array(flat),
                                   _ptr(out), _ptr(ws), int(training), int(bn_update_times), _stream()), 'spg_eccrnn_forward')
    return out, EccRnnState(cfg, graph, edgefeats, ws, training)


def eccrnn_backward(state: EccRnnState, groups, grad_out, out_grads=None):
    """out_grads: see pointnet_backward."""
    cfg, graph = state.cfg, state.graph
    N, E = graph.N, graph.E
    _require_training_state(state, 'RNN-ECC')
    grad_out = _req(grad_out.contiguous(), torch.float32, 'grad_out')
    bws = torch.empty(lib().spg_eccrnn_bwd_workspace_bytes(ctypes.byref(cfg), N, E), dtype=torch.uint8, device=grad_out.device)
    grad_h0 = torch.empty(N, cfg.nc, dtype=torch.float32, device=grad_out.device)
    gg = _grad_rows(groups, [4] * cfg.n_fnet + [6] * (len(groups) - cfg.n_fnet), out_grads)      # layers of the filter network, then the cell
    flatg = [t for r in gg for t in r]
    flat = [t for g in groups for t in g]
    check(lib().spg_eccrnn_backward(ctypes.byref(cfg), N, E, _ptr(graph.ws), _ptr(state.edgefeats), _ptr_array(flat),
                                    _ptr(grad_out), _ptr(grad_h0), _ptr_array(flatg), _ptr(state.ws), _ptr(bws), _stream()),
          'spg_eccrnn_backward')
    return grad_h0, gg


# --------------------------------------------------------------------------------------------------
# health of the dataflow-synchronised RNN-ECC launches
# --------------------------------------------------------------------------------------------------
def persistent_ecc_status(clear=False):
    """(time-outs, withheld optimiser updates) of the dataflow-synchronised RNN-ECC launches of the current device
    (include/spg_hip.h: spg_ecc_persistent_status).  The time-out word is sticky and read by the fused clamp + Adam launch itself: while
    it is non-zero every update is WITHHELD (parameters / moments bit-identical), so nothing computed from stale neighbour states
    reaches the model before the host has looked.  One blocking 16-byte copy: synchronises the device."""
    e, w = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().spg_ecc_persistent_status(ctypes.byref(e), ctypes.byref(w), 1 if clear else 0), 'spg_ecc_persistent_status')
    return int(e.value), int(w.value)


def recover_persistent_ecc(arena=None, group=None):
    """The per-step fail-safe's host half: reads and clears the status; when a recurrence has timed out, switches this process (every
    rank of `group`: the decision is all-reduced) to the per-iteration kernels (spg_tune key 8, which cannot time out) and takes the
    withheld updates off `arena`'s Adam step counter (FlatParameters.rewind_steps).  Returns the number of withheld updates (0:
    nothing happened) -- the caller repeats the batches it still holds.  COLLECTIVE when a process group is initialised (every rank
    must call it at the same step; group=False keeps it local)."""
    errors, withheld = persistent_ecc_status(clear=True)
    total = errors
    if group is not False:
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            on_gpu = dist.get_backend(group) == 'nccl'
            t = torch.tensor([float(errors)], dtype=torch.float64, device=torch.device('cuda', torch.cuda.current_device()) if on_gpu else 'cpu')
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            total = int(t.item())
    if total == 0:
        return 0
    lib().spg_tune(8, 1)
    if arena is not None and withheld:
        arena.rewind_steps(withheld)
    return max(withheld, 1)


def check_persistent_ecc(what='training', group=None):
    """Health check of the dataflow-synchronised RNN-ECC launches (include/spg_hip.h: spg_ecc_persistent_status): a
    wave whose bounded spin ran out (a peer workgroup was not resident in time: shared GPU, profiler, another stream holding
    CUs) carried on with stale neighbour states.  Since round 6 the fused optimiser launch WITHHOLDS its update while the time-out word
    is set, so the parameters are never touched by such a step; this check is the last line (epoch end, before a checkpoint).
    Synchronises the device.  Raises after clearing the counters and switching this process to the per-iteration kernels
    (spg_tune key 8), so a caller that catches the error can repeat the affected work safely.
    COLLECTIVE CONTRACT: with an initialised process group the count is summed over the ranks of `group` first -- EVERY rank of the
    group must call it at the same point (a read failure on one rank is folded into the reduced value and raised on every rank, so no
    rank is left alone in the collective); group=False keeps it local."""
    failed = None
    try:
        n, withheld = persistent_ecc_status(clear=True)
    except RuntimeError as exc:      # the counter could not be read: a different failure, not "-1 time-outs" -- but the collective still runs
        failed, n, withheld = exc, 0, 0
    total, any_failed = n, failed is not None
    if group is not False:
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            # data parallel: every rank must take the same decision (one rank raising alone leaves the others in the next
            # collective until the RCCL time-out, and the ranks would run different kernels afterwards)
            on_gpu = dist.get_backend(group) == 'nccl'
            t = torch.tensor([float(n), 1.0 if failed is not None else 0.0], dtype=torch.float64,
                             device=torch.device('cuda', torch.cuda.current_device()) if on_gpu else 'cpu')
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            total, any_failed = int(t[0].item()), bool(t[1].item() > 0)
    if any_failed:
        raise RuntimeError(f'the persistent RNN-ECC status could not be read during {what} on '
                           + ('this rank: ' + str(failed) if failed is not None else 'another rank of the job'))
    if total == 0:
        return
    lib().spg_tune(8, 1)
    raise RuntimeError(f'{total} persistent RNN-ECC spin time-out(s) ({n} on this rank; {withheld} optimiser update(s) withheld here) during '
                       f'{what}: the ECC outputs / gradients of the affected steps are wrong (a workgroup of the dataflow-synchronised launch '
                       'was not resident in time); the fused optimiser step withheld its updates from the first time-out on.  The process '
                       '(every rank of the job) now uses the per-iteration kernels (spg_tune key 8); repeat the work since the last check')
