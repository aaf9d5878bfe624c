"""Tensor-level wrappers over the C ABI (include/spg_hip.h): torch owns device memory and streams, the HIP
library does the arithmetic.  Every function here requires CUDA(ROCm) tensors and raises otherwise --
there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import EccRnnCfg, GnCfg, PointNetCfg, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _on_gpu(t, name):
    """The device test of _req on its own, for an argument that is converted before _req sees it."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f'{name} must live on the GPU: the superpoint_graph_amd kernels have no CPU path')
    return t


def _req(t: torch.Tensor, dtype=None, name='tensor'):
    _on_gpu(t, name)
    if t.device.index != torch.cuda.current_device():
        # the kernels are launched on the CURRENT device's stream; a tensor of another GPU would be an invalid access
        raise RuntimeError(f'{name} lives on cuda:{t.device.index} but the current device is cuda:{torch.cuda.current_device()}; '
                           'call torch.cuda.set_device() (or use `with torch.cuda.device_of(tensor):`) first')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return t


def _ptr_array(tensors: Sequence[Optional[torch.Tensor]]):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


# --------------------------------------------------------------------------------------------------
# host -> device staging
# --------------------------------------------------------------------------------------------------
def upload(host: torch.Tensor, device=None) -> torch.Tensor:
    """Asynchronous host-to-device copy of a small per-batch tensor (edge lists, index vectors, edge features) through the
    library's page-locked staging ring (spg_upload): a copy from PAGEABLE memory blocks the host until the stream reaches it
    -- i.e. until the previous step has drained, so host and GPU would take turns -- and pinning per batch costs tens of
    milliseconds.  The call returns once the copy is enqueued on the current stream; `host` may be re-used at once."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if host.is_cuda:
        return host.to(device)
    if host.is_pinned():                      # page-locked already (DataLoader pin_memory, pre-pinned buffers): a true asynchronous copy
        return host.to(device, non_blocking=True)
    if device.index is not None and device.index != torch.cuda.current_device():
        raise RuntimeError(f'upload: target cuda:{device.index} is not the current device cuda:{torch.cuda.current_device()}')
    host = host.contiguous()
    out = torch.empty(host.shape, dtype=host.dtype, device=device)
    check(lib().spg_upload(host.data_ptr(), host.numel() * host.element_size(), out.data_ptr(), _stream()), 'spg_upload')
    return out


def upload_packed(hosts, device=None):
    """Several small host tensors -> ONE staging copy -> views of one device buffer (include/spg_hip.h: spg_upload_packed), in the
    order given; None entries stay None.  What a fresh batch needs on the device besides its clouds travels this way (edge list,
    edge features, CloudEmbedder's index vectors, labels, diameters): one memcpy-and-enqueue instead of one per vector."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.index is not None and device.index != torch.cuda.current_device():
        raise RuntimeError(f'upload_packed: target cuda:{device.index} is not the current device cuda:{torch.cuda.current_device()}')
    live = [(i, t.contiguous()) for i, t in enumerate(hosts) if t is not None]
    for _, t in live:
        if t.is_cuda:
            raise TypeError('upload_packed takes host tensors')
    n = len(live)
    out = [None] * len(hosts)
    if n == 0:
        return out
    ptrs, sizes, offs = (ctypes.c_void_p * n)(), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    total = 0
    for k, (_, t) in enumerate(live):
        nb = t.numel() * t.element_size()
        ptrs[k], sizes[k], offs[k] = t.data_ptr() if nb else None, nb, total
        total += (nb + 255) & ~255
    buf = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    check(lib().spg_upload_packed(ptrs, sizes, offs, n, buf.data_ptr(), total, _stream()), 'spg_upload_packed')
    for k, (i, t) in enumerate(live):
        out[i] = buf[offs[k]:offs[k] + sizes[k]].view(t.dtype).view(t.shape)
    return out


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
# GRU cell
# --------------------------------------------------------------------------------------------------
def gru_cell_fwd(inp, hidden, params: Sequence[Optional[torch.Tensor]], layernorm: bool, ingate: bool):
    _req(inp, torch.float32, 'input'); _req(hidden, torch.float32, 'hidden')
    n = inp.shape[0]
    out = torch.empty_like(hidden)
    scratch = torch.empty(lib().spg_gru_scratch_floats(n), dtype=torch.float32, device=inp.device)
    check(lib().spg_gru_cell_fwd(_ptr(inp), _ptr(hidden), n, _ptr_array(params), int(layernorm), int(ingate), _ptr(out),
                                 _ptr(scratch), _stream()), 'spg_gru_cell_fwd')
    return out


def gru_cell_bwd(inp, hidden, grad_out, params, layernorm: bool, ingate: bool):
    n = inp.shape[0]
    grad_out = grad_out.contiguous()
    gi, gh = torch.empty_like(inp), torch.empty_like(hidden)
    grads = [None if p is None else torch.empty_like(p) for p in params]
    scratch = torch.empty(lib().spg_gru_scratch_floats(n), dtype=torch.float32, device=inp.device)
    check(lib().spg_gru_cell_bwd(_ptr(inp), _ptr(hidden), _ptr(grad_out), n, _ptr_array(params), int(layernorm), int(ingate),
                                 _ptr(gi), _ptr(gh), _ptr_array(grads), _ptr(scratch), _stream()), 'spg_gru_cell_bwd')
    return gi, gh, grads


def lstm_cell_fwd(inp, h, c, params: Sequence[Optional[torch.Tensor]], layernorm: bool, ingate: bool):
    _req(inp, torch.float32, 'input'); _req(h, torch.float32, 'hidden[0]'); _req(c, torch.float32, 'hidden[1]')
    n = inp.shape[0]
    hy, cy = torch.empty_like(h), torch.empty_like(c)
    check(lib().spg_lstm_cell_fwd(_ptr(inp), _ptr(h), _ptr(c), n, _ptr_array(params), int(layernorm), int(ingate), _ptr(hy),
                                  _ptr(cy), None, _stream()), 'spg_lstm_cell_fwd')
    return hy, cy


def lstm_cell_bwd(inp, h, c, grad_hy, grad_cy, params, layernorm: bool, ingate: bool):
    n = inp.shape[0]
    grad_hy = None if grad_hy is None else grad_hy.contiguous()
    grad_cy = None if grad_cy is None else grad_cy.contiguous()
    gi, gh, gc = torch.empty_like(inp), torch.empty_like(h), torch.empty_like(c)
    grads = [None if p is None else torch.empty_like(p) for p in params]
    scratch = torch.empty(lib().spg_lstm_scratch_floats(n), dtype=torch.float32, device=inp.device)
    check(lib().spg_lstm_cell_bwd(_ptr(inp), _ptr(h), _ptr(c), _ptr(grad_hy), _ptr(grad_cy), n, _ptr_array(params),
                                  int(layernorm), int(ingate), _ptr(gi), _ptr(gh), _ptr(gc), _ptr_array(grads), _ptr(scratch),
                                  _stream()), 'spg_lstm_cell_bwd')
    return gi, gh, gc, grads


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
    gg, flatg = [], []
    for li, g in enumerate(groups):
        if out_grads is not None:
            d = list(out_grads[li][:4])
        else:
            d = [None if g[k] is None else torch.empty_like(g[k]) for k in range(4)]
        gg.append(tuple(d))
        flatg += d + [None, None]
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
    gg = [tuple(None if g[k] is None else torch.empty_like(g[k]) for k in range(4)) for g in groups]
    g_T = torch.empty(B, 4, dtype=torch.float32, device=dev) if state.ext_transform is not None else None
    g_glob = torch.empty_like(state.clouds_global) if state.clouds_global is not None else None
    g_clouds = torch.empty_like(state.clouds) if want_clouds else None
    if B == 0:
        return [tuple(None if t is None else t.zero_() for t in row) for row in gg], g_T, g_glob, g_clouds
    nbytes = lib().spg_gn_bwd_workspace_bytes(ctypes.byref(cfg), B)
    bws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    flat = [t for g in groups for t in g]
    flatg = [t for row in gg for t in list(row) + [None, None]]
    _gn_check(lib().spg_gn_backward_ext(ctypes.byref(cfg), B, _ptr(state.clouds), _ptr(state.clouds_global), _ptr(state.ext_transform),
                                        _ptr_array(flat), _ptr(grad_emb), _ptr_array(flatg), _ptr(g_T), _ptr(g_glob), _ptr(g_clouds),
                                        _ptr(state.ws), _ptr(bws), _stream()), 'spg_gn_backward_ext')
    return gg, g_T, g_glob, g_clouds


# --------------------------------------------------------------------------------------------------
# RNN-ECC module
# --------------------------------------------------------------------------------------------------
def make_eccrnn_cfg(nc, nrepeats, matrix, layernorm, ingate, cat_all, fnet_widths, bnidx, llbias, bn_eps=1e-5,
                    bn_momentum=0.1, cell='gru') -> EccRnnCfg:
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
    gg, flatg = [], []
    nf = cfg.n_fnet
    for li, g in enumerate(groups):
        if out_grads is not None:
            d = (list(out_grads[li][:4]) + [None, None]) if li < nf else list(out_grads[li][:6])
        elif li < nf:
            d = [None if g[k] is None else torch.empty_like(g[k]) for k in range(4)] + [None, None]
        else:
            d = [None if g[k] is None else torch.empty_like(g[k]) for k in range(6)]
        gg.append(tuple(d))
        flatg += d
    flat = [t for g in groups for t in g]
    check(lib().spg_eccrnn_backward(ctypes.byref(cfg), N, E, _ptr(graph.ws), _ptr(state.edgefeats), _ptr_array(flat),
                                    _ptr(grad_out), _ptr(grad_h0), _ptr_array(flatg), _ptr(state.ws), _ptr(bws), _stream()),
          'spg_eccrnn_backward')
    return grad_h0, gg


# --------------------------------------------------------------------------------------------------
# batch construction on the device
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
        import torch.distributed as dist
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
        import torch.distributed as dist
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


def set_batch(edges, n_nodes: int):
    """edges i64 [E, 2] (source, target; batch node offsets applied) on the device -> (idxn i64 [E], degs i64 [N],
    perm i64 [E]): edges ordered by target (stable), see include/spg_hip.h."""
    _req(edges, torch.int64, 'edges')
    E = int(edges.shape[0])
    dev = edges.device
    idxn = torch.empty(E, dtype=torch.int64, device=dev)
    perm = torch.empty(E, dtype=torch.int64, device=dev)
    degs = torch.empty(n_nodes, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib().spg_set_batch_workspace_bytes(n_nodes, E), dtype=torch.uint8, device=dev)
    check(lib().spg_set_batch(_ptr(edges) if E else None, n_nodes, E, _ptr(idxn) if E else None, _ptr(degs), _ptr(perm) if E else None,
                              _ptr(ws), _ptr(err), _stream()), 'spg_set_batch')
    return idxn, degs, perm, err


def batch_graph_fits(n_nodes: int, n_edges: int, n_feat: int) -> bool:
    """True when the single-launch batch builder serves a batch of this size (include/spg_hip.h: spg_batch_graph_scratch_bytes)."""
    return n_edges > 0 and lib().spg_batch_graph_scratch_bytes(int(n_nodes), int(n_edges), int(n_feat)) > 0


def batch_graph_build(edges_h: torch.Tensor, feats_h: Optional[torch.Tensor], n_nodes: int, device=None):
    """The whole construction of a small batch in one launch (include/spg_hip.h: spg_batch_graph_build / _dev): edges i64 [E, 2]
    (batch node offsets applied) and edge features f32 [E, F], both on the HOST (uploaded here) or both on the DEVICE already -> (idxn, degs, feats_sorted, DeviceGraph, error flag) on the
    device, or None when the batch is too large for the single-workgroup builder (use set_batch + gather_rows + DeviceGraph)."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    E = int(edges_h.shape[0])
    F = 0 if feats_h is None else int(feats_h.shape[1])
    L = lib()
    nscratch = L.spg_batch_graph_scratch_bytes(n_nodes, E, F)
    on_dev = edges_h.is_cuda
    if nscratch == 0 or (feats_h is not None and feats_h.is_cuda != on_dev):
        return None
    edges_h = edges_h.contiguous()
    if edges_h.dtype != torch.int64:
        raise TypeError('edges must be int64')
    if feats_h is not None:
        feats_h = feats_h.contiguous()
        if feats_h.dtype != torch.float32 or feats_h.shape[0] != E:
            raise TypeError(f'edge features must be float32 [{E}, F]')
    idxn = torch.empty(E, dtype=torch.int64, device=device)
    degs = torch.empty(n_nodes, dtype=torch.int64, device=device)
    feats = torch.empty(E, F, dtype=torch.float32, device=device) if feats_h is not None else None
    ws = torch.empty(L.spg_graph_workspace_bytes(n_nodes, n_nodes, E), dtype=torch.uint8, device=device)
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=device)
    err = torch.empty(1, dtype=torch.int32, device=device)
    # (inputs already on the device: uploaded with the batch's other small vectors by ONE upload_packed)
    check((L.spg_batch_graph_build_dev if on_dev else L.spg_batch_graph_build)(edges_h.data_ptr() if E else None, feats_h.data_ptr() if (feats_h is not None and E) else None, n_nodes, E, F,
                                  _ptr(idxn) if E else None, _ptr(degs), _ptr(feats) if (feats is not None and E) else None, _ptr(ws),
                                  _ptr(scratch), _ptr(err), _stream()), 'spg_batch_graph_build')
    return idxn, degs, feats, DeviceGraph.from_workspace(ws, idxn, degs), err


def gather_rows(src, perm):
    _req(src, torch.float32, 'src'); _req(perm, torch.int64, 'perm')
    rows, cols = int(perm.numel()), int(src.shape[1])
    dst = torch.empty(rows, cols, dtype=torch.float32, device=src.device)
    check(lib().spg_gather_rows(_ptr(src), cols, _ptr(perm), rows, cols, _ptr(dst), cols, _stream()), 'spg_gather_rows')
    return dst


_EF_KIND = {'': 0, 'copy': 0, 'd': 1, 'ld': 2, 'r': 3, 'const': 4}


def edge_features(columns, edges, mean=None, scale=None):
    """columns: list of (kind, tensor or None, column) per OUTPUT column with kind in copy|d|ld|r|const; the tensor is a
    float32 / float64 device matrix (per edge for copy, per node otherwise).  edges i64 [E, 2]; mean / scale f64 [ncols]."""
    _req(edges, torch.int64, 'edges')
    specs = _lib.EdgeFeatureSpecs()
    if len(columns) > _lib.SPG_EF_MAX_COLS:
        raise ValueError('too many edge feature columns')
    specs.ncols = len(columns)
    keep = []
    for i, (kind, t, col) in enumerate(columns):
        sp = specs.col[i]
        sp.kind = _EF_KIND[kind]
        if t is not None:
            _req(t, name='attribute')
            if t.dtype not in (torch.float32, torch.float64) or t.dim() != 2:
                raise TypeError('attributes must be 2-d float32 / float64 matrices')
            sp.data, sp.ld, sp.column, sp.is_f64 = t.data_ptr(), t.shape[1], int(col), int(t.dtype == torch.float64)
            keep.append(t)
    E = int(edges.shape[0])
    out = torch.empty(E, len(columns), dtype=torch.float32, device=edges.device)
    check(lib().spg_edge_features(ctypes.byref(specs), _ptr(edges) if E else None, E, _ptr(mean), _ptr(scale), _ptr(out), _stream()),
          'spg_edge_features')
    return out


# --------------------------------------------------------------------------------------------------
# superpoint loader
# --------------------------------------------------------------------------------------------------
def load_superpoints(points, offsets, slot, sample_idx, colmap, xyznormalize: bool, n_valid: int, M=None, noise=None):
    """points f32 [Ntot, ncols], offsets i64 [S+1], slot i32 [S], sample_idx i32 [S, npts] (on the device), colmap:
    sequence of raw column indices (host) -> clouds f32 [n_valid, F, npts], diam f32 [n_valid].
    M: f64 [S, 3, 3] or None, noise: f32 [n_valid, npts, F] or None (device)."""
    _req(points, torch.float32, 'points'); _req(offsets, torch.int64, 'offsets'); _req(slot, torch.int32, 'slot')
    _req(sample_idx, torch.int32, 'sample_idx')
    colmap_h = (ctypes.c_int32 * len(colmap))(*[int(c) for c in colmap])
    S, npts, F = slot.numel(), sample_idx.shape[1], len(colmap)
    if offsets.numel() != S + 1 or sample_idx.shape[0] != S:
        raise ValueError('offsets / slot / sample_idx disagree on the number of superpoints')
    if M is not None:
        _req(M, torch.float64, 'M')
    if noise is not None:
        _req(noise, torch.float32, 'noise')
    clouds = torch.empty(n_valid, F, npts, dtype=torch.float32, device=points.device)
    diam = torch.empty(n_valid, dtype=torch.float32, device=points.device)
    check(lib().spg_load_superpoints(_ptr(points), points.shape[1], _ptr(offsets), S, _ptr(slot), _ptr(sample_idx), npts,
                                     int(bool(xyznormalize)), ctypes.cast(colmap_h, ctypes.c_void_p), F, _ptr(M), _ptr(noise), _ptr(clouds),
                                     _ptr(diam), _stream()), 'spg_load_superpoints')
    return clouds, diam


def loader_random(counts, ids, slot, npts: int, nfeat: int, n_valid: int, seed: int, step: int, augment: bool,
                  scale: float = 0.0, rot: bool = False, mirror_prob: float = 0.0, jitter: bool = False):
    """The loader's random streams generated on the device (Philox4x32-10 keyed by (seed, superpoint id, step)):
    counts / ids i64 [S], slot i32 [S] -> sample_idx i32 [S, npts], M f64 [S, 3, 3] or None, noise f32 [n_valid, npts, nfeat]
    or None -- the inputs of `load_superpoints` (reference learning/spg.py:207-214, 241-257)."""
    _req(counts, torch.int64, 'counts'); _req(ids, torch.int64, 'ids'); _req(slot, torch.int32, 'slot')
    S = slot.numel()
    if counts.numel() != S or ids.numel() != S:
        raise ValueError('counts / ids / slot disagree on the number of superpoints')
    dev = counts.device
    sidx = torch.empty(S, npts, dtype=torch.int32, device=dev)
    M = torch.empty(S, 3, 3, dtype=torch.float64, device=dev) if augment else None
    noise = torch.empty(n_valid, npts, nfeat, dtype=torch.float32, device=dev) if (augment and jitter) else None
    check(lib().spg_loader_random(_ptr(counts), _ptr(ids), _ptr(slot), S, int(npts), int(nfeat), int(seed) & (2 ** 64 - 1),
                                  int(step) & 0xFFFFFFFF, int(bool(augment)), float(scale), int(bool(rot)), float(mirror_prob),
                                  int(bool(jitter)), _ptr(sidx), _ptr(M), _ptr(noise), _stream()), 'spg_loader_random')
    return sidx, M, noise


# --------------------------------------------------------------------------------------------------
# loss
# --------------------------------------------------------------------------------------------------
class _CrossEntropyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, mean):
        logits = _req(logits.contiguous(), torch.float32, 'logits')
        target = _req(target.contiguous(), torch.int64, 'target')
        N, C = logits.shape
        buf = torch.empty(N + 2, dtype=torch.float32, device=logits.device)          # lse [N] | loss | normaliser
        check(lib().spg_cross_entropy_fwd(_ptr(logits), _ptr(target), _ptr(weight), N, C, int(ignore_index), int(mean),
                                          buf[N:].data_ptr(), _ptr(buf), buf[N + 1:].data_ptr(), _stream()), 'spg_cross_entropy_fwd')
        ctx.save_for_backward(logits, target, buf)
        ctx.weight, ctx.ignore_index, ctx.mean = weight, int(ignore_index), int(mean)
        _CrossEntropyFunction.last_normaliser = buf[N + 1:N + 2]      # sum of the class weights of the labelled rows (device)
        return buf[N]

    @staticmethod
    def backward(ctx, grad_loss):
        logits, target, buf = ctx.saved_tensors
        N, C = logits.shape
        g = torch.empty_like(logits)
        grad_loss = grad_loss.contiguous().float()
        check(lib().spg_cross_entropy_bwd(_ptr(logits), _ptr(target), _ptr(ctx.weight), _ptr(buf), buf[N + 1:].data_ptr(), _ptr(grad_loss),
                                          N, C, ctx.ignore_index, ctx.mean, _ptr(g), _stream()), 'spg_cross_entropy_bwd')
        return g, None, None, None, None


def cross_entropy(logits, target, weight=None, ignore_index=-100, reduction='mean', return_normaliser=False):
    """torch.nn.functional.cross_entropy for [N, C] logits and class-index targets (the form learning/main.py:205 uses),
    forward and backward one HIP launch each.  return_normaliser: also the [1] device tensor sum_i weight[target_i] over the
    labelled rows -- the loss weight w_r of a data-parallel rank (superpoint_graph_amd/dist.py), without a host copy."""
    if reduction not in ('mean', 'sum'):
        raise NotImplementedError("reduction must be 'mean' or 'sum'")
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise ValueError('cross_entropy expects logits [N, C] and targets [N]')
    if weight is not None:
        weight = _req(weight.contiguous(), torch.float32, 'weight')
    loss = _CrossEntropyFunction.apply(logits, target, weight, ignore_index, reduction == 'mean')
    if return_normaliser:
        return loss, _CrossEntropyFunction.last_normaliser
    return loss


# --------------------------------------------------------------------------------------------------
# evaluation accounting
# --------------------------------------------------------------------------------------------------
def eval_accumulate(logits, label_mode, label_vec, confusion, counters):
    """logits f32 [N, C] or [S, N, C]; label_mode i64 [N]; label_vec i64 [N, C]; confusion i64 [C, C] and counters i64 [2]
    are accumulated in place.  Returns pred i64 [N]."""
    _req(logits, torch.float32, 'logits'); _req(label_mode, torch.int64, 'label_mode'); _req(label_vec, torch.int64, 'label_vec')
    _req(confusion, torch.int64, 'confusion'); _req(counters, torch.int64, 'counters')
    S = 1 if logits.dim() == 2 else logits.shape[0]
    N, C = logits.shape[-2], logits.shape[-1]
    if label_vec.shape != (N, C) or label_mode.shape != (N,) or confusion.shape != (C, C):
        raise ValueError('shapes: logits [S,]N,C; label_vec N,C; label_mode N; confusion C,C')
    pred = torch.empty(N, dtype=torch.int64, device=logits.device)
    check(lib().spg_eval_accumulate(_ptr(logits), S, N * C, N, C, _ptr(label_mode), _ptr(label_vec), _ptr(pred),
                                    _ptr(confusion), _ptr(counters), _stream()), 'spg_eval_accumulate')
    return pred


# --------------------------------------------------------------------------------------------------
# superpoint-graph construction (partition/graphs.py compute_sp_graph after the triangulation, ply_c compute_geof)
# --------------------------------------------------------------------------------------------------
def _u8_workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def sp_graph(xyz, comp, n_com: int, tets, d_max: float, labels=None, label_rows=None, n_labels: int = 0):
    """xyz f32 [n,3], comp i32 [n], tets i32 [T,4] (Delaunay simplices), all on the device -> dict of device tensors with the
    keys of the reference's compute_sp_graph (partition/graphs.py:75-210).  Three host synchronisations (the numbers of raw
    interface pairs, unique edges and superedges size the next stage's buffers)."""
    _req(xyz, torch.float32, 'xyz'); _req(comp, torch.int32, 'comp'); _req(tets, torch.int32, 'tets')
    L, dev, st = lib(), xyz.device, _stream()
    n, T = int(xyz.shape[0]), int(tets.shape[0])
    if xyz.dim() != 2 or xyz.shape[1] != 3 or comp.numel() != n or (T and tets.shape[1] != 4):
        raise ValueError('sp_graph: xyz [n,3], comp [n], tets [T,4] expected')
    u64, f32 = torch.int64, torch.float32                 # (torch has no uint64 arithmetic: int64 storage, the library reads it unsigned)
    cnt = torch.zeros(1, dtype=u64, device=dev)
    # ---- superpoints (graphs.py:141-172) ----
    out = {'sp_centroids': torch.empty(n_com, 3, dtype=f32, device=dev), 'sp_length': torch.empty(n_com, 1, dtype=f32, device=dev),
           'sp_surface': torch.empty(n_com, 1, dtype=f32, device=dev), 'sp_volume': torch.empty(n_com, 1, dtype=f32, device=dev),
           'sp_point_count': torch.empty(n_com, 1, dtype=u64, device=dev)}
    sp_labels = None
    if labels is not None or label_rows is not None:
        sp_labels = torch.empty(n_com, n_labels + 1, dtype=torch.int32, device=dev)
        if labels is not None:
            _req(labels, torch.int32, 'labels')
        else:
            _req(label_rows, torch.int32, 'label_rows')
    ws = _u8_workspace(L.spg_spg_workspace_bytes(2, n), dev)
    check(L.spg_spg_superpoints(_ptr(xyz), n, _ptr(comp), n_com, _ptr(labels), _ptr(label_rows), n_labels, _ptr(out['sp_centroids']),
                                _ptr(out['sp_length']), _ptr(out['sp_surface']), _ptr(out['sp_volume']), _ptr(out['sp_point_count']),
                                _ptr(sp_labels), _ptr(ws), ws.numel(), st), 'spg_spg_superpoints')
    out['sp_labels'] = sp_labels
    # ---- interface edges of the tetrahedra, unique, shorter than d_max (:85-113) ----
    keys = torch.empty(max(12 * T, 1), dtype=u64, device=dev)
    check(L.spg_spg_tet_edges(_ptr(tets) if T else None, T, _ptr(comp), _ptr(keys), 12 * T, _ptr(cnt), st), 'spg_spg_tet_edges')
    n_raw = int(cnt.item())
    edge_keys = torch.empty(max(n_raw, 1), dtype=u64, device=dev)
    cc_keys = torch.empty(max(n_raw, 1), dtype=u64, device=dev)
    ws = _u8_workspace(L.spg_spg_workspace_bytes(0, n_raw), dev)
    check(L.spg_spg_unique_edges(_ptr(keys), n_raw, _ptr(xyz), _ptr(comp), n_com, float(d_max), _ptr(edge_keys), _ptr(cc_keys), _ptr(cnt),
                                 _ptr(ws), ws.numel(), st), 'spg_spg_unique_edges')
    n_edg = int(cnt.item())
    # ---- ordered by component pair, superedge segments (:117-128) ----
    cc_sorted = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    edges_sorted = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    seg_cc = torch.empty(max(n_edg, 1), dtype=u64, device=dev)
    seg_off = torch.empty(n_edg + 1, dtype=u64, device=dev)
    ws = _u8_workspace(L.spg_spg_workspace_bytes(1, n_edg), dev)
    check(L.spg_spg_group_edges(_ptr(cc_keys), _ptr(edge_keys), n_edg, _ptr(cc_sorted), _ptr(edges_sorted), _ptr(seg_cc), _ptr(seg_off),
                                _ptr(cnt), _ptr(ws), ws.numel(), st), 'spg_spg_group_edges')
    n_sedg = int(cnt.item())
    # ---- superedge features (:174-208) ----
    se = {'source': torch.empty(n_sedg, 1, dtype=torch.int32, device=dev), 'target': torch.empty(n_sedg, 1, dtype=torch.int32, device=dev)}
    for k, w in (('se_delta_mean', 3), ('se_delta_std', 3), ('se_delta_norm', 1), ('se_delta_centroid', 3), ('se_length_ratio', 1),
                 ('se_surface_ratio', 1), ('se_volume_ratio', 1), ('se_point_count_ratio', 1)):
        se[k] = torch.empty(n_sedg, w, dtype=f32, device=dev)
    check(L.spg_spg_superedges(_ptr(edges_sorted), _ptr(seg_cc), _ptr(seg_off), n_sedg, n_com, _ptr(xyz), _ptr(out['sp_centroids']),
                               _ptr(out['sp_length']), _ptr(out['sp_surface']), _ptr(out['sp_volume']), _ptr(out['sp_point_count']),
                               _ptr(se['source']), _ptr(se['target']), _ptr(se['se_delta_mean']), _ptr(se['se_delta_std']),
                               _ptr(se['se_delta_norm']), _ptr(se['se_delta_centroid']), _ptr(se['se_length_ratio']),
                               _ptr(se['se_surface_ratio']), _ptr(se['se_volume_ratio']), _ptr(se['se_point_count_ratio']), st),
          'spg_spg_superedges')
    out.update(se)
    out['edges'] = edges_sorted[:n_edg]                    # (source << 32 | target) of every Delaunay edge behind the superedges
    out['seg_off'] = seg_off[:n_sedg + 1]
    return out


def compute_geof(xyz, target, k_nn: int):
    """xyz f32 [n,3], target (u)int32 [n * k_nn] neighbour indices on the device -> geof f32 [n,4] (ply_c.cpp:384-462)."""
    _req(xyz, torch.float32, 'xyz'); _req(target, torch.int32, 'target')
    n = int(xyz.shape[0])
    if target.numel() != n * k_nn:
        raise ValueError(f'compute_geof: {n} points x {k_nn} neighbours need {n * k_nn} targets, got {target.numel()}')
    geof = torch.empty(n, 4, dtype=torch.float32, device=xyz.device)
    check(lib().spg_compute_geof(_ptr(xyz), _ptr(target), n, int(k_nn), _ptr(geof), _stream()), 'spg_compute_geof')
    return geof


def prune(xyz, voxel_size: float, rgb=None, labels=None, objects=None, n_labels: int = 0, n_objects: int = 0):
    """Voxel-grid subsampling (ply_c.cpp:288-382) of device tensors: xyz f32 [n,3], rgb u8 [n,3] or None, labels u8 [n] or None,
    objects i32 [n] (read as uint32) or None -> (xyz f32 [V,3], rgb u8 [V,3], labels i32 [V, n_labels+1], objects i32 [V, n_objects+1]);
    voxels in the order of their first point.  One host synchronisation (the number of voxels)."""
    _req(xyz, torch.float32, 'xyz')
    L, dev, st = lib(), xyz.device, _stream()
    n = int(xyz.shape[0])
    if rgb is not None:
        _req(rgb, torch.uint8, 'rgb')
    if labels is not None:
        _req(labels, torch.uint8, 'labels')
    if objects is not None:
        _req(objects, torch.int32, 'objects')
    ws = _u8_workspace(L.spg_prune_workspace_bytes(n), dev)
    nv = torch.zeros(1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.spg_prune_voxels(_ptr(xyz), n, float(voxel_size), _ptr(nv), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_prune_voxels')
    V = int(nv.item())
    if int(err.item()) & 1:
        raise ValueError('prune: more than 2^21 voxels along an axis (voxel_size too small for the extent of the cloud)')
    out_xyz = torch.empty(V, 3, dtype=torch.float32, device=dev)
    out_rgb = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    out_lab = torch.empty(V, n_labels + 1, dtype=torch.int32, device=dev)
    out_obj = torch.empty(V, n_objects + 1, dtype=torch.int32, device=dev)
    check(L.spg_prune_reduce(_ptr(xyz), _ptr(rgb), _ptr(labels), _ptr(objects), n, V, int(n_labels), int(n_objects), _ptr(out_xyz),
                             _ptr(out_rgb), _ptr(out_lab), _ptr(out_obj), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_prune_reduce')
    if int(err.item()) & 2:
        raise IndexError('prune: a label / object id exceeds n_labels / n_objects')
    return out_xyz, out_rgb, out_lab, out_obj


KNN_MAX_K = 47          # k + 1 <= 48: the largest top-k list the query kernels keep in registers without scratch


class KnnIndex:
    """Exact k-nearest-neighbour index of a device point set (csrc/spg_knn.hip): ref_xyz f32 [n,3] on the GPU, indexed once
    into a uniform grid; query() / self_query() answer on the device.  Order: float64 squared distance (dx*dx + dy*dy) + dz*dz
    (no fused multiply-add), ties by point index; self queries drop the query point itself.  The results do not depend on
    cell_size (None = automatic, ~32 points per occupied cell; a value is for tuning and tests).  query_capacity: the largest
    query set the workspace is sized for in one internal chunk (larger sets are streamed in chunks)."""

    def __init__(self, ref_xyz, cell_size=None, query_capacity: int = 0):
        _req(ref_xyz, torch.float32, 'ref_xyz')
        if ref_xyz.dim() != 2 or ref_xyz.shape[1] != 3:
            raise ValueError(f'knn: ref_xyz must be [n, 3], got {tuple(ref_xyz.shape)}')
        n = int(ref_xyz.shape[0])
        if n == 0:
            raise ValueError('knn: empty reference set')
        if n >= 2 ** 32 - 1:
            raise ValueError('knn: point indices are uint32: at most 2^32 - 2 reference points')
        if cell_size is not None and not (float(cell_size) > 0.0):
            raise ValueError(f'knn: cell_size must be > 0, got {cell_size}')
        L, dev = lib(), ref_xyz.device
        self.ref, self.n = ref_xyz, n
        self.ws = _u8_workspace(L.spg_knn_workspace_bytes(n, int(query_capacity), 1), dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        check(L.spg_knn_build(_ptr(ref_xyz), n, float(cell_size or 0.0), _ptr(self.err), _ptr(self.ws), self.ws.numel(), _stream()),
              'spg_knn_build')

    def _k(self, k, n_avail):
        k = int(k)
        if k < 1:
            raise ValueError(f'knn: k must be >= 1, got {k}')
        if k + 1 > KNN_MAX_K + 1:
            raise ValueError(f'knn: k + 1 = {k + 1} exceeds the limit of {KNN_MAX_K + 1} (k <= {KNN_MAX_K})')
        if k > n_avail:
            raise ValueError(f'knn: Expected n_neighbors <= n_samples, but n_samples = {self.n}, n_neighbors = '
                             f'{k + 1 if n_avail < self.n else k}')
        return k

    def _run(self, q, nq, k, self_query, distances):
        dev = self.ref.device
        idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
        dist = torch.empty(nq, k, dtype=torch.float32, device=dev) if distances else None
        check(lib().spg_knn_query(_ptr(q), nq, self.n, k, int(self_query), _ptr(idx), _ptr(dist), _ptr(self.err), _ptr(self.ws),
                                  self.ws.numel(), _stream()), 'spg_knn_query')
        if int(self.err.item()) & 1:
            raise ValueError('knn: the input contains NaN or infinity')
        return idx, dist

    def query_chunk(self, n_query: int) -> int:
        """queries per internal chunk that query() uses for n_query queries on this index's workspace."""
        return int(lib().spg_knn_query_chunk(self.n, int(n_query), self.ws.numel()))

    def self_query(self, k, distances=True):
        """k nearest other points of every reference point -> (idx i32 [n, k], dist f32 [n, k] or None)."""
        return self._run(None, self.n, self._k(k, self.n - 1), True, distances)

    def query(self, query_xyz, k, distances=True):
        """k nearest reference points of every query point -> (idx i32 [m, k], dist f32 [m, k] or None)."""
        _req(query_xyz, torch.float32, 'query_xyz')
        if query_xyz.dim() != 2 or query_xyz.shape[1] != 3:
            raise ValueError(f'knn: query_xyz must be [m, 3], got {tuple(query_xyz.shape)}')
        nq = int(query_xyz.shape[0])
        if nq >= 2 ** 32 - 1:
            raise ValueError('knn: at most 2^32 - 2 query points per call')
        return self._run(query_xyz, nq, self._k(k, self.n), False, distances)


def knn(ref_xyz, k: int, query_xyz=None, cell_size=None, distances: bool = True):
    """Exact k nearest neighbours on the device (sklearn NearestNeighbors(algorithm='kd_tree') in the reference's
    partition/graphs.py:11-73 and provider.py:681-687).  ref_xyz f32 [n,3]; query_xyz f32 [m,3] or None = self query (the point
    itself is dropped) -> (idx int32 [m, k], distances float32 [m, k] or None), in query order.  1 <= k <= KNN_MAX_K."""
    index = KnnIndex(ref_xyz, cell_size, 0 if query_xyz is None else int(query_xyz.shape[0]))
    if query_xyz is None:
        return index.self_query(k, distances)
    return index.query(query_xyz, k, distances)


# --------------------------------------------------------------------------------------------------
# graph contrastive loss of the learned partition (csrc/spg_edgeloss.hip; reference supervized_partition/losses.py)
# --------------------------------------------------------------------------------------------------
EDGE_MAX_D = 64
_DIST_TYPES = {'euclidian': 0, 'intrinsic': 1, 'scalar': 2}


def _dist_code(dist_type):
    if dist_type not in _DIST_TYPES:
        raise ValueError(" %s is an unknown argument of parameter --dist_type" % (dist_type))
    return _DIST_TYPES[dist_type]


def _loss_codes(loss):
    """(intra, inter) of a --loss string, by the reference's substring tests in their order (losses.py:46-61)."""
    if 'tv' in loss:
        intra = 0
    elif 'laplacian' in loss:
        intra = 1
    elif 'TVH' in loss:
        intra = 2
    else:
        raise ValueError(" %s is an unknown argument of parameter --loss" % (loss))
    if 'zhang' in loss:
        inter = 0
    elif 'TVminus' in loss:
        inter = 1
    else:
        raise ValueError(" %s is an unknown argument of parameter --loss" % (loss))
    return intra, inter


class EdgeGraph:
    """Edges of one batch on the device with their per-vertex incidence CSR (built once, used by the loss forward, its
    atomic-free backward, connected_components and crosspartition_weights): src / tgt int64 [E] device tensors, n vertices.
    rowptr i32 [n + 1]; inc i32 [2E] = edge << 1 | side (side 0: the vertex is the edge's source), ascending edge id inside a
    vertex; ends i32 [E, 2].  One host synchronisation (the range check of the indices).  build() may be called again with
    other edges; after an IndexError the object holds no graph until a build() succeeds."""

    def __init__(self, src, tgt, n: int):
        self.n, self.E, self.valid = int(n), 0, False
        self.build(src, tgt)

    def build(self, src, tgt):
        src = _req(src, torch.int64, 'src'); tgt = _req(tgt, torch.int64, 'tgt')
        if src.dim() != 1 or src.shape != tgt.shape:
            raise ValueError(f'EdgeGraph: src and tgt must be [E], got {tuple(src.shape)} and {tuple(tgt.shape)}')
        n, E = self.n, int(src.numel())
        if not (1 <= n < 2 ** 31 - 1 and E < 2 ** 30):
            raise ValueError(f'EdgeGraph: 1 <= n < 2^31 - 1 and E < 2^30 expected, got n = {n}, E = {E}')
        L, dev = lib(), src.device
        self.valid = False
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        inc = torch.empty(2 * E, dtype=torch.int32, device=dev)
        ends = torch.empty(E, 2, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _u8_workspace(L.spg_edgegraph_workspace_bytes(n, E), dev)
        check(L.spg_edgegraph_build(_ptr(src), _ptr(tgt), E, n, _ptr(rowptr), _ptr(inc), _ptr(ends), _ptr(err), _ptr(ws), ws.numel(),
                                    _stream()), 'spg_edgegraph_build')
        if int(err.item()) & 1:
            raise IndexError(f'EdgeGraph: an edge index is outside [0, {n})')
        self.E, self.rowptr, self.inc, self.ends, self.device = E, rowptr, inc, ends, dev
        self.valid = True
        return self

    def _use(self):
        if not self.valid:
            raise RuntimeError('EdgeGraph: the last build() failed; build() it again before use')
        return self


def _edge_forward(mode, emb, graph, dist_code, intra, inter, is_transition, weights, diff):
    """-> (diff, dx, dl, loss f64 [2]) of spg_edge_forward (mode 1: diff; 2: loss from diff, graph = None; 3: both)."""
    L = lib()
    E, dev = (graph.E, graph.device) if graph is not None else (int(diff.numel()), diff.device)
    f32 = torch.float32
    dx = dl = loss = ws = None
    if mode & 1:
        diff = torch.empty(E, dtype=f32, device=dev)
        dx = torch.empty(E, dtype=f32, device=dev) if dist_code == 1 else None
    if mode & 2:
        dl = torch.empty(E, dtype=f32, device=dev)
        loss = torch.empty(2, dtype=torch.float64, device=dev)
        ws = _u8_workspace(L.spg_edge_forward_workspace_bytes(E), dev)
    n, d = (int(emb.shape[0]), int(emb.shape[1])) if emb is not None else (1, 1)
    check(L.spg_edge_forward(mode, _ptr(emb), n, d, _ptr(graph.ends) if graph is not None else None, E, dist_code, intra, inter, _ptr(is_transition), _ptr(weights),
                             _ptr(diff), _ptr(dx), _ptr(dl), _ptr(loss), _ptr(ws), ws.numel() if ws is not None else 0, _stream()),
          'spg_edge_forward')
    return diff, dx, dl, loss


def _edge_backward(emb, graph, dist_code, dl, is_transition, up, gdiff, dx):
    grad = torch.empty_like(emb)
    check(lib().spg_edge_backward(_ptr(emb), int(emb.shape[0]), int(emb.shape[1]), _ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends),
                                  graph.E, dist_code, _ptr(dl), _ptr(is_transition), _ptr(up), _ptr(gdiff), _ptr(dx), _ptr(grad),
                                  _stream()), 'spg_edge_backward')
    return grad


def _emb_arg(emb, graph):
    emb = _req(emb.contiguous(), torch.float32, 'embeddings')
    if emb.dim() != 2 or emb.shape[0] != graph.n:
        raise ValueError(f'embeddings must be [{graph.n}, d], got {tuple(emb.shape)}')
    if not 1 <= emb.shape[1] <= EDGE_MAX_D:
        raise ValueError(f'embeddings: 1 <= d <= {EDGE_MAX_D} expected, got d = {emb.shape[1]}')
    return emb


def _edge_vec(t, dtype, E, name):
    t = _req(t.contiguous() if t.dtype == dtype else t.to(dtype).contiguous(), dtype, name)
    if t.shape != (E,):
        raise ValueError(f'{name} must be [{E}], got {tuple(t.shape)}')
    return t


def _up_pair(g1, g2, dev):
    z = torch.zeros((), dtype=torch.float32, device=dev)
    return torch.stack([z if g1 is None else g1.float().reshape(()), z if g2 is None else g2.float().reshape(())])


class _EdgeDistFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, dist_code):
        emb = _emb_arg(emb, graph)
        diff, dx, _, _ = _edge_forward(1, emb, graph, dist_code, 0, 0, None, None, None)
        ctx.save_for_backward(emb, dx)
        ctx.graph, ctx.dist_code = graph, dist_code
        return diff

    @staticmethod
    def backward(ctx, grad_diff):
        emb, dx = ctx.saved_tensors
        gdiff = _req(grad_diff.contiguous(), torch.float32, 'grad_diff')
        return _edge_backward(emb, ctx.graph._use(), ctx.dist_code, None, None, None, gdiff, dx), None, None


class _EdgeLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, diff, is_transition, weights, intra, inter, dist_code):
        diff = _req(diff.contiguous(), torch.float32, 'diff')
        _, _, dl, loss = _edge_forward(2, None, None, dist_code, intra, inter, is_transition, weights, diff)
        ctx.save_for_backward(dl, is_transition)
        loss = loss.float()
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g1, g2):
        dl, is_transition = ctx.saved_tensors
        gdiff = torch.empty_like(dl)
        up = _up_pair(g1, g2, dl.device)
        check(lib().spg_edge_loss_backward(_ptr(dl), _ptr(is_transition), _ptr(up), dl.numel(), _ptr(gdiff), _stream()),
              'spg_edge_loss_backward')
        return gdiff, None, None, None, None, None


class _ContrastiveEdgeLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, graph, is_transition, weights, intra, inter, dist_code):
        emb = _emb_arg(emb, graph)
        diff, dx, dl, loss = _edge_forward(3, emb, graph, dist_code, intra, inter, is_transition, weights, None)
        ctx.save_for_backward(emb, dx, dl, is_transition)
        ctx.graph, ctx.dist_code = graph, dist_code
        loss = loss.float()
        return loss[0], loss[1], diff

    @staticmethod
    def backward(ctx, g1, g2, grad_diff):
        emb, dx, dl, is_transition = ctx.saved_tensors
        up = _up_pair(g1, g2, emb.device)
        gdiff = None if grad_diff is None else _req(grad_diff.contiguous(), torch.float32, 'grad_diff')
        return (_edge_backward(emb, ctx.graph._use(), ctx.dist_code, dl, is_transition, up, gdiff, dx),
                None, None, None, None, None, None)


def edge_dist(embeddings, graph: EdgeGraph, dist_type='euclidian'):
    """compute_dist (losses.py:31-42): embeddings f32 [n, d <= 64] -> diff f32 [E]; differentiable (atomic-free backward)."""
    code = _dist_code(dist_type)
    return _EdgeDistFunction.apply(embeddings, graph._use(), code)


def edge_loss(diff, is_transition, weights, loss='TVH_zhang', dist_type='euclidian'):
    """compute_loss (losses.py:44-64) from a given diff f32 [E] -> (loss1, loss2), float64 sums in a fixed order returned as
    float32 scalars; differentiable wrt diff."""
    intra, inter = _loss_codes(loss)
    code = _dist_code(dist_type)
    _on_gpu(diff, 'diff')
    if diff.dim() != 1:
        raise ValueError(f'diff must be [E], got {tuple(diff.shape)}')
    E = int(diff.numel())
    return _EdgeLossFunction.apply(diff, _edge_vec(is_transition, torch.uint8, E, 'is_transition'),
                                   _edge_vec(weights, torch.float32, E, 'weights'), intra, inter, code)


def contrastive_edge_loss(embeddings, graph: EdgeGraph, is_transition, weights, loss='TVH_zhang', dist_type='euclidian'):
    """compute_dist + compute_loss in one launch over the edges -> (loss1, loss2, diff), bit-identical to edge_dist followed by
    edge_loss; the backward is one launch over the vertices through the incidence CSR (no atomics, deterministic)."""
    intra, inter = _loss_codes(loss)
    code = _dist_code(dist_type)
    graph._use()
    _on_gpu(embeddings, 'embeddings')
    return _ContrastiveEdgeLossFunction.apply(embeddings, graph, _edge_vec(is_transition, torch.uint8, graph.E, 'is_transition'),
                                              _edge_vec(weights, torch.float32, graph.E, 'weights'), intra, inter, code)


def connected_components(graph: EdgeGraph, active):
    """Components of the vertices over the edges with active != 0 (libply_c.connected_comp with cutoff 0) ->
    (in_component i32 [n], n_components int, component_size i32 [n_components]), numbered by ascending smallest member."""
    graph._use()
    active = _edge_vec(active, torch.uint8, graph.E, 'active')
    L, dev, n = lib(), graph.device, graph.n
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    ncomp = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _u8_workspace(L.spg_cc_workspace_bytes(n), dev)
    check(L.spg_connected_components(_ptr(graph.ends), _ptr(active), graph.E, n, _ptr(comp), _ptr(size), _ptr(ncomp), _ptr(ws),
                                     ws.numel(), _stream()), 'spg_connected_components')
    k = int(ncomp.item())
    return comp, k, size[:k]


def crosspartition_weights(graph: EdgeGraph, pred_in_component, is_transition, factor, return_components=False):
    """compute_weights_XPART (losses.py:130-166): pred_in_component integer [n] (the predicted partition), is_transition [E]
    -> weights f32 [E]: 1 + min(size_a, size_b) / count(pair) * factor on transition edges (float64, rounded once), 1 elsewhere;
    a, b are the components over the edges that neither the truth nor the prediction cuts.
    return_components: also (in_component_x i32 [n], n_components int, component_size i32)."""
    graph._use()
    is_transition = _edge_vec(is_transition, torch.uint8, graph.E, 'is_transition')
    _on_gpu(pred_in_component, 'pred_in_component')
    pred = _req(pred_in_component.to(torch.int32).contiguous(), torch.int32, 'pred_in_component')
    L, dev, n = lib(), graph.device, graph.n
    if pred.shape != (n,):
        raise ValueError(f'pred_in_component must be [{n}], got {tuple(pred.shape)}')
    w = torch.empty(graph.E, dtype=torch.float32, device=dev)
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    ncomp = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _u8_workspace(L.spg_xpart_workspace_bytes(n, graph.E), dev)
    check(L.spg_xpart_weights(_ptr(graph.ends), graph.E, n, _ptr(pred), _ptr(is_transition), float(factor), _ptr(w), _ptr(comp),
                              _ptr(size), _ptr(ncomp), _ptr(ws), ws.numel(), _stream()), 'spg_xpart_weights')
    if return_components:
        k = int(ncomp.item())
        return w, comp, k, size[:k]
    return w


# --------------------------------------------------------------------------------------------------
# evaluation of a predicted partition and the SEAL weights (csrc/spg_parteval.hip; reference supervized_partition/
# supervized_partition.py:248-375, partition/provider.py:689-695, learning/metrics.py:87-108, losses.py:119-128, :168-186)
# --------------------------------------------------------------------------------------------------
PARTEVAL_MAX_CLASSES = 64
_RELAX_MODES = {'reference': 0, 'symmetric': 1}


def _vertex_vec(t, n, name):
    """An integer [n] device tensor as contiguous int32 (the values must fit: ids and labels below 2^31)."""
    _on_gpu(t, name)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f'{name} must be an integer tensor, got {t.dtype}')
    if t.shape != (n,):
        raise ValueError(f'{name} must be [{n}], got {tuple(t.shape)}')
    return _req(t.to(torch.int32).contiguous(), torch.int32, name)


def _indicator(t, E, name):
    """A bool / uint8 [E] device tensor as contiguous uint8 (bool is reinterpreted, not copied)."""
    _on_gpu(t, name)
    if t.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f'{name} must be bool or uint8, got {t.dtype}')
    if t.shape != (E,):
        raise ValueError(f'{name} must be [{E}], got {tuple(t.shape)}')
    t = t.contiguous()
    return _req(t.view(torch.uint8) if t.dtype == torch.bool else t, torch.uint8, name)


def _raise_partition_flag(flag, n_com):
    f = int(flag.item())
    if f & 1:
        raise IndexError(f'a component id is outside [0, {n_com})')
    if f & 2:
        raise ValueError('values must be non-negative')


class PartitionIndex:
    """A partition of n vertices given by in_component integer [n] (device) and n_com: order i32 [n] = the vertices by
    component, ascending inside a component (np.flatnonzero(in_component == c) is order[offsets[c]:offsets[c + 1]]), offsets
    i32 [n_com + 1], size i32 [n_com].  An id no vertex carries is a component of size 0; an id outside [0, n_com) raises
    IndexError (one host synchronisation; _flag: a device int32 the caller reads later instead)."""

    def __init__(self, in_component, n_com: int, _flag=None):
        if not torch.is_tensor(in_component) or in_component.dim() != 1:
            raise ValueError('PartitionIndex: in_component must be a [n] tensor')
        n, n_com = int(in_component.numel()), int(n_com)
        if not (1 <= n < 2 ** 31 - 1 and 1 <= n_com < 2 ** 31 - 1):
            raise ValueError(f'PartitionIndex: 1 <= n, n_com < 2^31 - 1 expected, got n = {n}, n_com = {n_com}')
        comp = _vertex_vec(in_component, n, 'in_component')
        L, dev = lib(), comp.device
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if _flag is None else _flag
        order = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n_com + 1, dtype=torch.int32, device=dev)
        size = torch.empty(n_com, dtype=torch.int32, device=dev)
        ws = _u8_workspace(L.spg_partition_index_workspace_bytes(n, n_com), dev)
        check(L.spg_partition_index(_ptr(comp), n, n_com, _ptr(order), _ptr(offsets), _ptr(size), _ptr(flag), _ptr(ws), ws.numel(),
                                    _stream()), 'spg_partition_index')
        if _flag is None:
            _raise_partition_flag(flag, n_com)
        self.n, self.n_com, self.device = n, n_com, dev
        self.in_component, self.order, self.offsets, self.size = comp, order, offsets, size


def _label_majority(index, labels):
    _on_gpu(labels, 'labels')
    if labels.dim() != 2 or labels.shape[0] != index.n or labels.shape[1] < 2:
        raise ValueError(f'labels must be [{index.n}, C + 1] (column 0 = unlabelled), got {tuple(labels.shape)}')
    C = int(labels.shape[1]) - 1
    if C > PARTEVAL_MAX_CLASSES:
        raise ValueError(f'labels: at most {PARTEVAL_MAX_CLASSES} classes, got C = {C}')
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise TypeError(f'labels must be an integer tensor, got {labels.dtype}')
    # uint32 counts: int32 storage holds the same 32 bits (torch has no uint32 arithmetic)
    lab = _req(labels.contiguous() if labels.dtype in (torch.int32, getattr(torch, 'uint32', torch.int32)) else labels.to(torch.int32).contiguous(), None, 'labels')
    dev, n_com = index.device, index.n_com
    sums = torch.empty(n_com, C, dtype=torch.int64, device=dev)
    label_com = torch.empty(n_com, dtype=torch.int32, device=dev)
    full_pred = torch.empty(index.n, dtype=torch.int32, device=dev)
    confusion = torch.empty(C, C, dtype=torch.int64, device=dev)
    check(lib().spg_component_label_majority(_ptr(lab), index.n, C, _ptr(index.in_component), _ptr(index.order), n_com, _ptr(sums),
                                             _ptr(label_com), _ptr(full_pred), _ptr(confusion), _stream()), 'spg_component_label_majority')
    return dict(sums=sums, label_com=label_com, full_pred=full_pred, confusion=confusion)


def component_label_majority(index: PartitionIndex, labels):
    """perfect_prediction (partition/provider.py:689-695) and its confusion matrix: labels integer [n, C + 1] per-point label
    histograms (column 0 = unlabelled, left out), C <= 64 -> dict(sums i64 [n_com, C], label_com i32 [n_com] = first arg-max
    (0 for an all-zero row), full_pred i32 [n] (the uint32 labels of the reference), confusion i64 [C, C] with
    confusion[:, label_com[c]] += sums[c, :] = ConfusionMatrix.count_predicted_batch(labels[:, 1:], full_pred))."""
    if not isinstance(index, PartitionIndex):
        raise TypeError('component_label_majority: index must be a PartitionIndex')
    return _label_majority(index, labels)


def _component_mode(in_component, values, n_com, flag):
    n = int(in_component.numel())
    vals = _vertex_vec(values, n, 'values')
    L, dev = lib(), in_component.device
    freq = torch.empty(n_com, dtype=torch.int32, device=dev)
    value = torch.empty(n_com, dtype=torch.int32, device=dev)
    ws = _u8_workspace(L.spg_component_mode_workspace_bytes(n, n_com), dev)
    check(L.spg_component_mode(_ptr(in_component), _ptr(vals), n, n_com, _ptr(freq), _ptr(value), _ptr(flag), _ptr(ws), ws.numel(),
                               _stream()), 'spg_component_mode')
    return freq, value


def component_mode(index: PartitionIndex, values):
    """mode() of every component (losses.py:168-173, metrics.py:95-100): values integer [n], 0 <= value < 2^31 ->
    (freq i32 [n_com] = count of the most frequent value, value i32 [n_com] = the smallest of the most frequent); an empty
    component gives 0 and -1.  One host synchronisation (negative values raise ValueError)."""
    if not isinstance(index, PartitionIndex):
        raise TypeError('component_mode: index must be a PartitionIndex')
    flag = torch.zeros(1, dtype=torch.int32, device=index.device)
    freq, value = _component_mode(index.in_component, values, index.n_com, flag)
    _raise_partition_flag(flag, index.n_com)
    return freq, value


def seal_weights(graph: EdgeGraph, index: PartitionIndex, objects, is_transition, factor):
    """compute_weights_SEAL (losses.py:119-128): index = the predicted partition, objects integer [n] >= 0 (the true object of
    every vertex), is_transition [E] -> weights f32 [E]: float32(1 + double(max over both ends of size - mode frequency of
    their predicted component) * factor) on transition edges (float64, rounded once), 1 elsewhere.  One host synchronisation."""
    graph._use()
    if not isinstance(index, PartitionIndex):
        raise TypeError('seal_weights: index must be a PartitionIndex')
    if index.n != graph.n:
        raise ValueError(f'seal_weights: the partition has {index.n} vertices, the graph {graph.n}')
    is_transition = _edge_vec(is_transition, torch.uint8, graph.E, 'is_transition')
    flag = torch.zeros(1, dtype=torch.int32, device=index.device)
    freq, _ = _component_mode(index.in_component, objects, index.n_com, flag)
    w = torch.empty(graph.E, dtype=torch.float32, device=graph.device)
    check(lib().spg_seal_weights(_ptr(graph.ends), graph.E, graph.n, _ptr(index.in_component), _ptr(index.size), _ptr(freq), index.n_com,
                                 _ptr(is_transition), float(factor), _ptr(w), _stream()), 'spg_seal_weights')
    _raise_partition_flag(flag, index.n_com)
    return w


def _relax(graph, binary_u8, tolerance, mode_code):
    L, dev = lib(), graph.device
    out = torch.empty(graph.E, dtype=torch.uint8, device=dev)
    ws = _u8_workspace(L.spg_relax_edges_workspace_bytes(graph.n), dev)
    check(L.spg_relax_edges(_ptr(graph.ends), graph.E, graph.n, _ptr(binary_u8), tolerance, mode_code, _ptr(out), _ptr(ws), ws.numel(),
                            _stream()), 'spg_relax_edges')
    return out


def relax_edges(graph: EdgeGraph, binary, tolerance: int, mode='reference'):
    """relax_edge_binary (losses.py:175-186): binary bool / uint8 [E] -> the indicator after `tolerance` rounds of "mark both ends
    of every set edge, then set edges from the marks" (same dtype; tolerance 0 is a copy).
    mode 'symmetric': an edge is set if either of its ends is marked -- what the reference's text describes.
    mode 'reference': what the reference's function computes.  Its vertex marks are a uint8 array, so
    `relaxed_binary[transition_vertex[edg_source]] = True` is integer indexing with the values 0 and 1, not a mask: every
    round sets EDGE 1 if any edge's source is marked and EDGE 0 if any edge's source is not, and the relaxation itself spreads
    through the target ends only.  Reproduced as it is; needs E >= 2 when tolerance > 0 (ValueError), where the reference
    raises an IndexError or not, depending on the data."""
    graph._use()
    if mode not in _RELAX_MODES:
        raise ValueError(f"relax_edges: mode must be 'reference' or 'symmetric', got {mode!r}")
    tolerance = int(tolerance)
    if tolerance < 0:
        raise ValueError(f'relax_edges: tolerance >= 0 expected, got {tolerance}')
    b = _indicator(binary, graph.E, 'binary')
    if mode == 'reference' and tolerance > 0 and graph.E < 2:
        raise ValueError("relax_edges: mode 'reference' writes edges 0 and 1 and needs E >= 2")
    out = _relax(graph, b, tolerance, _RELAX_MODES[mode])
    return out.view(torch.bool) if binary.dtype == torch.bool else out


def _boundary_counts(a, b):
    counts = torch.empty(2, 2, dtype=torch.int64, device=a.device)
    check(lib().spg_boundary_counts(_ptr(a), _ptr(b), a.numel(), _ptr(counts), _stream()), 'spg_boundary_counts')
    return counts


def boundary_counts(a, b):
    """a (truth), b (prediction): bool / uint8 [E] -> counts i64 [2, 2], counts[a != 0][b != 0] (the count_predicted_batch_hard
    matrix of evaluate_final; metrics.py:87-92: recall = 100 * counts[1, 1] / (counts[1, 0] + counts[1, 1]), precision =
    100 * counts[1, 1] / (counts[0, 1] + counts[1, 1]))."""
    if not torch.is_tensor(a) or a.dim() != 1:
        raise ValueError('boundary_counts: a and b must be [E] tensors')
    E = int(a.numel())
    return _boundary_counts(_indicator(a, E, 'a'), _indicator(b, E, 'b'))


def partition_scores(graph: EdgeGraph, pred_in_component, n_com: int, is_transition, labels, tolerance: int):
    """What the body of evaluate() / evaluate_final() does with a predicted partition (supervized_partition.py:282-293,
    :335-343), on the device: -> dict(n_clusters = n_com, confusion i64 [C, C] (the ASA matrix of perfect_prediction),
    br_counts i64 [2, 2] = boundary_counts(is_transition, relaxed predicted transitions), bp_counts i64 [2, 2] =
    boundary_counts(relaxed is_transition, predicted transitions), full_pred i32 [n]); the relaxation is the reference's
    (relax_edges mode 'reference').  One host synchronisation (the range check of the component ids)."""
    graph._use()
    tolerance = int(tolerance)
    if tolerance < 0:
        raise ValueError(f'partition_scores: tolerance >= 0 expected, got {tolerance}')
    if tolerance > 0 and graph.E < 2:
        raise ValueError('partition_scores: the reference relaxation needs E >= 2')
    if not torch.is_tensor(pred_in_component) or pred_in_component.shape != (graph.n,):
        raise ValueError(f'pred_in_component must be a [{graph.n}] tensor')
    trans = _indicator(is_transition, graph.E, 'is_transition')
    dev = graph.device
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    index = PartitionIndex(pred_in_component, n_com, _flag=flag)
    maj = _label_majority(index, labels)
    pred_trans = torch.empty(graph.E, dtype=torch.uint8, device=dev)
    check(lib().spg_pred_transition(_ptr(graph.ends), graph.E, graph.n, _ptr(index.in_component), _ptr(pred_trans), _stream()),
          'spg_pred_transition')
    br = _boundary_counts(trans, _relax(graph, pred_trans, tolerance, 0))
    bp = _boundary_counts(_relax(graph, trans, tolerance, 0), pred_trans)
    _raise_partition_flag(flag, index.n_com)
    return dict(n_clusters=index.n_com, confusion=maj['confusion'], br_counts=br, bp_counts=bp, full_pred=maj['full_pred'])


# --------------------------------------------------------------------------------------------------
# batches of the learned partition on the device (csrc/spg_tiles.hip; reference supervized_partition/graph_processing.py:347-436,
# :534-546, partition/ply_c/random_subgraph.cpp)
# --------------------------------------------------------------------------------------------------
TILES_MAX_K = 64
TILES_VERTICES_PER_BLOCK = 32      # selected vertices one workgroup of the tile kernel takes
_GLOBAL_FEAT_KEYS = ('e', 'rgb', 'XY', 'xy')


def _scene_array(t, shape, name):
    _on_gpu(t, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must be {list(shape)}, got {list(t.shape)}')
    return _req(t.contiguous(), torch.float32, name)


def neighbourhood_tiles(xyz, nei, k: int, rows=None, rgb=None, global_feat='', elevation=None, xyn=None, cloud_rgb=True,
                        stream_stores=True):
    """The tiles of graph_loader (graph_processing.py:389-411) -> (clouds f32 [m, 3 or 6, k], clouds_global f32 [m, G], diameters
    f32 [m]), bit for bit what numpy computes in float32: xyz f32 [N, 3]; nei int32 / int64 [N, K >= k], indices into the full
    cloud, 1 <= k <= 64; rows: ascending ids of the selected vertices (int64 [m]; None = all); rgb f32 [N, 3] (already / 255) adds the
    neighbours' colours as channels 3..5 unless cloud_rgb is False (the reference's use_rgb = 0, which still needs rgb for the
    'rgb' global feature).  clouds_global = diameters, then per key that is a substring of global_feat, in this order: 'e'
    elevation f32 [N], 'rgb' the vertex's own rgb, 'XY' xyn f32 [N, 2], 'xy' xyz[rows, :2].  stream_stores: non-temporal stores
    of clouds (the faster form wherever the two differed: profiles/tiles_bench.txt).  An index outside [0, N) in nei or rows raises IndexError (one host synchronisation)."""
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError('xyz must be a [N, 3] tensor')
    N, k = int(xyz.shape[0]), int(k)
    xyz = _scene_array(xyz, (N, 3), 'xyz')
    _on_gpu(nei, 'nei')
    if nei.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'nei must be int32 or int64, got {nei.dtype}')
    if nei.dim() != 2 or nei.shape[0] != N:
        raise ValueError(f'nei must be [{N}, K], got {list(nei.shape)}')
    K = int(nei.shape[1])
    if not (1 <= k <= TILES_MAX_K and k <= K):
        raise ValueError(f'1 <= k <= {TILES_MAX_K} and k <= K = {K} expected, got k = {k}')
    if not 1 <= N < 2 ** 31 - 1:
        raise ValueError(f'1 <= N < 2^31 - 1 expected, got N = {N}')
    nei = _req(nei.contiguous(), None, 'nei')
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dim() != 1:
            raise ValueError('rows must be a [m] tensor')
        rows = _req(rows.to(torch.int64).contiguous(), torch.int64, 'rows')
        m = int(rows.numel())
    else:
        m = N
    want = {key: key in global_feat for key in _GLOBAL_FEAT_KEYS}
    if rgb is not None:
        rgb = _scene_array(rgb, (N, 3), 'rgb')
    elif want['rgb']:
        raise ValueError("global_feat has 'rgb' but rgb is None")
    if want['e']:
        if elevation is None:
            raise ValueError("global_feat has 'e' but elevation is None")
        elevation = _scene_array(elevation.reshape(-1) if torch.is_tensor(elevation) else elevation, (N,), 'elevation')
    if want['XY']:
        if xyn is None:
            raise ValueError("global_feat has 'XY' but xyn is None")
        xyn = _scene_array(xyn, (N, 2), 'xyn')
    cloud_rgb = bool(cloud_rgb) and rgb is not None
    F = 6 if cloud_rgb else 3
    G = 1 + (1 if want['e'] else 0) + (3 if want['rgb'] else 0) + (2 if want['XY'] else 0) + (2 if want['xy'] else 0)
    dev = xyz.device
    clouds = torch.empty(m, F, k, dtype=torch.float32, device=dev)
    clouds_global = torch.empty(m, G, dtype=torch.float32, device=dev)
    diameters = torch.empty(m, dtype=torch.float32, device=dev)
    if m == 0:
        return clouds, clouds_global, diameters
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().spg_neighbourhood_tiles(_ptr(xyz), _ptr(rgb), N, _ptr(nei), 1 if nei.dtype == torch.int64 else 0, K, k, _ptr(rows), m,
                                        1 if cloud_rgb else 0, _ptr(elevation) if want['e'] else None, _ptr(xyn) if want['XY'] else None,
                                        1 if want['rgb'] else 0, 1 if want['xy'] else 0, 1 if stream_stores else 0, _ptr(clouds),
                                        _ptr(clouds_global), _ptr(diameters), _ptr(err), _stream()), 'spg_neighbourhood_tiles')
    if int(err.item()) & 1:
        raise IndexError(f'neighbourhood_tiles: an index in nei or rows is outside [0, {N})')
    return clouds, clouds_global, diameters


def _host_f32(a, shape, name):
    import numpy as np
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
    if a.shape != shape:
        raise ValueError(f'{name} must be {list(shape)}, got {list(a.shape)}')
    return a


def augment_whole(xyz, rgb, ref_point=None, M=None, noise_xyz=None, noise_rgb=None):
    """augment_cloud_whole (graph_processing.py:534-546) with the random quantities as inputs (drawn and clipped by the caller, so
    the reference's random stream stays usable) -> (xyz, rgb): xyz = ((xyz - ref_point) @ M + ref_point) + noise_xyz, every
    product and sum rounded on its own in float32; rgb = clip(rgb + noise_rgb, -1, 1).  ref_point [3] and M [3, 3] are host values
    (both or neither; the caller sets ref_point[2] = 0 as the reference does); noise_* f32 [N, 3] device tensors.  Every argument
    that is None leaves its part out: with all of them None the inputs are returned as they are.  rgb may be None."""
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError('xyz must be a [N, 3] tensor')
    N = int(xyz.shape[0])
    xyz = _scene_array(xyz, (N, 3), 'xyz')
    if (M is None) != (ref_point is None):
        raise ValueError('augment_whole: ref_point and M come together')
    if rgb is not None:
        rgb = _scene_array(rgb, (N, 3), 'rgb')
    elif noise_rgb is not None:
        raise ValueError('augment_whole: noise_rgb needs rgb')
    if M is None and noise_xyz is None and noise_rgb is None:
        return xyz, rgb
    Mh = rh = None
    if M is not None:
        Mh, rh = _host_f32(M, (3, 3), 'M'), _host_f32(ref_point, (3,), 'ref_point')
    if noise_xyz is not None:
        noise_xyz = _scene_array(noise_xyz, (N, 3), 'noise_xyz')
    if noise_rgb is not None:
        noise_rgb = _scene_array(noise_rgb, (N, 3), 'noise_rgb')
    xyz_out = torch.empty_like(xyz)
    rgb_out = torch.empty_like(rgb) if noise_rgb is not None else None
    check(lib().spg_augment_whole(_ptr(xyz), _ptr(rgb), N, Mh.ctypes.data if Mh is not None else None,
                                  rh.ctypes.data if rh is not None else None, _ptr(noise_xyz), _ptr(noise_rgb), _ptr(xyz_out),
                                  _ptr(rgb_out), _stream()), 'spg_augment_whole')
    return xyz_out, (rgb_out if rgb_out is not None else rgb)


def random_subgraph(graph: EdgeGraph, subgraph_size: int, seeds, state=None):
    """libply_c.random_subgraph (partition/ply_c/random_subgraph.cpp) with the seed vertices as an explicit int64 sequence, consumed
    in order, in place of the reference's unseeded rand() -> (selected_edg u8 [E], selected_ver u8 [n], n_seen, n_seeds_used,
    state).  Its queue discipline is reproduced: an already selected seed is skipped but consumed; neighbours are visited in
    adjacency order (ascending edge id, as Boost inserts them); once n_seen reaches subgraph_size every vertex still in the queue
    examines its first adjacency slot only and the first unselected one of those is accepted, so n_seen is usually
    subgraph_size + 1.  subgraph_size > n raises ValueError (the reference writes out of bounds there).  When the seeds run out
    first, n_seen < subgraph_size; a further call with more seeds and the returned state continues.  A seed outside [0, n) raises
    IndexError.  One host synchronisation."""
    graph._use()
    n, E, dev = graph.n, graph.E, graph.device
    subgraph_size = int(subgraph_size)
    if subgraph_size > n:
        raise ValueError(f'random_subgraph: subgraph_size = {subgraph_size} exceeds the {n} vertices of the graph')
    if subgraph_size < 0:
        raise ValueError(f'random_subgraph: subgraph_size >= 0 expected, got {subgraph_size}')
    if not torch.is_tensor(seeds):
        seeds = torch.as_tensor(seeds, dtype=torch.int64)
    if seeds.dim() != 1 or seeds.dtype.is_floating_point:
        raise ValueError('random_subgraph: seeds must be an integer [n_seeds] sequence')
    seeds = _req(seeds.to(device=dev, dtype=torch.int64).contiguous(), torch.int64, 'seeds')
    if state is None:
        selected_ver = torch.zeros(n, dtype=torch.uint8, device=dev)
        n_seen = 0
    else:
        selected_ver, n_seen = state
        selected_ver = _req(selected_ver, torch.uint8, 'state')
        if selected_ver.shape != (n,):
            raise ValueError(f'random_subgraph: state belongs to a graph of {selected_ver.numel()} vertices, this one has {n}')
        selected_ver = selected_ver.clone()
    L = lib()
    st = torch.tensor([int(n_seen), 0, 0], dtype=torch.int64).to(dev)
    selected_edg = torch.empty(E, dtype=torch.uint8, device=dev)
    ws = _u8_workspace(L.spg_random_subgraph_workspace_bytes(n), dev)
    check(L.spg_random_subgraph(_ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends), E, n, subgraph_size, _ptr(seeds), int(seeds.numel()),
                                _ptr(selected_ver), _ptr(selected_edg), _ptr(st), _ptr(ws), ws.numel(), _stream()), 'spg_random_subgraph')
    n_seen, used, err = (int(v) for v in st.tolist())
    if err & 1:
        raise IndexError(f'random_subgraph: seed {used} is outside [0, {n})')
    return selected_edg, selected_ver, n_seen, used, (selected_ver, n_seen)


def induced_subgraph(graph: EdgeGraph, selected_ver, selected_edg):
    """graph_processing.py:375-379 on the device -> (rows i64 [m] the selected vertices ascending, new_ver_index i64 [n] with -1
    where unselected, kept i64 [E'] the selected edge ids in order, edg_source i64 [E'], edg_target i64 [E'] =
    new_ver_index[end points of the kept edges]).  Scans on the device; one host read (the two counts)."""
    graph._use()
    n, E, dev = graph.n, graph.E, graph.device
    sv = _indicator(selected_ver, n, 'selected_ver')
    se = _indicator(selected_edg, E, 'selected_edg')
    L, i64 = lib(), torch.int64
    rows = torch.empty(n, dtype=i64, device=dev)
    new_ver_index = torch.empty(n, dtype=i64, device=dev)
    kept, src, tgt = (torch.empty(E, dtype=i64, device=dev) for _ in range(3))
    counts = torch.empty(2, dtype=i64, device=dev)
    ws = _u8_workspace(L.spg_induced_subgraph_workspace_bytes(n, E), dev)
    check(L.spg_induced_subgraph(_ptr(graph.ends), E, n, _ptr(sv), _ptr(se), _ptr(rows), _ptr(new_ver_index), _ptr(kept), _ptr(src), _ptr(tgt),
                                 _ptr(counts), _ptr(ws), ws.numel(), _stream()), 'spg_induced_subgraph')
    m, Ek = (int(v) for v in counts.tolist())
    return rows[:m], new_ver_index, kept[:Ek], src[:Ek], tgt[:Ek]


# --------------------------------------------------------------------------------------------------
# neighbourhood sub-sampling of the supervised loader (csrc/spg_sample.hip; reference learning/spg.py:115-144)
# --------------------------------------------------------------------------------------------------
def _resident(a, dtype, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    t = t.to(dtype).contiguous()
    return t if t.is_cuda else upload(t, dev)


class ResidentSPG:
    """A scene's superpoint graph in device memory: edges i64 [E, 2] in file order with their EdgeGraph, the edge features f32
    [E, F] (or None) and the vertices' point counts i64 [n] (or None; needed for a cut).  Host arrays are uploaded here.  The
    EdgeGraph's range check synchronises once, after every upload: the object is complete on every stream when this returns."""

    def __init__(self, edges, feats, sizes, n: int):
        dev = torch.device('cuda', torch.cuda.current_device())
        self.n = int(n)
        self.edges = _resident(edges, torch.int64, dev).reshape(-1, 2)
        self.E = int(self.edges.shape[0])
        self.feats = None if feats is None else _resident(feats, torch.float32, dev).reshape(self.E, -1)
        self.sizes = None if sizes is None else _resident(sizes, torch.int64, dev).reshape(-1)
        if self.sizes is not None and self.sizes.numel() != self.n:
            raise ValueError(f'ResidentSPG: {self.sizes.numel()} sizes for {self.n} vertices')
        self.graph = EdgeGraph(self.edges[:, 0].contiguous(), self.edges[:, 1].contiguous(), self.n)
        self.device = self.graph.device


class SPGSample:
    """What sample_spg returns: host `vids` i64 [n] (original ids of the kept vertices; their position is their new id) and `degs`
    i64 [n] (in-degrees), the counts `n`, `E`, and on the device `edges` i64 [E, 2] (relabelled), `feats` f32 [E, F] or None, `kept`
    i64 [E] (ids of the kept edges)."""
    __slots__ = ('vids', 'degs', 'n', 'E', 'edges', 'feats', 'kept')


_sample_side = {}      # device index -> (the sampler's stream, its page-locked read-back buffer)


def _sampler(dev, n_words):
    ent = _sample_side.get(dev.index)
    if ent is None or ent[1].numel() < n_words:
        stream = ent[0] if ent is not None else torch.cuda.Stream(device=dev)
        ent = _sample_side[dev.index] = (stream, torch.empty(max(n_words, 4096), dtype=torch.int64).pin_memory())
    return ent


def _index_vector(a, name):
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.int64))
    if t.dim() != 1 or t.dtype.is_floating_point:
        raise ValueError(f'sample_spg: {name} must be an integer vector')
    return t.to(torch.int64).contiguous()


def sample_spg(g: ResidentSPG, perm=None, centres=None, order: int = 0, minpts: int = 0, hardcutoff: int = 0) -> SPGSample:
    """The loader's sub-sampling (permute_vertices -> random_neighborhoods -> k_big_enough) cut out of a resident graph: perm
    (vertex k becomes position perm[k]) or None, centres (ids in the permuted numbering) or None = every vertex is a member,
    else the members are the vertices within `order` steps of a centre, direction ignored; along the permuted positions a member is
    kept while the count of members of >= minpts points is <= hardcutoff (hardcutoff <= 0: all members).  Index-exact with the host
    path; include/spg_hip.h: spg_sample_spg.  perm / centres: host sequences (staged here) or device tensors.
    The launches and the read-back run on the sampler's own stream and ONLY that stream is synchronised (once): the call does not
    wait for work in flight on the current stream.  After it returns the outputs may be used on any stream.
    A centre outside [0, n) raises IndexError, a perm that is no permutation of 0 ... n - 1 ValueError."""
    g.graph._use()
    n, E, dev = g.n, g.E, g.device
    hardcutoff, minpts, order = int(hardcutoff), int(minpts), int(order)
    if order < 0:
        raise ValueError(f'sample_spg: order >= 0 expected, got {order}')
    if hardcutoff > 0 and g.sizes is None:
        raise ValueError('sample_spg: a cut (hardcutoff > 0) needs the sizes of the resident graph')
    perm, centres = _index_vector(perm, 'perm'), _index_vector(centres, 'centres')
    if perm is not None and perm.numel() != n:
        raise ValueError(f'sample_spg: perm has {perm.numel()} entries, the graph {n} vertices')
    L, i64 = lib(), torch.int64
    F = 0 if g.feats is None else int(g.feats.shape[1])
    stream, pinned = _sampler(dev, 3 + 2 * n)
    with torch.cuda.stream(stream):
        staged = upload_packed([t if (t is not None and not t.is_cuda) else None for t in (perm, centres)], dev)
        perm_d, centres_d = (s if s is not None else t for s, t in zip(staged, (perm, centres)))
        back = torch.empty(3 + 2 * n, dtype=i64, device=dev)          # head, vids, degs: one read-back
        head, vids, degs = back[:3], back[3:3 + n], back[3 + n:]
        edges = torch.empty(E, 2, dtype=i64, device=dev)
        kept = torch.empty(E, dtype=i64, device=dev)
        feats = torch.empty(E, F, dtype=torch.float32, device=dev) if g.feats is not None else None
        ws = _u8_workspace(L.spg_sample_spg_workspace_bytes(n, E), dev)
        check(L.spg_sample_spg(_ptr(g.graph.ends), E, n, _ptr(perm_d), _ptr(centres_d), 0 if centres_d is None else int(centres_d.numel()),
                               _ptr(g.sizes), _ptr(g.feats), F, order, minpts, hardcutoff, _ptr(vids), _ptr(edges), _ptr(kept), _ptr(feats),
                               _ptr(degs), _ptr(head), _ptr(ws), ws.numel(), stream.cuda_stream), 'spg_sample_spg')
        host = pinned[:3 + 2 * n]
        host.copy_(back, non_blocking=True)
    stream.synchronize()
    m, Ek, err = (int(v) for v in host[:3].tolist())
    if err & 1:
        raise IndexError(f'sample_spg: a centre is outside [0, {n})')
    if err & 2:
        raise ValueError(f'sample_spg: perm is not a permutation of 0 ... {n - 1}')
    out = SPGSample()
    out.n, out.E = m, Ek
    out.vids, out.degs = host[3:3 + m].clone(), host[3 + n:3 + n + m].clone()
    out.edges, out.kept, out.feats = edges[:Ek], kept[:Ek], (feats[:Ek] if feats is not None else None)
    # allocated on the sampler's stream, consumed on the caller's: the allocator must not hand the blocks out again before that use
    cur = torch.cuda.current_stream(dev)
    for t in (edges, kept, feats):
        if t is not None:
            t.record_stream(cur)
    return out


# --------------------------------------------------------------------------------------------------
# the scene structure of the learned partition (csrc/spg_structure.hip; reference supervized_partition/graph_processing.py:120-190)
# --------------------------------------------------------------------------------------------------
_ID_MODES = {'objects': 1, 'labels': 2, 'given': 3}


def _scene_xyz(xyz, who):
    """xyz as every scene op takes it: float32 [n, 3] on the device, n >= 1 -> n"""
    _req(xyz, torch.float32, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f'{who}: xyz must be [n, 3] with n >= 1, got {tuple(xyz.shape)}')
    return int(xyz.shape[0])


def _raise_nonfinite(word):
    """bit 0 of an error word of the scene ops: sklearn's message for a coordinate that is NaN or infinite"""
    if word & 1:
        raise ValueError('Input contains NaN or infinity.')


def scene_structure(xyz, knn_idx, k_adj: int, ids=None, hist=None, id_mode='objects', geof=None, rgb=None):
    """What graph_processing.py:main() computes per file between prune, the kNN search and compute_geof (:126, :144-190), on
    device tensors: xyz f32 [n, 3]; knn_idx i32 [n, k_local] as ops.knn returns it (the point itself dropped); the first k_adj
    columns are the adjacency.  The vertex ids that decide is_transition come from
      id_mode 'objects': hist i32 [n, C] (pruned s3dis objects)  -> hist[:, 1:].argmax(1) + 1,
      id_mode 'labels':  hist i32 [n, C] (pruned vkitti labels)   -> hist.argmax(1); the objects are then the components over
                         the edges that are no transition (ops.connected_components: numbered by smallest member),
      id_mode 'given':   ids integer [n].
    geof f32 [n, 4] (ops.compute_geof) gets its column 3 doubled IN PLACE (:177); rgb u8 [n, 3] is returned as f32 / 255 (:353).
    -> dict of device tensors: edg_source, edg_target i64 [n * k_adj], nei (knn_idx itself: adopted, not copied), is_transition
    u8, hard_ids i64 [n], objects i64 [n], elevation f32 [n] (z - min z), xyn f32 [n, 2], geof, rgb (None when not given), and
    graph, the EdgeGraph of the adjacency.  Host reads: the error word after the frame pass (ValueError on NaN / infinity before
    anything else is launched) and after the edges, the EdgeGraph's, and the component count with id_mode 'labels'."""
    n, k_adj = _scene_xyz(xyz, 'scene_structure'), int(k_adj)
    _req(knn_idx, torch.int32, 'knn_idx')
    if knn_idx.dim() != 2 or knn_idx.shape[0] != n:
        raise ValueError(f'scene_structure: knn_idx must be [{n}, k_local], got {tuple(knn_idx.shape)}')
    k_local = int(knn_idx.shape[1])
    if not 1 <= k_adj <= k_local:
        raise ValueError(f'scene_structure: 1 <= k_adj <= k_local = {k_local} expected, got {k_adj}')
    if id_mode not in _ID_MODES:
        raise ValueError(f"scene_structure: id_mode must be 'objects', 'labels' or 'given', got {id_mode!r}")
    mode, ids_is_i64 = _ID_MODES[id_mode], 0
    if id_mode == 'given':
        if ids is None or hist is not None:
            raise ValueError("scene_structure: id_mode 'given' takes ids (and no hist)")
        if not torch.is_tensor(ids) or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.shape != (n,):
            raise ValueError(f'scene_structure: ids must be an integer tensor [{n}]')
        if ids.dtype not in (torch.int32, torch.int64):
            ids = ids.to(torch.int64)
        _req(ids, None, 'ids')
        ids_is_i64 = int(ids.dtype == torch.int64)
    else:
        if hist is None or ids is not None:
            raise ValueError(f'scene_structure: id_mode {id_mode!r} takes hist (and no ids)')
        _req(hist, torch.int32, 'hist')
        min_cols = 2 if id_mode == 'objects' else 1                  # 'objects' takes its arg-max from column 1 on
        if hist.dim() != 2 or hist.shape[0] != n or hist.shape[1] < min_cols:
            raise ValueError(f'scene_structure: hist must be [{n}, C] with C >= {min_cols}, got {tuple(hist.shape)}')
    if geof is not None:
        _req(geof, torch.float32, 'geof')
        if geof.shape != (n, 4):
            raise ValueError(f'scene_structure: geof must be [{n}, 4], got {tuple(geof.shape)}')
    if rgb is not None:
        _req(rgb, torch.uint8, 'rgb')
        if rgb.shape != (n, 3):
            raise ValueError(f'scene_structure: rgb must be [{n}, 3], got {tuple(rgb.shape)}')
    L, dev, st = lib(), xyz.device, _stream()
    f32, i64, u8 = torch.float32, torch.int64, torch.uint8
    frame = torch.empty(5, dtype=f32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _u8_workspace(L.spg_structure_frame_workspace_bytes(n), dev)
    check(L.spg_structure_frame(_ptr(xyz), n, _ptr(frame), _ptr(err), _ptr(ws), ws.numel(), st), 'spg_structure_frame')
    _raise_nonfinite(int(err.item()))
    E = n * k_adj
    out = {'elevation': torch.empty(n, dtype=f32, device=dev), 'xyn': torch.empty(n, 2, dtype=f32, device=dev),
           'hard_ids': torch.empty(n, dtype=i64, device=dev), 'geof': geof, 'nei': knn_idx,
           'rgb': torch.empty(n, 3, dtype=f32, device=dev) if rgb is not None else None}
    check(L.spg_structure_vertices(_ptr(xyz), n, _ptr(frame), _ptr(rgb), _ptr(hist), int(hist.shape[1]) if hist is not None else 0, mode,
                                   _ptr(ids), ids_is_i64, _ptr(out['elevation']), _ptr(out['xyn']), _ptr(out['rgb']), _ptr(geof),
                                   _ptr(out['hard_ids']), st), 'spg_structure_vertices')
    out['edg_source'], out['edg_target'] = torch.empty(E, dtype=i64, device=dev), torch.empty(E, dtype=i64, device=dev)
    out['is_transition'], active = torch.empty(E, dtype=u8, device=dev), torch.empty(E, dtype=u8, device=dev)
    check(L.spg_structure_edges(_ptr(knn_idx), n, k_local, k_adj, _ptr(out['hard_ids']), _ptr(out['edg_source']), _ptr(out['edg_target']),
                                _ptr(out['is_transition']), _ptr(active), _ptr(err), st), 'spg_structure_edges')
    if int(err.item()) & 2:
        raise IndexError(f'scene_structure: a neighbour index is outside [0, {n})')
    out['graph'] = EdgeGraph(out['edg_source'], out['edg_target'], n)
    if id_mode == 'labels':
        comp, _, _ = connected_components(out['graph'], active)
        out['objects'] = comp.to(i64)
    else:
        out['objects'] = out['hard_ids']
    return out


# --------------------------------------------------------------------------------------------------
# the ground-plane elevation (csrc/spg_plane.hip; reference supervized_partition/graph_processing.py:181-186, learning/s3dis_dataset.py:130-133)
# --------------------------------------------------------------------------------------------------
PLANE_MAX_TRIALS = 1024


def ransac_subsets(n_low: int, trials: int = 100, seed: int = 0):
    """The first `trials` triples that sklearn's RANSACRegressor(random_state=seed) draws from n_low samples: the stream of
    sample_without_replacement(n_low, 3, random_state=np.random.RandomState(seed)) -> int64 [trials, 3] (host).  n_low >= 300
    (3 / n_low <= 0.01): tracking selection, randint(n_low) until three distinct values; 4 <= n_low <= 299: permutation(n_low)[:3];
    n_low == 3: (0, 1, 2) without a draw.  sklearn draws lazily, one triple per trial: this is a prefix of the same stream."""
    n_low, trials = int(n_low), int(trials)
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    rs = np.random.RandomState(seed)
    out = np.empty((trials, 3), np.int64)
    for t in range(trials):
        if n_low == 3:
            out[t] = (0, 1, 2)
        elif n_low < 300:
            out[t] = rs.permutation(n_low)[:3]
        else:
            sel = []
            while len(sel) < 3:
                j = int(rs.randint(n_low))
                if j not in sel:
                    sel.append(j)
            out[t] = sel
    return out


def plane_elevation(xyz, subsets=None, seed: int = 0, max_trials: int = 100, low_height: float = 0.5):
    """The elevation of graph_processing.py:181-186 with plane_model: z minus the plane that sklearn 1.7's
    RANSACRegressor(random_state=seed) fits to the points less than low_height above the lowest one, restated on the device
    (csrc/spg_plane.hip): xyz f32 [n, 3] on the device -> dict: elevation f32 [n], coef f64 [2],
    intercept f64 (0-d), threshold f32 (0-d: median |y - median y| in float32, numpy's bits), low_index i32 [n_low], inlier_mask u8
    [n_low] (device tensors) and the host ints n_low, n_trials (what sklearn's n_trials_ counts), best_trial.
    subsets: integer [T, 3], indices into the low points, one triple per trial (T <= 1024 replaces max_trials); None draws
    ransac_subsets(n_low, max_trials, seed) on the host.  Every trial is evaluated; sklearn's acceptance loop is replayed on the
    device.  Host reads: n_low with the error word (ValueError on NaN / infinity before anything else), and the error word with
    n_trials / best_trial at the end (ValueError when no trial found a consensus set, IndexError for a subset index)."""
    n = _scene_xyz(xyz, 'plane_elevation')
    L, dev, st = lib(), xyz.device, _stream()
    low_index = torch.empty(n, dtype=torch.int32, device=dev)
    head = torch.empty(2, dtype=torch.int32, device=dev)                   # n_low, error word: one read
    ws = _u8_workspace(L.spg_plane_workspace_bytes(n, -1, 0), dev)
    check(L.spg_plane_low(_ptr(xyz), n, float(low_height), _ptr(low_index), _ptr(head), _ptr(head[1:]), _ptr(ws), ws.numel(), st), 'spg_plane_low')
    n_low, err = (int(v) for v in head.tolist())
    _raise_nonfinite(err)
    if n_low < 3:
        raise ValueError(f'`min_samples` may not be larger than number of samples: n_samples = {n_low}.')
    if subsets is None:
        if not 1 <= int(max_trials) <= PLANE_MAX_TRIALS:
            raise ValueError(f'plane_elevation: 1 <= max_trials <= {PLANE_MAX_TRIALS} expected, got {max_trials}')
        subsets = ransac_subsets(n_low, int(max_trials), seed)
    if not torch.is_tensor(subsets):
        subsets = torch.from_numpy(np.ascontiguousarray(np.asarray(subsets)))
    if subsets.dtype.is_floating_point or subsets.dim() != 2 or subsets.shape[1] != 3 or not 1 <= subsets.shape[0] <= PLANE_MAX_TRIALS:
        raise ValueError(f'plane_elevation: subsets must be an integer array [T, 3] with 1 <= T <= {PLANE_MAX_TRIALS}')
    subsets = subsets.to(device=dev, dtype=torch.int32).contiguous()
    T = int(subsets.shape[0])
    out = {'elevation': torch.empty(n, dtype=torch.float32, device=dev), 'coef': torch.empty(2, dtype=torch.float64, device=dev),
           'intercept': torch.empty((), dtype=torch.float64, device=dev), 'threshold': torch.empty((), dtype=torch.float32, device=dev),
           'low_index': low_index[:n_low], 'inlier_mask': torch.empty(n_low, dtype=torch.uint8, device=dev)}
    tail = torch.zeros(3, dtype=torch.int32, device=dev)                   # n_trials, best_trial, error word
    ws = _u8_workspace(L.spg_plane_workspace_bytes(n, n_low, T), dev)
    check(L.spg_plane_fit(_ptr(xyz), n, _ptr(low_index), n_low, _ptr(subsets), T, _ptr(out['elevation']), _ptr(out['coef']), _ptr(out['intercept']),
                          _ptr(out['threshold']), _ptr(out['inlier_mask']), _ptr(tail), _ptr(tail[2:]), _ptr(ws), ws.numel(), st), 'spg_plane_fit')
    n_trials, best, err = (int(v) for v in tail.tolist())
    if err & 4:
        raise IndexError(f'plane_elevation: a subset index is outside [0, {n_low})')
    if err & 2:
        raise ValueError('RANSAC could not find a valid consensus set. All `max_trials` iterations were skipped because each randomly chosen '
                         'sub-sample failed the passing criteria.')
    out.update(n_low=n_low, n_trials=n_trials, best_trial=best)
    return out


# --------------------------------------------------------------------------------------------------
# parsed superpoint clouds (csrc/spg_parsed.hip; reference learning/{s3dis,sema3d,vkitti,custom}_dataset.py: preprocess_pointclouds)
# --------------------------------------------------------------------------------------------------
PARSED_RECIPES = {'s3dis': (0, 15), 'sema3d': (1, 11), 'custom': (1, 11), 'vkitti': (2, 14)}      # name -> (SPG_PARSED_*, columns)
CLASS_COUNT_MAX = 4096


def scene_stats(xyz, with_distance: bool = False):
    """The statistics preprocess_pointclouds takes of a scene, by fixed-order reductions (the same input gives the same bits):
    xyz f32 [n, 3] on the device -> (stats_f32 [6] = min x, y, z, max x, y, z; stats_f64 [5] = mean x, y, z and, with_distance,
    the mean and population standard deviation of the distance to the room centre in float64; centroid f32 [3]), device tensors.
    One host read: the error word (ValueError on NaN / infinity)."""
    n = _scene_xyz(xyz, 'scene_stats')
    L, dev = lib(), xyz.device
    s32, s64 = torch.empty(6, dtype=torch.float32, device=dev), torch.empty(5, dtype=torch.float64, device=dev)
    centroid, err = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = _u8_workspace(L.spg_parsed_workspace_bytes(n), dev)
    check(L.spg_parsed_stats(_ptr(xyz), n, int(bool(with_distance)), _ptr(s32), _ptr(s64), _ptr(centroid), _ptr(err), _ptr(ws), ws.numel(),
                             _stream()), 'spg_parsed_stats')
    _raise_nonfinite(int(err.item()))
    return s32, s64, centroid


def parsed_points(recipe, xyz, rgb, comp_off, comp_idx, geof=None, elevation=None, trim=None, lpsv_raw: bool = False):
    """The datasets preprocess_pointclouds writes for one scene, as one device buffer (csrc/spg_parsed.hip, DESIGN.md section
    4.11h).  recipe 's3dis' (15 columns: xyz, rgb, e, lpsv[4], xyzn[3], dist), 'sema3d' / 'custom' (11: xyz, rgb, z / 100,
    geof - 0.5) or 'vkitti' (14: xyz, rgb, e, four zeros, xyzn).  xyz f32 [n, 3]; rgb u8 | f32 [n, 3]; geof f32 [n, 4] (not for
    vkitti); s3dis: elevation f32 [n] or None (z / 4 - 0.5), lpsv_raw: geof unchanged (supervized_partition).  Component c owns
    comp_idx[comp_off[c] : comp_off[c + 1]] (comp_off i64 [C + 1], host or device; comp_idx i32 | i64 [M] on the device; a vertex
    may appear in no component or in several).  trim: {component: positions inside it (integer sequence)} -- the component's rows
    are then comp_idx[comp_off[c] + positions], in that order.
    -> points f32 [Ntot, ncols] with the rows of component 0, 1, ... back to back, centroid f32 [3] (device), offsets i64 [C + 1]
    (host numpy).  Host traffic: comp_off down when it lives on the device, the offset and trim tables up, two reads of the error
    word (ValueError for NaN / infinity, IndexError for a component index or a trim position out of range)."""
    if recipe not in PARSED_RECIPES:
        raise ValueError(f'parsed_points: recipe must be one of {sorted(PARSED_RECIPES)}, got {recipe!r}')
    code, ncols = PARSED_RECIPES[recipe]
    n, dev = _scene_xyz(xyz, 'parsed_points'), xyz.device
    _req(rgb, None, 'rgb')
    if rgb.dtype not in (torch.uint8, torch.float32) or rgb.shape != (n, 3):
        raise ValueError(f'parsed_points: rgb must be uint8 or float32 [{n}, 3]')
    if code != 2:
        if geof is None:
            raise ValueError(f'parsed_points: recipe {recipe!r} needs geof')
        _req(geof, torch.float32, 'geof')
        if geof.shape != (n, 4):
            raise ValueError(f'parsed_points: geof must be [{n}, 4], got {tuple(geof.shape)}')
    else:
        geof = None
    if elevation is not None:
        if code != 0:
            raise ValueError("parsed_points: only recipe 's3dis' takes an elevation")
        _req(elevation, torch.float32, 'elevation')
        if elevation.shape != (n,):
            raise ValueError(f'parsed_points: elevation must be [{n}], got {tuple(elevation.shape)}')
    _req(comp_idx, None, 'comp_idx')
    if comp_idx.dtype not in (torch.int32, torch.int64) or comp_idx.dim() != 1:
        raise ValueError('parsed_points: comp_idx must be int32 or int64 [M]')
    M = int(comp_idx.numel())
    src_h = (comp_off.cpu().numpy() if torch.is_tensor(comp_off) else np.asarray(comp_off)).astype(np.int64).reshape(-1)
    C = len(src_h) - 1
    if C < 1 or src_h[0] != 0 or src_h[-1] > M or (np.diff(src_h) < 0).any():
        raise ValueError(f'parsed_points: comp_off must be [C + 1] with C >= 1, ascending from 0 to at most {M}')
    sizes = np.diff(src_h)
    out_sizes, trim_off_h, trim_parts, n_trim = sizes.copy(), None, [], 0
    if trim:
        trim_off_h = np.full(C, -1, np.int64)
        for c in sorted(trim):
            pos = np.asarray(trim[c])
            if not 0 <= int(c) < C or pos.ndim != 1 or pos.dtype.kind not in 'iu':
                raise ValueError(f'parsed_points: trim maps a component in [0, {C}) to a 1-d integer array')
            if pos.size and (pos.max() >= 2 ** 31 or pos.min() < -2 ** 31):
                raise IndexError(f'parsed_points: a trim position of component {c} is outside [0, {int(sizes[c])})')
            trim_off_h[c], out_sizes[c] = n_trim, pos.size
            trim_parts.append(pos.astype(np.int32))
            n_trim += pos.size
    off_h = np.zeros(C + 1, np.int64)
    np.cumsum(out_sizes, out=off_h[1:])
    n_rows = int(off_h[-1])
    if n_rows >= 2 ** 31 - 1:
        raise ValueError('parsed_points: fewer than 2^31 - 1 rows expected')
    L, st = lib(), _stream()
    s32, s64, centroid = scene_stats(xyz, code == 0)        # (sema3d reads no statistic: the centroid and the finite check)
    out_off_d, src_off_d = torch.from_numpy(off_h).to(dev), torch.from_numpy(src_h).to(dev)
    trim_off_d = trim_d = None
    if trim_off_h is not None:          # (one spare entry: the table is never empty)
        trim_off_d, trim_d = torch.from_numpy(trim_off_h).to(dev), torch.from_numpy(np.concatenate(trim_parts + [np.zeros(1, np.int32)])).to(dev)
    points = torch.empty(n_rows, ncols, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.spg_parsed_rows(code, _ptr(xyz), n, _ptr(rgb), int(rgb.dtype == torch.float32), _ptr(geof), _ptr(elevation), int(bool(lpsv_raw)),
                            _ptr(s32), _ptr(s64), _ptr(out_off_d), _ptr(src_off_d), C, _ptr(comp_idx), int(comp_idx.dtype == torch.int64),
                            _ptr(trim_d), _ptr(trim_off_d), n_rows, _ptr(points), _ptr(err), st), 'spg_parsed_rows')
    flag = int(err.item())
    if flag & 2:
        raise IndexError(f'parsed_points: a component index is outside [0, {n})')
    if flag & 4:
        raise IndexError('parsed_points: a trim position is outside its component')
    return points, centroid, off_h


def class_count(labels, n_classes: int):
    """np.bincount(np.argmax(labels[:, 1:], 1), minlength=n_classes) of the label histograms labels u32 | i32 [n, n_classes + 1] on
    the device (first maximum; an all-zero row counts for class 0) -> i64 [n_classes] on the device."""
    n_classes = int(n_classes)
    _req(labels, None, 'labels')
    if labels.dtype not in (torch.int32, torch.uint32):
        raise TypeError(f'class_count: labels must be uint32 or int32, got {labels.dtype}')
    if not 1 <= n_classes <= CLASS_COUNT_MAX:
        raise ValueError(f'class_count: 1 <= n_classes <= {CLASS_COUNT_MAX} expected, got {n_classes}')
    if labels.dim() != 2 or labels.shape[1] != n_classes + 1:
        raise ValueError(f'class_count: labels must be [n, {n_classes + 1}], got {tuple(labels.shape)}')
    count = torch.empty(n_classes, dtype=torch.int64, device=labels.device)
    check(lib().spg_class_count(_ptr(labels), int(labels.dtype == torch.int32), int(labels.shape[0]), n_classes, _ptr(count), _stream()),
          'spg_class_count')
    return count


# --------------------------------------------------------------------------------------------------
# raw cloud text (csrc/spg_text.hip; pandas.read_csv in the reference's partition/provider.py): DESIGN.md section 4.11i
# --------------------------------------------------------------------------------------------------
TEXT_MAX_COLS = 16
TEXT_ERRORS = {1: 'the wrong number of fields', 2: 'an empty field (a leading, trailing or double space)',
               3: 'a byte that is not part of a number', 4: 'a field outside the number grammar ([+-]digits[.digits], at most 15 '
               'digits, at most 22 behind the point, no exponent)', 5: 'a colour or label that is not a whole number in [0, 255]',
               6: 'a line longer than the cap'}


class CloudTextError(ValueError):
    """A line outside the contract of parse_cloud_text.  line: the index of the first refused line among the non-blank lines,
    offset: the byte the code points at (both counted from the start of the buffer, or of the file in CloudTextReader),
    code: a key of TEXT_ERRORS, refused: how many lines of the buffer were refused."""

    def __init__(self, line, code, offset, refused, source=''):
        self.line, self.code, self.offset, self.refused = int(line), int(code), int(offset), int(refused)
        super().__init__(f'cloud text{" " + source if source else ""}: line {self.line} (non-blank lines counted from 0), byte '
                         f'{self.offset}: {TEXT_ERRORS.get(self.code, "refused")} [code {self.code}]; {self.refused} line(s) refused')


def text_layout():
    """{'index_tile', 'max_line'} of csrc/spg_text.hip in bytes (spg_text_debug_layout; host only)."""
    L = lib()
    return {'index_tile': int(L.spg_text_debug_layout(0)), 'max_line': int(L.spg_text_debug_layout(1))}


def _text_roles(n_cols, xyz_cols, rgb_cols, label_col):
    n_cols = int(n_cols)
    if not 1 <= n_cols <= TEXT_MAX_COLS:
        raise ValueError(f'parse_cloud_text: 1 <= n_cols <= {TEXT_MAX_COLS} expected, got {n_cols}')
    roles = [-1] * n_cols
    picks = []
    for name, cols, first in (('xyz_cols', xyz_cols, 0), ('rgb_cols', rgb_cols, 3)):
        if cols is not None:
            cols = [int(c) for c in cols]
            if len(cols) != 3:
                raise ValueError(f'parse_cloud_text: {name} names three columns')
            picks += [(c, first + k) for k, c in enumerate(cols)]
    if label_col is not None:
        picks.append((int(label_col), 6))
    if not picks:
        raise ValueError('parse_cloud_text: no column selected')
    for c, r in picks:
        if not 0 <= c < n_cols or roles[c] != -1:
            raise ValueError(f'parse_cloud_text: column {c} is outside 0 ... {n_cols - 1} or selected twice')
        roles[c] = r
    return (ctypes.c_int * n_cols)(*roles)


def parse_cloud_text(text_u8, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, final_block=True, line_base=0, byte_base=0,
                     source=''):
    """The lines of a text cloud (`x y z i r g b` of Semantic3D, `x y z r g b` of S3DIS, one label per line) parsed on the device:
    text_u8 uint8 [n_bytes] on the GPU -> (xyz f32 [n, 3] | None, rgb u8 [n, 3] | None, label u8 [n] | None, n, consumed).
    n_cols fields per line, separated by exactly one space; a line ends at '\\n' (one '\\r' in front belongs to it), empty lines are
    skipped.  consumed: the bytes up to and including the last complete line; with final_block an unterminated last line counts
    and consumed = n_bytes, without it the caller carries text_u8[consumed:] in front of the next block.
    Values: the digits as an integer over a power of ten in float64, rounded once to float32 (= np.float32(float(token)), what
    pandas.read_csv returns on this grammar); zeros are +0.0; rgb / label are whole numbers in [0, 255].  Everything else raises
    CloudTextError (a ValueError) that names the first refused line, its byte and the reason (include/spg_hip.h).
    Two host synchronisations: the line count, which sizes the outputs, and the error record behind the parse.
    line_base / byte_base / source only shift and label what an error reports."""
    _req(text_u8, torch.uint8, 'text_u8')
    if text_u8.dim() != 1:
        raise ValueError('parse_cloud_text: text_u8 must be one-dimensional')
    roles = _text_roles(n_cols, xyz_cols, rgb_cols, label_col)
    if text_u8.data_ptr() % 16:
        text_u8 = text_u8.clone()                 # (a slice: the 16-byte loads want the allocator's alignment)
    L, dev, st = lib(), text_u8.device, _stream()
    nb = int(text_u8.numel())
    ws = _u8_workspace(L.spg_text_workspace_bytes(nb), dev)
    head = torch.empty(2, dtype=torch.int64, device=dev)
    check(L.spg_text_index(_ptr(text_u8), nb, int(bool(final_block)), _ptr(head), _ptr(ws), ws.numel(), st), 'spg_text_index')
    n, consumed = (int(v) for v in head.tolist())
    line_start = torch.empty(n, dtype=torch.int64, device=dev)
    check(L.spg_text_lines(_ptr(text_u8), nb, n, _ptr(line_start), _ptr(ws), ws.numel(), st), 'spg_text_lines')
    xyz = torch.empty(n, 3, dtype=torch.float32, device=dev) if xyz_cols is not None else None
    rgb = torch.empty(n, 3, dtype=torch.uint8, device=dev) if rgb_cols is not None else None
    label = torch.empty(n, dtype=torch.uint8, device=dev) if label_col is not None else None
    error = torch.empty(4, dtype=torch.int64, device=dev)
    check(L.spg_text_parse(_ptr(text_u8), nb, _ptr(line_start), n, int(n_cols), roles, _ptr(xyz), _ptr(rgb), _ptr(label), _ptr(error),
                           st), 'spg_text_parse')
    first, code, where, refused = error.tolist()
    if refused:
        raise CloudTextError(line_base + first, code, byte_base + where, refused, source)
    return xyz, rgb, label, n, consumed


class CloudTextReader:
    """Iterates over a text cloud file in device batches of exactly `rows` lines (fewer in the last): (xyz, rgb, label) as
    parse_cloud_text returns them.  The file is read block_bytes at a time into one page-locked buffer and uploaded from there;
    the unfinished last line of a block is carried in front of the next, so the batches do not depend on block_bytes and a
    cloud larger than a block streams through.  Nothing is parsed on the host.  skip_lines: that many leading (non-blank) lines
    are parsed and dropped (the header line pandas consumes in the reference's read_semantic3d_format)."""

    def __init__(self, path, n_cols, xyz_cols=(0, 1, 2), rgb_cols=None, label_col=None, rows=1 << 20, block_bytes=1 << 26,
                 skip_lines=0, device=None):
        if int(rows) < 1 or int(block_bytes) < 1 or int(skip_lines) < 0:
            raise ValueError('CloudTextReader: rows >= 1, block_bytes >= 1 and skip_lines >= 0 expected')
        _text_roles(n_cols, xyz_cols, rgb_cols, label_col)
        self.path, self.n_cols, self.cols = path, int(n_cols), (xyz_cols, rgb_cols, label_col)
        self.rows, self.block_bytes, self.skip_lines = int(rows), int(block_bytes), int(skip_lines)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def __iter__(self):
        max_line = text_layout()['max_line']
        pinned = torch.empty(self.block_bytes + max_line + 2, dtype=torch.uint8).pin_memory()
        host = pinned.numpy()
        carry, lines, offset, skip, held = 0, 0, 0, self.skip_lines, None
        with open(self.path, 'rb', buffering=0) as f:
            final = False
            while not final:
                got = 0
                while got < self.block_bytes:
                    r = f.readinto(memoryview(host)[carry + got:carry + self.block_bytes])
                    if not r:
                        final = True
                        break
                    got += r
                total = carry + got
                # (parse_cloud_text synchronises behind this copy, so the buffer is free again when it returns)
                text = pinned[:total].to(self.device, non_blocking=True)
                xyz, rgb, label, n, consumed = parse_cloud_text(text, self.n_cols, *self.cols, final_block=final,
                                                                line_base=lines, byte_base=offset, source=str(self.path))
                carry = total - consumed
                if carry > max_line + 2:
                    raise CloudTextError(lines + n, 6, offset + consumed + max_line, 1, str(self.path))
                host[:carry] = host[consumed:total].copy()
                lines, offset = lines + n, offset + consumed
                new = [None if t is None else t[min(skip, n):] for t in (xyz, rgb, label)]
                skip -= min(skip, n)
                held = new if held is None else [None if a is None else torch.cat((a, b)) for a, b in zip(held, new)]
                count = next(int(t.shape[0]) for t in held if t is not None)
                while count >= self.rows:
                    yield tuple(None if t is None else t[:self.rows] for t in held)
                    held = [None if t is None else t[self.rows:] for t in held]
                    count -= self.rows
        if held is not None and next(int(t.shape[0]) for t in held if t is not None) > 0:
            yield tuple(held)


# --------------------------------------------------------------------------------------------------
# l0 cut pursuit (csrc/spg_cutpursuit.hip): the min cut and the partition solver that libcp.cutpursuit /
# cutpursuit2 stand for.  UNPINNED against libcp (absent from the reference, unseeded k-means); tests/cutpursuit_restatement.py
# restates both and the device agrees with it exactly.
# --------------------------------------------------------------------------------------------------
MINCUT_LIMIT = 1 << 28
MINCUT_MAX_PULSES = 1 << 16          # (profiles/cutpursuit_bench.txt: the largest count measured is far below 1 / 8 of this)
CP_MAX_D = 32


def _i64_vec(t, count, name):
    _on_gpu(t, name)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f'{name} must be an integer tensor, got {t.dtype}')
    if t.shape != (count,):
        raise ValueError(f'{name} must be [{count}], got {tuple(t.shape)}')
    return _req(t.to(torch.int64).contiguous(), torch.int64, name)


def min_cut(graph: EdgeGraph, cap, cost0, cost1, max_pulses: Optional[int] = None, return_info: bool = False):
    """label uint8 [n] minimising sum_v cost_label(v) + sum_e cap_e [label_u != label_v]: cap integer [E], cost0 / cost1 integer [n]
    (the prices of labels 0 and 1), every value in [0, 2^28).  Among the minimisers the one with the fewest ones; self-loops and
    zero capacities are inert, parallel edges add up.  Integer push-relabel in pulses (spg_mincut): the result does not depend on
    scheduling.  ValueError for a value outside the range, RuntimeError when max_pulses pulses do not finish it.
    return_info: also {'pulses', 'launches', 'levels'}."""
    graph._use()
    n, E = graph.n, graph.E
    cap, cost0, cost1 = _i64_vec(cap, E, 'cap'), _i64_vec(cost0, n, 'cost0'), _i64_vec(cost1, n, 'cost1')
    max_pulses = MINCUT_MAX_PULSES if max_pulses is None else int(max_pulses)
    L, dev = lib(), graph.device
    label = torch.empty(n, dtype=torch.uint8, device=dev)
    info = (ctypes.c_int64 * 4)()
    ws = _u8_workspace(L.spg_mincut_workspace_bytes(n, E), dev)
    check(L.spg_mincut(_ptr(graph.rowptr), _ptr(graph.inc), _ptr(graph.ends), E, n, _ptr(cap), _ptr(cost0), _ptr(cost1), max_pulses,
                       _ptr(label), ctypes.cast(info, ctypes.c_void_p), _ptr(ws), ws.numel(), _stream()), 'spg_mincut')
    if info[0] & 1:
        raise ValueError('min_cut: cap, cost0 and cost1 must lie in [0, 2^28)')
    if info[0] & 2:
        raise RuntimeError(f'min_cut: vertices are still active after max_pulses = {max_pulses} pulses')
    if return_info:
        return label, {'pulses': int(info[1]), 'launches': int(info[2]), 'levels': int(info[3])}
    return label


def _cp_sums(key, mq, q, K):
    """W i64 [K] = sum mq, S i64 [K, D] = sum mq * q over the vertices with key >= 0"""
    n, D = q.shape
    W = torch.empty(K, dtype=torch.int64, device=q.device)
    S = torch.empty(K, D, dtype=torch.int64, device=q.device)
    check(lib().spg_cp_accumulate(_ptr(key), _ptr(mq), _ptr(q), n, D, K, _ptr(W), _ptr(S), _stream()), 'spg_cp_accumulate')
    return W, S


def _cp_dist(q, key, C):
    n, D = q.shape
    out = torch.empty(n, dtype=torch.float64, device=q.device)
    check(lib().spg_cp_dist(_ptr(q), _ptr(key), _ptr(C), n, D, int(C.shape[0]), _ptr(out), _stream()), 'spg_cp_dist')
    return out


def _cp_farthest(dist, key, mq, K):
    """-> (idx i64 [K]: the first positive-weight vertex of every key with the largest dist, n if none; that dist f64 [K])"""
    n = int(dist.numel())
    best = torch.empty(K, dtype=torch.int64, device=dist.device)
    idx = torch.empty(K, dtype=torch.int32, device=dist.device)
    check(lib().spg_cp_farthest(_ptr(dist), _ptr(key), _ptr(mq), n, K, _ptr(best), _ptr(idx), _stream()), 'spg_cp_farthest')
    return idx.long(), best.view(torch.float64)


def _cp_means(W, S):
    has = (W > 0)[:, None]
    return torch.where(has, S.double() / W.double().clamp(min=1.0)[:, None], torch.zeros((), dtype=torch.float64, device=W.device))


def _cp_recentre(C, key, lab, mq, q):
    key2 = torch.where(key >= 0, 2 * key + lab, key)
    W, S = _cp_sums(key2.contiguous(), mq, q, int(C.shape[0]))
    return torch.where((W > 0)[:, None], S.double() / W.double().clamp(min=1.0)[:, None], C).contiguous()


def _cp_exp(x):
    return int(np.frexp(float(x))[1])


def _cp_ldexp(x, k):
    """x * 2^k for a float64 tensor and a host integer k (exact: 2.0 ** k is a float64 for every k that can occur with float32 input)"""
    return x * (2.0 ** int(k))


def _cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam):
    W, S = _cp_sums(comp, mq, q, ncom)
    fid = (mq.double() * _cp_dist(q, comp, _cp_means(W, S).contiguous())).sum()
    cutw = w64[comp[src] != comp[tgt]].sum()
    fid, cutw = torch.stack([fid, cutw]).tolist()
    return float(np.ldexp(fid, -(km + 2 * kf)) + lam * cutw)


def _cp_first_of_groups(sorted_keys):
    first = torch.ones_like(sorted_keys, dtype=torch.bool)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return first


def _cp_renumber(r):
    """ids r i64 [n] -> (i32 [n] numbered 0.. by smallest member, count)"""
    rs, order = torch.sort(r, stable=True)
    first = _cp_first_of_groups(rs)
    roots, member = rs[first], order[first]                       # (stable: the first of a group is its smallest member)
    new = torch.zeros(int(r.max().item()) + 1, dtype=torch.int64, device=r.device)
    new[roots[torch.argsort(member)]] = torch.arange(roots.numel(), device=r.device)
    return new[r].to(torch.int32).contiguous(), int(roots.numel())


def _cp_merge_small(comp, ncom, src, tgt, w, cutoff):
    """the cutoff rounds of cut_pursuit -> (comp i32, ncom, rounds)"""
    dev, E = comp.device, int(w.numel())
    wq = torch.zeros(E, dtype=torch.int64, device=dev)
    wmax = float(w.max().item()) if E else 0.0
    if wmax > 0:
        wq = torch.round(_cp_ldexp(w.double(), 30 - _cp_exp(wmax))).long()
    rounds = 0
    while True:
        c = comp.long()
        size = torch.bincount(c, minlength=ncom)
        a, b = c[src], c[tgt]
        x = a != b
        pa, pb, pw = torch.cat([a[x], b[x]]), torch.cat([b[x], a[x]]), torch.cat([wq[x], wq[x]])
        keep = size[pa] < cutoff
        pa, pb, pw = pa[keep], pb[keep], pw[keep]
        if pa.numel() == 0:
            return comp, ncom, rounds
        pair, inv = torch.unique(pa * ncom + pb, return_inverse=True)
        tot = torch.zeros(pair.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, pw)
        ca, cb = pair // ncom, pair % ncom
        # per small component the neighbour with the largest summed weight, lowest id on ties: pairs are sorted by (ca, cb); a stable
        # sort by descending weight, then a stable sort by ca, leaves the winner first in every group
        o1 = torch.sort(tot, descending=True, stable=True)[1]
        o2 = torch.sort(ca[o1], stable=True)[1]
        order = o1[o2]
        first = _cp_first_of_groups(ca[order])
        ptr = torch.arange(ncom, device=dev)
        ptr[ca[order][first]] = cb[order][first]
        ids = torch.arange(ncom, device=dev)
        mutual = (ptr[ptr] == ids) & (ids < ptr)
        ptr = torch.where(mutual, ids, ptr)
        for _ in range(max(1, int(ncom).bit_length())):
            ptr = ptr[ptr]
        comp, ncom = _cp_renumber(ptr[c])
        rounds += 1


def cut_pursuit(obs, graph: EdgeGraph, edge_weight, node_weight=None, reg_strength=None, cutoff: int = 0, weight_decay: float = 1.0,
                max_ite: int = 5, kmeans_ite: int = 3, flow_steps: int = 2, max_pulses: Optional[int] = None, return_stats: bool = False):
    """l0 cut pursuit: a piecewise-constant x minimising sum_v m_v |x_v - f_v|^2 + reg_strength sum_e w_e [x_u != x_v] greedily by
    binary splits of every component (DESIGN.md section 4.11j states the algorithm; tests/cutpursuit_restatement.py restates it).
    obs f32 [n, D <= 32], edge_weight f32 [E] >= 0, node_weight f32 [n] >= 0 or None (all 1).
    -> (in_component i32 [n] numbered by smallest member, n_com, values f32 [n_com, D] the weighted means, energies: the float64
    energy after every iteration).  Observations and weights are quantised once (20 and 10 bits below the largest), all sums over
    vertices are int64 and the cuts are integer min cuts (min_cut), so the partition does not depend on scheduling.
    return_stats: also {'pulses': per min cut, 'launches', 'merge_rounds'}."""
    graph._use()
    if reg_strength is None:
        raise TypeError('cut_pursuit: reg_strength is required')
    n, E, dev = graph.n, graph.E, graph.device
    obs = _req(obs, torch.float32, 'obs')
    if obs.dim() != 2 or obs.shape[0] != n or obs.shape[1] < 1:
        raise ValueError(f'obs must be [{n}, D] with D >= 1, got {tuple(obs.shape)}')
    D = int(obs.shape[1])
    if D > CP_MAX_D:
        raise ValueError(f'cut_pursuit: D <= {CP_MAX_D} expected, got D = {D}')
    w = _edge_vec(_on_gpu(edge_weight, 'edge_weight'), torch.float32, E, 'edge_weight')
    m = torch.ones(n, dtype=torch.float32, device=dev) if node_weight is None else _on_gpu(node_weight, 'node_weight')
    m = _req(m.to(torch.float32).contiguous(), torch.float32, 'node_weight')
    if m.shape != (n,):
        raise ValueError(f'node_weight must be [{n}], got {tuple(m.shape)}')
    zero = torch.zeros(1, dtype=torch.float32, device=dev)
    finite = torch.isfinite(obs).all() & torch.isfinite(w).all() & torch.isfinite(m).all()
    head = torch.stack([(~finite).float(), obs.abs().max(), m.max(), m.min(), torch.cat([w, zero]).min()]).tolist()
    _raise_nonfinite(int(head[0]))
    if not np.isfinite(float(reg_strength)) or reg_strength < 0:
        raise ValueError(f'cut_pursuit: reg_strength >= 0 and finite expected, got {reg_strength}')
    if head[3] < 0:
        raise ValueError('cut_pursuit: node_weight >= 0 expected')
    if head[4] < 0:
        raise ValueError('cut_pursuit: edge_weight >= 0 expected')
    kf, km = 20 - _cp_exp(head[1]), 10 - _cp_exp(head[2])
    q = torch.round(_cp_ldexp(obs.double(), kf)).to(torch.int32).contiguous()
    mq = torch.round(_cp_ldexp(m.double(), km)).to(torch.int32).contiguous()
    qd, mqd, w64 = q.double(), mq.double(), w.double()
    src, tgt = graph.ends[:, 0].long(), graph.ends[:, 1].long()
    comp, ncom = torch.zeros(n, dtype=torch.int32, device=dev), 1
    sat = torch.zeros(n, dtype=torch.bool, device=dev)
    cut = torch.zeros(E, dtype=torch.bool, device=dev)
    minus1 = torch.full((), -1, dtype=torch.int32, device=dev)
    energies, pulses, launches = [], [], 0
    for t in range(int(max_ite)):
        lam = float(reg_strength) * float(weight_decay) ** t
        K = ncom
        key = torch.where(sat, minus1, comp).contiguous()
        W, S = _cp_sums(key, mq, q, K)
        i0, _ = _cp_farthest(_cp_dist(q, key, _cp_means(W, S).contiguous()), key, mq, K)
        C0 = qd[i0.clamp(max=n - 1)].contiguous()
        i1, far = _cp_farthest(_cp_dist(q, key, C0), key, mq, K)
        C1 = qd[i1.clamp(max=n - 1)]
        done = (W == 0) | (far <= 0)
        sat = sat | done[comp.long()]
        key = torch.where(sat, minus1, comp).contiguous()
        if bool(sat.all().item()):
            energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
            break
        C = torch.stack([C0, C1], 1).reshape(2 * K, D).contiguous()
        k0 = torch.where(key >= 0, 2 * key, minus1).contiguous()
        k1 = torch.where(key >= 0, 2 * key + 1, minus1).contiguous()
        lab = torch.zeros(n, dtype=torch.int32, device=dev)
        for _ in range(int(kmeans_ite)):
            lab = (_cp_dist(q, k1, C) < _cp_dist(q, k0, C)).to(torch.int32)
            C = _cp_recentre(C, key, lab, mq, q)
        for _ in range(int(flow_steps)):
            u = mqd * (_cp_dist(q, k0, C) - _cp_dist(q, k1, C))
            capf = torch.where(cut, torch.zeros((), dtype=torch.float64, device=dev),
                               _cp_ldexp(lam * w64, km + 2 * kf))
            M = float(torch.cat([u.abs(), capf]).max().item())
            p = 27 - _cp_exp(M) if M > 0 else 0
            uq = torch.round(_cp_ldexp(u, p)).long()
            capq = torch.round(_cp_ldexp(capf, p)).long()
            lab8, info = min_cut(graph, capq, uq.clamp(min=0), (-uq).clamp(min=0), max_pulses=max_pulses, return_info=True)
            pulses.append(info['pulses'])
            launches += info['launches']
            lab = lab8.to(torch.int32)
            C = _cp_recentre(C, key, lab, mq, q)
        newcut = ~cut & (lab[src] != lab[tgt])
        c = comp.long()
        ones = torch.zeros(ncom, dtype=torch.int64, device=dev).index_add_(0, c, lab.long())
        size = torch.bincount(c, minlength=ncom)
        sat = sat | ((ones == 0) | (ones == size))[c]
        if not bool(newcut.any().item()):
            energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
            break
        comp, ncom, _ = connected_components(graph, (~(cut | newcut)).to(torch.uint8))
        cut = comp[src] != comp[tgt]
        energies.append(_cp_energy(q, mq, kf, km, comp, ncom, src, tgt, w64, lam))
        if bool(sat.all().item()):
            break
    rounds = 0
    if cutoff > 0:
        comp, ncom, rounds = _cp_merge_small(comp, ncom, src, tgt, w, int(cutoff))
    W, S = _cp_sums(comp, mq, q, ncom)
    c = comp.long()
    P = torch.zeros(ncom, D, dtype=torch.int64, device=dev).index_add_(0, c, q.long())
    size = torch.bincount(c, minlength=ncom)
    num = torch.where((W > 0)[:, None], S, P).double()
    den = torch.where(W > 0, W, size).double()
    values = _cp_ldexp(num / den[:, None], -kf).float()
    if return_stats:
        return comp, ncom, values, energies, {'pulses': pulses, 'launches': launches, 'merge_rounds': rounds}
    return comp, ncom, values, energies
