"""RNN-ECC module and GRU / LSTM cells with the reference's module API (learning/modules.py:128-316)."""
import torch
import torch.nn as nn

from .. import _lib, ops
from ..flat import mark_direct_write, prepare_autograd_fallback
from . import _layers


class _CellEx:
    """What GRUCellEx and LSTMCellEx add to torch's cells: row normalisation of the gate pre-activations and an input gate
    (same parameters as the reference: weight_ih, weight_hh, bias_ih, bias_hh, ig.*); the HIP kernels serve hidden = input in
    ops.model.CELL_WIDTHS (8, 16, 32, 64, 128) with bias."""

    def __init__(self, input_size, hidden_size, bias=True, layernorm=True, ingate=True):
        super().__init__(input_size, hidden_size, bias)
        self._layernorm = layernorm
        self._ingate = ingate
        if layernorm:
            self.add_module('ini', nn.InstanceNorm1d(1, eps=1e-5, affine=False, track_running_stats=False))
            self.add_module('inh', nn.InstanceNorm1d(1, eps=1e-5, affine=False, track_running_stats=False))
        if ingate:
            self.add_module('ig', nn.Linear(hidden_size, input_size, bias=True))

    def param_tensors(self):
        return _layers.cell_row(self)

    def _autograd_params(self, input):
        if not input.is_cuda:
            raise RuntimeError(f'superpoint_graph_amd.{type(self).__name__} has no CPU path')
        self._check_supported()
        return [p for p in self.param_tensors() if p is not None]

    def _check_supported(self):
        """NotImplementedError, before any launch, for what the HIP cells do not serve; the message names what they do."""
        if self.input_size != self.hidden_size or self.bias_ih is None:
            raise NotImplementedError(f'the HIP {self._KIND} cell needs input_size == hidden_size and bias=True (got input_size '
                                      f'{self.input_size}, hidden_size {self.hidden_size}, bias {self.bias_ih is not None}); '
                                      f'supported widths: {", ".join(map(str, ops.model.CELL_WIDTHS))}')
        ops.model.check_cell_width(self.hidden_size, what=f'the HIP {self._KIND} cell')

    def __repr__(self):
        s = super().__repr__() + '('
        if self._ingate:
            s += 'ingate'
        if self._layernorm:
            s += ' layernorm'
        return s + ')'


class GRUCellEx(_CellEx, nn.GRUCell):
    """GRU cell of the reference (learning/modules.py:205-259); forward/backward run in one fused HIP kernel each."""
    _KIND = 'GRU'

    def forward(self, input, hidden):
        return _GRUCellFunction.apply(self, input.contiguous(), hidden.contiguous(), *self._autograd_params(input))


class _GRUCellFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cell, input, hidden, *params):
        ctx.cell = cell
        ctx.save_for_backward(input, hidden)
        return ops.gru_cell_fwd(input, hidden, cell.param_tensors(), cell._layernorm, cell._ingate)

    @staticmethod
    def backward(ctx, grad_out):
        input, hidden = ctx.saved_tensors
        cell = ctx.cell
        gi, gh, grads = ops.gru_cell_bwd(input, hidden, grad_out, cell.param_tensors(), cell._layernorm, cell._ingate)
        return (None, gi, gh) + tuple(g for g in grads if g is not None)


class LSTMCellEx(_CellEx, nn.LSTMCell):
    """LSTM cell of the reference (learning/modules.py:262-316).  forward(input, (h, c)) -> (hy, cy), one fused HIP kernel
    each way."""
    _KIND = 'LSTM'

    def forward(self, input, hidden):
        params = self._autograd_params(input)
        return _LSTMCellFunction.apply(self, input.contiguous(), hidden[0].contiguous(), hidden[1].contiguous(), *params)


class _LSTMCellFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cell, input, h, c, *params):
        ctx.cell = cell
        ctx.save_for_backward(input, h, c)
        return ops.lstm_cell_fwd(input, h, c, cell.param_tensors(), cell._layernorm, cell._ingate)

    @staticmethod
    def backward(ctx, grad_hy, grad_cy):
        input, h, c = ctx.saved_tensors
        cell = ctx.cell
        gi, gh, gc, grads = ops.lstm_cell_bwd(input, h, c, grad_hy, grad_cy, cell.param_tensors(), cell._layernorm, cell._ingate)
        return (None, gi, gh, gc) + tuple(g for g in grads if g is not None)


class _LinearFunction(torch.autograd.Function):
    """nn.Linear on the few-row MFMA kernels: y = x W^T + b; backward = data gradient, weight gradient, bias column sum."""

    @staticmethod
    def forward(ctx, module, x, weight, bias):
        ctx.module = module
        ctx.save_for_backward(x, weight)
        return ops.linear_fwd(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        m = ctx.module
        gy = gy.contiguous()
        need_dx = ctx.needs_input_grad[1]
        direct = getattr(m, '_spg_direct_grads', False) and weight.grad is not None and weight.grad.is_contiguous() and \
            (m.bias is None or (m.bias.grad is not None and m.bias.grad.is_contiguous()))
        if direct:          # FlatParameters: write into the arena views, nothing for autograd to accumulate
            mark_direct_write(m)
            gx, _, _ = ops.linear_backward(gy, x, weight, need_dx, m.bias is not None, out_w=weight.grad,
                                           out_b=None if m.bias is None else m.bias.grad)
            return None, gx, None, None
        if getattr(m, '_spg_direct_grads', False):
            if any(p is not None and p.requires_grad and (p.grad is None or not p.grad.is_contiguous()) for p in (weight, m.bias)):
                raise RuntimeError(_layers.ARENA_ERROR)
            prepare_autograd_fallback(m)       # partly frozen layer: autograd accumulates what is returned
        gx, gw, gb = ops.linear_backward(gy, x, weight, need_dx, m.bias is not None)
        return None, gx, gw, gb


class HipLinear(nn.Linear):
    """`nn.Linear` (same parameters / state_dict keys / initialisation) whose forward and backward run on the HIP kernels
    for 2-d float32 CUDA inputs -- the classifier of the graph network (reference learning/graphnet.py:47-49).  torch's
    path costs three hipBLASLt launches with host-side argument uploads, a reduction and two accumulations per step."""

    def _kernel_shape_ok(self):
        w = self.weight
        return w.is_contiguous() and w.shape[1] % 4 == 0 and w.data_ptr() % 16 == 0

    _spg_kernel_grads = property(_kernel_shape_ok)      # FlatParameters: the HIP backward writes the gradient views on the kernel path

    def forward(self, input):
        if input.is_cuda and input.dim() == 2 and input.dtype == torch.float32 and self._kernel_shape_ok():
            return _LinearFunction.apply(self, input.contiguous(), self.weight, self.bias)
        if getattr(self, '_spg_direct_grads', False) and torch.is_grad_enabled():
            prepare_autograd_fallback(self)       # torch's path accumulates: see FlatParameters(lazy_zero=True)
        return super(HipLinear, self).forward(input)


class _EccRnnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, cfg, rows, hx, edgefeats, graph, training, *flat_params):
        out, state = ops.eccrnn_forward(cfg, graph, hx.contiguous(), edgefeats, rows, training, 1)
        ctx.module, ctx.state, ctx.rows, ctx.nflat = module, state, rows, len(flat_params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        def run(out_grads):
            grad_h0, gg = ops.eccrnn_backward(ctx.state, ctx.rows, grad_out, out_grads)
            return gg, grad_h0
        flat, grad_h0 = _layers.arena_or_autograd(ctx.module, ctx.rows, ctx.nflat, run)
        return (None, None, None, grad_h0, None, None, None) + flat


class RNNGraphConvModule(nn.Module):
    """Recurrent graph convolution: filter-generating network once, then nrepeats x {ECC, RNN cell}
    (reference learning/modules.py:128-183; same constructor signature, `_cell` / `_fnet` attribute names).
    With a GRUCellEx / LSTMCellEx cell of a supported width (ops.model.CELL_WIDTHS; matrix filters up to 64) the whole module is one C
    call (spg_eccrnn_forward); the one-launch recurrence serves 32 channels, the other widths run one launch per iteration."""
    _spg_kernel_grads = True      # FlatParameters: the HIP backward writes the gradient views of filter network and cell

    def __init__(self, cell, filter_net, nfeat=None, vv=True, gc_info=None, nrepeats=1, cat_all=False,
                 edge_mem_limit=1e20, use_pyg=True, cuda=True):
        super(RNNGraphConvModule, self).__init__()
        self._cell = cell
        self._isLSTM = 'LSTM' in type(cell).__name__
        self._fnet = filter_net
        self._nrepeats = nrepeats
        self._cat_all = cat_all
        self._edge_mem_limit = edge_mem_limit
        self._vv = vv
        self.set_info(gc_info)
        self.use_pyg = use_pyg
        if use_pyg:
            raise NotImplementedError('--use_pyg 1 (torch_geometric NNConv) is out of scope of the HIP path; use --use_pyg 0')

    def set_info(self, gc_info):
        self._gci = gc_info

    def _cfg_and_groups(self):
        """(cfg, rows): the cached configuration, and the filter network's layer rows followed by the cell's row."""
        cached = self.__dict__.get('_cg_cache')
        if cached is None:
            cached = self.__dict__['_cg_cache'] = self._build_cfg_and_modules()
        cfg, fg = cached
        return cfg, [_layers.layer_row(lin, bn) for lin, bn in fg] + [_layers.cell_row(self._cell)]

    def _cfg_for(self, cfg, gci, n_nodes):
        """The configuration of this batch: the cached `cfg`, with the batch's scene boundaries attached when the graph is
        too large for one round of the one-launch GRU recurrence (include/spg_hip.h: spg_eccrnn_cfg.n_parts) -- whole scenes are
        then processed in rounds instead of one launch per iteration.  A copy per distinct partition: the configuration object of
        a forward travels with its saved state to the backward."""
        parts = getattr(gci, '_parts', None)
        if parts is None or n_nodes <= 2048 or len(parts) - 1 > _lib.SPG_MAX_PARTS or len(parts) < 3:
            return cfg
        key = tuple(parts)
        cache = self.__dict__.setdefault('_cfg_parts_cache', {})
        c2 = cache.get(key)
        if c2 is None:
            c2 = type(cfg).from_buffer_copy(cfg)
            c2.n_parts = len(parts) - 1
            for i, v in enumerate(parts):
                c2.part_ptr[i] = int(v)
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            cache[key] = c2
        return c2

    def _build_cfg_and_modules(self):
        fg = _layers.layer_pairs(self._fnet, _layers.FNET_STACK)
        widths = [fg[0][0].in_features] + [lin.out_features for lin, _ in fg]
        nc = self._cell.hidden_size
        matrix = widths[-1] == nc * nc and widths[-1] != nc
        self._cell._check_supported()      # the cell's own refusals (width, input_size, bias)
        ops.model.check_cell_width(nc, matrix, 'the fused RNN-ECC path')
        bn = next((b for _, b in fg if b is not None), None)
        if bn is not None:
            _layers.bn_momentum(bn)
        cfg = ops.make_eccrnn_cfg(nc, self._nrepeats, matrix, self._cell._layernorm, self._cell._ingate, self._cat_all,
                                  widths, _layers.fnet_bnidx(fg), fg[-1][0].bias is not None,
                                  1e-5 if bn is None else bn.eps, 0.1 if bn is None or bn.momentum is None else bn.momentum,
                                  cell='lstm' if self._isLSTM else 'gru')
        return cfg, fg

    def forward(self, hx):
        if not hx.is_cuda:
            raise RuntimeError('superpoint_graph_amd.RNNGraphConvModule has no CPU path')
        idxn, idxe, degs, degs_gpu, edgefeats = self._gci.get_buffers()
        if idxe is not None:
            raise NotImplementedError('filter sharing (idxe) is not supported by the fused RNN-ECC path')
        cfg, rows = self._cfg_and_groups()      # (first: refuses an unsupported width before anything is launched)
        if self.training:
            _layers.advance_batch_counters(self._fnet)
        graph = self._gci.device_graph()
        cfg = self._cfg_for(cfg, self._gci, graph.N)
        return _EccRnnFunction.apply(self, cfg, rows, hx, edgefeats.contiguous().float(), graph, self.training,
                                     *_layers.node_inputs(self, rows, hx.device))
