"""The glue between nn.Module and the C ABI, stated once: which tensors a layer hands to libspg_hip and in what order (the
6-pointer rows of include/spg_hip.h), which of them autograd sees, where each gradient lands in FlatParameters mode, and the
BatchNorm batch counters.  PointNet / STNkD (pointnet.py), the RNN-ECC module and its cells (modules.py) and FusedStep
(fused.py) are built on it; it imports none of them.

Only the module STRUCTURE is ever cached by the callers: tensors are looked up from the module objects on every call, because
.to() / load_state_dict() replace buffers and FlatParameters re-points .data / .grad."""
import torch
import torch.nn as nn

from ..flat import mark_direct_write

ARENA_ERROR = ('FlatParameters mode: a parameter has no contiguous .grad view into the gradient arena '
               '(optimizer.zero_grad(set_to_none=True) or a frozen parameter?); use FlatParameters.zero_grad()')
FUSED_ARENA_ERROR = 'FusedStep: a parameter has no contiguous .grad view into the gradient arena'

# what a Sequential may hold: (parametric layers, normalisations, tolerated parameter-free modules, refusal of anything else)
POINTNET_STACK = ((nn.Conv1d, nn.Linear), (nn.BatchNorm1d, nn.GroupNorm), (nn.ReLU, nn.Dropout),
                  '{} is not supported by the HIP PointNet (norm must be "batch", "layer" or "group")')
FNET_STACK = ((nn.Linear,), (nn.BatchNorm1d,), (nn.ReLU,), 'unsupported filter-network module {}')


def layer_pairs(seq, kind):
    """(layer, norm-or-None) per parametric layer of a Sequential[layer, (norm), ReLU, ...]; `kind`: POINTNET_STACK | FNET_STACK."""
    layers, norms, passive, refusal = kind
    pairs, mods = [], list(seq)
    for i, m in enumerate(mods):
        if isinstance(m, layers):
            pairs.append((m, mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], norms) else None))
        elif not isinstance(m, norms + passive):
            raise NotImplementedError(refusal.format(type(m).__name__))
    return pairs


def fnet_bnidx(pairs):
    """create_fnet()'s `bnidx`: the (last) layer of the filter network followed by a BatchNorm, -1 for none."""
    return max((i for i, (_, norm) in enumerate(pairs) if norm is not None), default=-1)


class LayerRow(tuple):
    """Six tensors (or None) of one table row in the order of include/spg_hip.h: (weight, bias, norm.weight, norm.bias,
    running_mean, running_var) of a layer.  The first `live` entries carry a gradient."""
    live, zero_bias = 4, False


class BatchNormLayerRow(LayerRow):
    """A layer in front of a train-mode BatchNorm: the gradient of its bias is exactly zero and is never written.  (BatchNorm's
    rule alone: the GroupNorm kernels normalise per cloud, not per channel, and write the bias gradient.)"""
    zero_bias = True


class CellRow(LayerRow):
    """(weight_ih, weight_hh, bias_ih, bias_hh, ig.weight, ig.bias) of a GRUCellEx / LSTMCellEx."""
    live = 6


def layer_row(lin, norm):
    if norm is None:
        return LayerRow((lin.weight, lin.bias, None, None, None, None))
    row = BatchNormLayerRow if isinstance(norm, nn.BatchNorm1d) else LayerRow
    return row((lin.weight, lin.bias, norm.weight, norm.bias, getattr(norm, 'running_mean', None), getattr(norm, 'running_var', None)))


def cell_row(cell):
    ig = cell._modules['ig'] if cell._ingate else None
    return CellRow((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
                    None if ig is None else ig.weight, None if ig is None else ig.bias))


def flat_params(rows):
    """The autograd input list of a HIP node: every live tensor, row by row."""
    return [t for row in rows for t in row[:row.live] if t is not None]


def grad_targets(rows, strict=False):
    """The .grad views (FlatParameters: into one flat gradient buffer) the kernels write directly: one tuple of `row.live`
    entries per row, None where there is no parameter or nothing is written.  A missing or non-contiguous view gives None
    for the whole table, or raises when `strict`."""
    out = []
    for row in rows:
        tgt = []
        for k in range(row.live):
            t = row[k]
            if t is None or (row.zero_bias and k == 1):
                tgt.append(None)
            elif t.grad is None or not t.grad.is_contiguous():
                if strict:
                    raise RuntimeError(FUSED_ARENA_ERROR)
                return None
            else:
                tgt.append(t.grad)
        out.append(tuple(tgt))
    return out


def bn_momentum(bn):
    """BatchNorm1d(momentum=None) means a cumulative moving average and track_running_stats=False means batch statistics
    in eval mode: neither is implemented by the kernels (exponential average only) -- refuse instead of silently using 0.1."""
    if bn.momentum is None:
        raise NotImplementedError('BatchNorm1d(momentum=None) (cumulative average) is not implemented on the HIP path')
    if not bn.track_running_stats or bn.running_mean is None:
        raise NotImplementedError('BatchNorm1d(track_running_stats=False) is not implemented on the HIP path')
    return bn.momentum


def advance_batch_counters(root, times=1):
    """num_batches_tracked += times for every BatchNorm below `root` (a module or a Sequential) in one launch -- none when the
    counters live on the host (FlatParameters(host_counters=True))."""
    bns = root.__dict__.get('_spg_bn_cache')
    if bns is None:               # the module structure is fixed after construction
        bns = root.__dict__['_spg_bn_cache'] = [m for m in root.modules()
                                                if isinstance(m, nn.BatchNorm1d) and m.num_batches_tracked is not None]
    if bns:
        torch._foreach_add_([m.num_batches_tracked for m in bns], times)


_anchors = {}


def grad_anchor(device):
    """A 1-element tensor that requires grad: the single differentiable input of the HIP autograd nodes in FlatParameters mode."""
    a = _anchors.get(device)
    if a is None:
        a = _anchors[device] = torch.zeros(1, device=device, requires_grad=True)
    return a


def node_inputs(module, rows, device):
    """The trailing inputs of a HIP autograd node.  In FlatParameters mode the kernels write the gradients into the arena, so
    autograd only needs ONE differentiable input to create the node (instead of tracking ~60 parameter tensors)."""
    if getattr(module, '_spg_direct_grads', False) and torch.is_grad_enabled():
        return [grad_anchor(device)]
    return flat_params(rows)


def arena_or_autograd(module, rows, nflat, backward):
    """The parameter half of a HIP node's backward.  `backward(out_grads)` launches the kernels -- writing into `out_grads` (see
    grad_targets) unless it is None -- and returns (gradient rows, whatever else the node returns).
    -> (the gradients of the node's `nflat` trailing inputs, that remainder)."""
    arena = getattr(module, '_spg_direct_grads', False)
    direct = grad_targets(rows) if arena else None
    if direct is not None:      # gradients are written straight into the pre-assigned .grad views, nothing for autograd to accumulate
        mark_direct_write(module)
        return (None,) * nflat, backward(direct)[1]
    if arena and nflat == 1:    # the anchor is the only input: autograd could not deliver the gradients
        raise RuntimeError(ARENA_ERROR)
    gg, rest = backward(None)
    return tuple(g for row, grow in zip(rows, gg) for g in grow[:row.live] if g is not None), rest
