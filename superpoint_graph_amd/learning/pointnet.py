"""PointNet superpoint embedder with the reference's module API (learning/pointnet.py:16-180).

The classes own the SAME parameters under the SAME state_dict keys as the reference (they are built from
the same nn.Conv1d / nn.BatchNorm1d / nn.Linear containers in the same order, so initialisation under a
given seed is identical and reference checkpoints load), but `forward` hands the parameter pointers to
libspg_hip (spg_pointnet_forward / spg_pointnet_backward): fused 1x1-conv + BatchNorm + ReLU + max-pool
MFMA kernels instead of cuDNN/cuBLAS calls."""
import torch
import torch.nn as nn

from .. import ops
from . import _layers


def _norm_module(norm, n_group, width):
    """The normalisation the reference puts behind a layer of `width` channels (learning/pointnet.py:30-35)."""
    if norm == 'batch':
        return nn.BatchNorm1d(width)
    if norm == 'layer':
        return nn.GroupNorm(1, width)
    if norm == 'group':
        return nn.GroupNorm(n_group, width)
    raise ValueError(f'norm must be "batch", "layer" or "group", got {norm!r}')


def _stack(layer, nin, widths, norm, n_group, bare_last=False, prelast_do=0):
    """The modules of a Sequential[layer(in, out), norm, ReLU, ...] over `widths`, constructed in the reference's order
    (learning/pointnet.py:24-47, 81-105).  bare_last: neither norm nor ReLU behind the last layer; prelast_do: Dropout in front of it."""
    modules = []
    for i, width in enumerate(widths):
        modules.append(layer(widths[i - 1] if i > 0 else nin, width))
        if i < len(widths) - 1 or not bare_last:
            modules.append(_norm_module(norm, n_group, width))
            modules.append(nn.ReLU(True))
        if i == len(widths) - 2 and prelast_do > 0:
            modules.append(nn.Dropout(prelast_do))
    return modules


def _conv1x1(nin, nout):
    return nn.Conv1d(nin, nout, 1)


def _groupnorm_spec(*modules):
    """None for BatchNorm networks; (n_group, eps) when every normalisation of `modules` is a GroupNorm with one group count.
    A mix of BatchNorm and GroupNorm, or GroupNorms that differ, are refused: no kernel covers them."""
    norms = [m for mod in modules for m in mod.modules() if isinstance(m, (nn.BatchNorm1d, nn.GroupNorm))]
    gns = [m for m in norms if isinstance(m, nn.GroupNorm)]
    if not gns:
        return None
    if len(gns) != len(norms):
        raise NotImplementedError('a mix of BatchNorm and GroupNorm in one model is not implemented on the HIP path '
                                  '(build the STN and the PointNet with the same `norm`)')
    spec = {(m.num_groups, m.eps) for m in gns}
    if len(spec) != 1:
        raise NotImplementedError(f'GroupNorm layers with different (num_groups, eps) {sorted(spec)} are not implemented on the HIP path')
    if any(not m.affine for m in gns):
        raise NotImplementedError('GroupNorm(affine=False) is not implemented on the HIP path')
    return spec.pop()


class _LayerTable(nn.Module):
    """What STNkD and PointNet share: `layer_groups()` -- their (Conv1d | Linear, norm-or-None) pairs -- as the rows of tensors
    that the library takes."""
    _spg_kernel_grads = True      # FlatParameters: the HIP backward writes the gradient views of every parameter below

    def _groups_tensors(self):
        return [_layers.layer_row(lin, norm) for lin, norm in self.layer_groups()]

    def _bump_batches_tracked(self, times):
        _layers.advance_batch_counters(self, times)


class STNkD(_LayerTable):
    """Spatial Transformer Net producing a KxK transformation matrix (reference learning/pointnet.py:16-61).
    Inside PointNet it is evaluated by the fused HIP pipeline; called on its own it runs the same kernels
    through a PointNet-less plan (K must be 2)."""

    def __init__(self, nfeat, nf_conv, nf_fc, K=2, norm='batch', affine=True, n_group=1):
        super(STNkD, self).__init__()
        self.convs = nn.Sequential(*_stack(_conv1x1, nfeat, nf_conv, norm, n_group))
        self.fcs = nn.Sequential(*_stack(nn.Linear, nf_conv[-1], nf_fc, norm, n_group))
        self.proj = nn.Linear(nf_fc[-1], K * K)
        nn.init.constant_(self.proj.weight, 0)
        nn.init.constant_(self.proj.bias, 0)
        self.eye = torch.eye(K).unsqueeze(0)
        self._nfeat, self._nf_conv, self._nf_fc, self._K = nfeat, list(nf_conv), list(nf_fc), K

    # ---- stand-alone evaluation (inside PointNet the STN is part of the fused pipeline) ----
    # An STN is structurally a PointNet segment without its own STN and without global features:
    # convs -> max-pool -> fcs -> plain last layer (proj); the same C entry points run it.
    def layer_groups(self):
        return (_layers.layer_pairs(self.convs, _layers.POINTNET_STACK) + _layers.layer_pairs(self.fcs, _layers.POINTNET_STACK)
                + [(self.proj, None)])

    def _cfg(self, npts):
        bn0 = self.convs[1]
        ops.model.pointnet_segments(npts)      # NotImplementedError with the rule for an npts the kernels do not serve
        return ops.make_pointnet_cfg(self._nfeat, 0, 0, npts, [], [], self._nf_conv, self._nf_fc + [self._K * self._K], False,
                                     bn0.eps, _layers.bn_momentum(bn0))

    def _gn_cfg(self, npts):
        n_group, eps = _groupnorm_spec(self)
        return ops.make_gn_cfg(self._nfeat, 0, npts, self._nf_conv, self._nf_fc + [self._K * self._K], n_group, eps)

    def forward(self, input):
        """[B, nfeat, P] -> [B, K, K] transformation matrices (reference learning/pointnet.py:55-61)."""
        if not input.is_cuda:
            raise RuntimeError('superpoint_graph_amd.STNkD has no CPU path; move the module and inputs to the GPU')
        self.eye = self.eye.to(input.device)
        input, rows = input.contiguous().float(), self._groups_tensors()
        if _groupnorm_spec(self) is not None:      # norm = 'layer' | 'group': the cloud-resident kernels (spg_groupnorm.hip)
            out = _GroupNormFunction.apply(self, rows, input, None, None, *_layers.flat_params(rows))
        else:
            self._cfg(input.shape[2])      # (an unsupported npts is refused here, before the batch counters move)
            if self.training:
                self._bump_batches_tracked(1)
            out = _PointNetFunction.apply(self, rows, input, None, None, self.training, 1, *_layers.node_inputs(self, rows, input.device))
        return out.view(-1, self.eye.size(1), self.eye.size(2)) + self.eye


def _minus_identity(T):
    """[B, 4] = T - I of externally computed 2x2 matrices, as the *_ext entry points take them (None: no transform)."""
    return None if T is None else T.reshape(-1, 4) - torch.eye(2, device=T.device, dtype=T.dtype).reshape(1, 4)


class _PointNetFunction(torch.autograd.Function):
    """autograd node around spg_pointnet_forward / spg_pointnet_backward; parameters are passed as inputs so that autograd
    delivers their gradients (FlatParameters mode: one anchor, the kernels write into the arena).  With `T` it is a PointNet
    WITHOUT inner STN whose xy channels are transformed by externally computed 2x2 matrices, differentiable wrt those
    matrices and wrt the global features (what LocalCloudEmbedder.run_batch composes, learning/pointnet.py:188-205)."""

    @staticmethod
    def forward(ctx, module, rows, clouds, clouds_global, T, training, bn_update_times, *flat_params):
        emb, state = ops.pointnet_forward(module._cfg(clouds.shape[2]), clouds, clouds_global, rows, training, bn_update_times,
                                          ext_transform=_minus_identity(T))
        ctx.module, ctx.state, ctx.rows, ctx.nflat = module, state, rows, len(flat_params)
        return emb

    @staticmethod
    def backward(ctx, grad_emb):
        def run(out_grads):
            if ctx.state.ext_transform is None:
                return ops.pointnet_backward(ctx.state, ctx.rows, grad_emb, out_grads), (None, None)
            gg, g_T, g_glob = ops.pointnet_backward(ctx.state, ctx.rows, grad_emb, out_grads, want_input_grads=True)
            return gg, (g_glob, g_T.view(-1, 2, 2))
        flat, (g_glob, g_T) = _layers.arena_or_autograd(ctx.module, ctx.rows, ctx.nflat, run)
        return (None, None, None, g_glob, g_T, None, None) + flat


class _GroupNormFunction(torch.autograd.Function):
    """A GroupNorm / LayerNorm network without inner STN (a stand-alone STNkD, or a PointNet with nfeat_stn = 0) through
    spg_gn_forward_ext / spg_gn_backward_ext: differentiable wrt the clouds, the global features, the externally computed
    2x2 matrices `T` (None: no transform) and the parameters.  Train and eval are the same function."""

    @staticmethod
    def forward(ctx, module, rows, clouds, clouds_global, T, *flat_params):
        out, state = ops.gn_forward(module._gn_cfg(clouds.shape[2]), clouds, clouds_global, rows, ext_transform=_minus_identity(T))
        ctx.state, ctx.rows, ctx.glob_shape = state, rows, None if clouds_global is None else clouds_global.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gg, g_T, g_glob, g_clouds = ops.gn_backward(ctx.state, ctx.rows, grad_out, want_clouds=ctx.needs_input_grad[2])
        if g_T is not None:
            g_T = g_T.view(-1, 2, 2)
        if g_glob is not None:
            g_glob = g_glob.view(ctx.glob_shape)
        flat = [g for row in gg for g in row if g is not None]
        return (None, None, g_clouds, g_glob, g_T) + tuple(flat)


class PointNet(_LayerTable):
    """PointNet with one spatial transformer and a "global" input concatenated after the max-pool
    (reference learning/pointnet.py:63-133; same constructor signature)."""

    def __init__(self, nf_conv, nf_fc, nf_conv_stn, nf_fc_stn, nfeat, nfeat_stn=2, nfeat_global=1, prelast_do=0.5,
                 last_ac=False, is_res=False, norm='batch', affine=True, n_group=1, last_bn=False):
        super(PointNet, self).__init__()
        torch.manual_seed(0)          # reference learning/pointnet.py:78
        if nfeat_stn > 0:
            self.stn = STNkD(nfeat_stn, nf_conv_stn, nf_fc_stn, norm=norm, n_group=n_group)
        self.nfeat_stn = nfeat_stn
        self.convs = nn.Sequential(*_stack(_conv1x1, nfeat, nf_conv, norm, n_group))
        modules = _stack(nn.Linear, nf_conv[-1] + nfeat_global, nf_fc, norm, n_group, not last_ac, prelast_do)
        if is_res:
            nn.init.normal_(modules[-1].weight, mean=0, std=1e-2)
            nn.init.normal_(modules[-1].bias, mean=0, std=1e-2)
        self.fcs = nn.Sequential(*modules)
        self._nfeat, self._nfeat_global, self._last_ac, self._prelast_do = nfeat, nfeat_global, last_ac, prelast_do
        self._nf_conv, self._nf_fc = list(nf_conv), list(nf_fc)

    # ---- parameter plumbing ----
    def layer_groups(self):
        lg = self.__dict__.get('_lg_cache')
        if lg is None:                # the module structure is fixed after construction
            lg = self.stn.layer_groups() if self.nfeat_stn > 0 else []
            lg = lg + _layers.layer_pairs(self.convs, _layers.POINTNET_STACK) + _layers.layer_pairs(self.fcs, _layers.POINTNET_STACK)
            self.__dict__['_lg_cache'] = lg
        return lg

    def _cfg(self, npts):
        cache = self.__dict__.setdefault('_cfg_cache', {})
        if npts not in cache:
            ops.model.pointnet_segments(npts)      # NotImplementedError with the rule for an npts the kernels do not serve
            stn_conv = self.stn._nf_conv if self.nfeat_stn > 0 else []
            stn_fc = self.stn._nf_fc if self.nfeat_stn > 0 else []
            bn0 = self.convs[1]
            cache[npts] = ops.make_pointnet_cfg(self._nfeat, self.nfeat_stn, self._nfeat_global, npts, stn_conv, stn_fc,
                                                self._nf_conv, self._nf_fc, self._last_ac, bn0.eps, _layers.bn_momentum(bn0))
        return cache[npts]

    def _gn_spec(self):
        """None for a BatchNorm model, else (n_group, eps); refuses what the GroupNorm kernels do not cover."""
        if '_gn_spec_cache' in self.__dict__:      # the module structure is fixed after construction (as layer_groups assumes)
            return self.__dict__['_gn_spec_cache']
        spec = _groupnorm_spec(self)
        if spec is not None and self.nfeat_stn > 0:
            raise NotImplementedError('a GroupNorm / LayerNorm PointNet with an inner STN (nfeat_stn > 0, CloudEmbedder) is not implemented '
                                      'on the HIP path: the reference has --ptn_norm for the local embedder only (LocalCloudEmbedder: '
                                      'a stand-alone model.stn and a model.ptn with nfeat_stn = 0)')
        self.__dict__['_gn_spec_cache'] = spec
        return spec

    def _gn_cfg(self, npts):
        n_group, eps = self._gn_spec()
        return ops.make_gn_cfg(self._nfeat, self._nfeat_global, npts, self._nf_conv, self._nf_fc, n_group, eps, self._last_ac)

    def forward(self, input, input_global, bn_update_times=1):
        if not input.is_cuda:
            raise RuntimeError('superpoint_graph_amd.PointNet has no CPU path; move the model and inputs to the GPU')
        if self.training and self._prelast_do > 0:
            raise NotImplementedError('ptn_prelast_do > 0 (dropout before the last layer) is not implemented on the HIP path')
        if self.nfeat_stn > 0 and self.stn._K != 2:
            raise NotImplementedError('the fused STN applies a 2x2 transform (K=2), as PointNet.forward does')
        input, rows = input.contiguous().float(), self._groups_tensors()
        if self._gn_spec() is not None:      # norm = 'layer' | 'group': the cloud-resident kernels (spg_groupnorm.hip)
            return _GroupNormFunction.apply(self, rows, input, input_global, None, *_layers.flat_params(rows))
        self._cfg(input.shape[2])      # (an unsupported npts is refused here, before the batch counters move)
        if self.training:
            self._bump_batches_tracked(bn_update_times)
        return _PointNetFunction.apply(self, rows, input, input_global, None, self.training, bn_update_times,
                                       *_layers.node_inputs(self, rows, input.device))


class LocalCloudEmbedder():
    """Local PointNet of the supervised partition (reference learning/pointnet.py:182-218, used by
    supervized_partition/supervized_partition.py:184,218): millions of k-nearest-neighbour clouds [n, nfeat, k] through a
    stand-alone STN (`model.stn`) and a PointNet built with nfeat_stn = 0 (`model.ptn`), embeddings L2-normalised.  The
    reference chunks the batch for cuDNN (2^16 - 1 clouds per call, :193) and materialises the transformed clouds; here the
    2x2 transform is applied by the first convolution while it stages the cloud.  The kernels have no chunk limit, but the
    reference's chunks are OBSERVABLE in training mode (every chunk is its own BatchNorm batch: own statistics, own
    running-stat update), so training-mode batches above 2^16 - 1 clouds are processed in the same chunks; in eval mode
    (running statistics) the whole batch is one launch sequence.  A GroupNorm / LayerNorm model (--ptn_norm layer|group) has no
    batch statistics: its chunks are unobservable, so the whole batch is one launch sequence in training mode too."""

    CHUNK = 2 ** 16 - 1      # learning/pointnet.py:193

    def __init__(self, args):
        self.nfeat_stn = args.ptn_nfeat_stn
        self.stn_as_global = args.stn_as_global

    def run_batch(self, model, clouds, clouds_global, *excess):
        if not clouds.is_cuda:
            raise RuntimeError('superpoint_graph_amd.LocalCloudEmbedder has no CPU path')
        n = clouds.shape[0]
        if n > self.CHUNK and model.ptn._gn_spec() is None and (model.ptn.training or (self.nfeat_stn > 0 and model.stn.training)):
            # the reference's order: all STN chunks, then all PointNet chunks (:196-198, :204-206); the two networks share no
            # BatchNorm layer, so chunk-by-chunk evaluation of the pair gives the same statistics and updates
            clouds_global = clouds_global.reshape(n, -1)
            return torch.cat([self._run(model, clouds[a:a + self.CHUNK], clouds_global[a:a + self.CHUNK])
                              for a in range(0, n, self.CHUNK)])
        return self._run(model, clouds, clouds_global)

    def _run(self, model, clouds, clouds_global):
        ptn = model.ptn
        if ptn.nfeat_stn > 0:
            raise ValueError('LocalCloudEmbedder expects model.ptn without an inner STN (nfeat_stn = 0) and a separate model.stn')
        clouds = clouds.contiguous().float()
        clouds_global = clouds_global.float().reshape(clouds.shape[0], -1)
        if ptn._gn_spec() is not None:
            return self._run_groupnorm(model, clouds, clouds_global)
        if self.nfeat_stn > 0 and _groupnorm_spec(model.stn) is not None:
            raise NotImplementedError('a mix of BatchNorm and GroupNorm in one model is not implemented on the HIP path '
                                      '(model.stn is GroupNorm, model.ptn is BatchNorm)')
        if self.nfeat_stn > 0:
            T = model.stn(clouds[:, :self.nfeat_stn, :].contiguous())
            if self.stn_as_global:
                clouds_global = torch.cat([clouds_global, T.reshape(-1, 4)], 1)
            if ptn.training:
                ptn._bump_batches_tracked(1)
            rows = ptn._groups_tensors()
            out = _PointNetFunction.apply(ptn, rows, clouds, clouds_global.contiguous(), T, ptn.training, 1,
                                          *_layers.node_inputs(ptn, rows, clouds.device))
        else:
            out = ptn(clouds, clouds_global.contiguous())
        return nn.functional.normalize(out)

    def _run_groupnorm(self, model, clouds, clouds_global):
        """The same composition (learning/pointnet.py:195-207) on the cloud-resident GroupNorm kernels: the transform is applied
        while a cloud is staged, and the gradient flows back into T through the transform and through `stn_as_global`."""
        ptn, T = model.ptn, None
        if ptn.training and ptn._prelast_do > 0:
            raise NotImplementedError('ptn_prelast_do > 0 (dropout before the last layer) is not implemented on the HIP path')
        if self.nfeat_stn > 0:
            # (the two networks may differ in their group count: the reference's create_model hands ptn_n_group to the STN only)
            if _groupnorm_spec(model.stn) is None:
                raise NotImplementedError('a mix of BatchNorm and GroupNorm in one model is not implemented on the HIP path '
                                          '(model.stn is BatchNorm, model.ptn is GroupNorm)')
            if self.nfeat_stn != 2 or model.stn._K != 2:
                raise NotImplementedError('the GroupNorm local embedder applies a 2x2 transform to the xy rows (ptn_nfeat_stn = 2, K = 2)')
            T = model.stn(clouds[:, :2, :].contiguous())
            if self.stn_as_global:
                clouds_global = torch.cat([clouds_global, T.reshape(-1, 4)], 1)
        rows = ptn._groups_tensors()
        out = _GroupNormFunction.apply(ptn, rows, clouds, clouds_global.contiguous(), T, *_layers.flat_params(rows))
        return nn.functional.normalize(out)

    def run_batch_cpu(self, model, clouds, clouds_global, *excess):
        """Embeddings on the host (the reference moves 1023-cloud chunks to the CPU as they are computed to bound GPU
        memory, :207-218); with 288 GB of HBM the whole batch is embedded at once and copied back."""
        return self.run_batch(model, clouds, clouds_global).cpu()


class _ScatterEmbeddings(torch.autograd.Function):
    """descriptors[i] = embeddings[slot[i]] for embeddable superpoints, exact zeros for the others (reference
    learning/pointnet.py:177-179: zero-initialised matrix + index_copy_), one launch each way instead of fill + index_copy_."""

    @staticmethod
    def forward(ctx, out, slot_of_row, idx_valid):
        ctx.idx_valid = idx_valid
        return ops.gather_rows(out.contiguous(), slot_of_row)

    @staticmethod
    def backward(ctx, grad):
        return ops.gather_rows(grad.contiguous(), ctx.idx_valid), None, None


def flag_index_vectors(clouds_flag):
    """HOST index vectors CloudEmbedder derives from `clouds_flag` (learning/pointnet.py:149,162,177-179): rows of the valid
    superpoints, and the embedding row of every superpoint (-1 for the too-small ones) -> (idx_valid, slot_of_row), int64."""
    valid = clouds_flag.eq(0)
    idx_valid = torch.nonzero(valid).reshape(-1)
    slot = torch.cumsum(valid.to(torch.int64), 0) - 1
    slot[~valid] = -1
    return idx_valid, slot


def attach_staged_flags(clouds_flag, idx_valid_dev, slot_dev):
    """The device copies of flag_index_vectors(clouds_flag), uploaded by the caller (a device collate packs them into the batch's one
    staging copy: GraphConvInfo.set_batch_device(extras=...)), attached to the flag tensor for CloudEmbedder."""
    clouds_flag._spg_staged = (idx_valid_dev, slot_dev)
    return clouds_flag._spg_staged


def stage_flags(clouds_flag):
    """Index vectors CloudEmbedder derives from `clouds_flag` (rows of the valid superpoints, embedding row of every
    superpoint), computed and uploaded on the CURRENT stream and attached to the flag tensor: a device collate calls this
    while it builds the batch (on the side stream of learning/prefetch.py), so the training stream starts a step without the
    two small uploads.  -> (idx_valid, slot_of_row) on the device."""
    staged = getattr(clouds_flag, '_spg_staged', None)
    if staged is None:
        dev = torch.device('cuda', torch.cuda.current_device())
        idx_valid, slot = flag_index_vectors(clouds_flag)
        # (staging ring, non-blocking: a pageable H2D would stall the host until the stream has drained)
        if clouds_flag.is_cuda:       # (a flag vector that lives on the device already: its index vectors do too)
            staged = clouds_flag._spg_staged = (idx_valid, slot)
        else:
            staged = clouds_flag._spg_staged = tuple(ops.upload_packed([idx_valid, slot], dev))
    return staged


class CloudEmbedder():
    """Evaluates PointNet on superpoints; too small superpoints get zero embeddings (reference
    learning/pointnet.py:138-180).  `ptn_mem_monger` keeps its observable semantics (autograd is cut after
    the embeddings, `bw_hook()` back-propagates into PointNet, BatchNorm running statistics advance twice
    per step) but nothing is recomputed: the raw layer outputs stay in HBM."""

    def __init__(self, args):
        self.args = args
        self.bw_hook = lambda: None
        self.run = self.run_full_monger if args.ptn_mem_monger else self.run_full
        self._flag_cache = (None, None, None)      # (clouds_flag tensor, idx_valid, slot_of_row on the device)

    def _to_device(self, clouds_flag, clouds, clouds_global):
        dev = torch.device('cuda', torch.cuda.current_device())
        if self._flag_cache[0] is not clouds_flag:       # (same batch object again: benchmarks, multi-pass evaluation)
            self._flag_cache = (clouds_flag,) + tuple(stage_flags(clouds_flag))      # staged by the device collate, or now
        self._slot_of_row = self._flag_cache[2]
        return self._flag_cache[1], ops.upload(clouds, dev), ops.upload(clouds_global, dev)

    def _scatter(self, out, idx_valid, n_rows):
        if out.shape[0] == 0:                          # no embeddable superpoint in the batch
            return out.new_zeros(n_rows, out.size(1))
        return _ScatterEmbeddings.apply(out, self._slot_of_row, idx_valid)

    def run_full(self, model, clouds_meta, clouds_flag, clouds, clouds_global):
        if not self.args.cuda:
            raise RuntimeError('superpoint_graph_amd has no CPU path (--cuda 1 required)')
        idx_valid, clouds, clouds_global = self._to_device(clouds_flag, clouds, clouds_global)
        out = model.ptn(clouds, clouds_global)
        return self._scatter(out, idx_valid, clouds_flag.size(0))

    def run_full_monger(self, model, clouds_meta, clouds_flag, clouds, clouds_global):
        if not self.args.cuda:
            raise RuntimeError('superpoint_graph_amd has no CPU path (--cuda 1 required)')
        idx_valid, clouds, clouds_global = self._to_device(clouds_flag, clouds, clouds_global)
        ptn = model.ptn
        if not model.training:
            with torch.no_grad():
                out = ptn(clouds, clouds_global)
            self.bw_hook = lambda: None
        else:
            # one forward that keeps its activations; the running statistics advance as in the reference's
            # forward + re-forward (learning/pointnet.py:167,173)
            live = ptn(clouds, clouds_global, bn_update_times=2)
            out = live.detach().requires_grad_(True)

            def bw_hook():
                if out.grad is not None:
                    live.backward(out.grad)
            self.bw_hook = bw_hook
        return self._scatter(out, idx_valid, clouds_flag.size(0))
