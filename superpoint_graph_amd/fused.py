"""FusedStep: forward + backward of one training step as ONE call into libspg_hip (include/spg_hip.h: spg_train_step).

The reference's loop body (learning/main.py:199-208)
    embeddings = ptnCloudEmbedder.run(model, *clouds_data); outputs = model.ecc(embeddings)
    loss = cross_entropy(outputs, label_mode, weight=class_weights); loss.backward(); ptnCloudEmbedder.bw_hook()
costs ~15 autograd nodes / ctypes calls and, on the device, orders the filter network's forward in front of the recurrence
and the tail of the RNN-ECC backward in front of PointNet's backward although neither depends on PointNet.  For the standard
model -- `gru_R...` / `lstm_R...` followed by `f_K` (every documented configuration) -- with its parameters in a
FlatParameters arena this object issues the same kernels through one C call that knows the whole step (the two chains travel
next to PointNet's launches, superpoint_graph_amd/csrc/spg_step.hip).  For GRU models the classifier and the cross entropy
run inside the one-launch recurrence (per node, in the wavefront that owns it).  Results are those of the
module-level path: tests/test_gpu_fused.py compares loss, logits, every gradient and the BatchNorm statistics bit for bit with
the classifier / loss as separate launches (spg_tune key 15 = 1) and at fp32 round-off in the default form.

What it keeps of the module API's observable behaviour: BatchNorm batch counters advance (twice for PointNet with
`ptn_mem_monger`, like the reference's forward + re-forward), too-small superpoints get exact-zero descriptors, the gradients
land in `p.grad` (the arena), `arena.zero_grad()` / `optimizer_step()` work as before.  What it does not do: autograd -- the
returned loss / logits are detached; anything outside `supports(model)` must use the modules."""
from __future__ import annotations

import ctypes
import types

import torch

from . import _lib, ops
from .flat import mark_direct_write
from .learning._layers import advance_batch_counters, grad_targets
from .learning.modules import HipLinear, RNNGraphConvModule
from .learning.pointnet import PointNet, stage_flags
from .ops._core import _ptr_array, _req, _stream
from .ops.model import rows6


def _workspaces(dev, *sizes):
    """One uint8 tensor per workspace query of the library (0: the query failed)."""
    if min(sizes) == 0:
        raise RuntimeError('workspace query failed: ' + _lib.lib().spg_last_error().decode())
    return [torch.empty(max(int(n), 256), dtype=torch.uint8, device=dev) for n in sizes]


def supports(model) -> bool:
    """True for `model.ptn` = PointNet (inner STN or none) and `model.ecc` = GraphNetwork of exactly one recurrent graph
    convolution followed by one linear layer that the HIP kernels serve."""
    ptn, ecc = getattr(model, 'ptn', None), getattr(model, 'ecc', None)
    if not isinstance(ptn, PointNet) or ecc is None:
        return False
    kids = list(ecc.children())
    if len(kids) != 2 or not isinstance(kids[0], RNNGraphConvModule) or not isinstance(kids[1], HipLinear):
        return False
    conv, fc = kids
    if conv._cell.hidden_size != 32 or conv._cell.input_size != 32 or conv._cell.bias_ih is None:
        return False
    return fc._kernel_shape_ok() and ptn._prelast_do == 0 and (ptn.nfeat_stn == 0 or ptn.stn._K == 2)


class FusedStep:
    def __init__(self, model, arena, class_weights=None, reduction='mean', ignore_index=-100, ptn_mem_monger=True):
        if not supports(model):
            raise NotImplementedError('FusedStep serves PointNet + GraphNetwork("gru_R.../lstm_R...,f_K") only')
        if arena is None or arena.model is not model:
            raise ValueError('FusedStep needs the FlatParameters arena of this model (the kernels write the gradients in place)')
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError("reduction must be 'mean' or 'sum'")
        self.model, self.arena = model, arena
        self.ptn = model.ptn
        self.conv, self.fc = list(model.ecc.children())
        # (validated like every other device operand: a CPU / other-GPU tensor here would reach the kernels as a wild pointer)
        self.class_weights = None if class_weights is None else _req(class_weights.detach().float().contiguous(), torch.float32, 'class_weights')
        if self.class_weights is not None and self.class_weights.numel() != list(model.ecc.children())[1].out_features:
            raise ValueError('class_weights: one weight per class expected')
        self.mean = reduction == 'mean'
        self.ignore_index = int(ignore_index)
        self.bn_times = 2 if ptn_mem_monger else 1
        self._plan = None
        self._bufs = {}

    # ---- parameter / gradient pointer tables: the arena's views never move ----
    def _tables(self, npts):
        if self._plan is not None and self._plan['npts'] == npts:
            return self._plan
        ptn_cfg = self.ptn._cfg(npts)
        ecc_cfg, ecc_rows = self.conv._cfg_and_groups()
        tables = []      # parameters and gradient targets of PointNet, then of the RNN-ECC module: six pointers per row
        for rows in (self.ptn._groups_tensors(), ecc_rows):
            tables += [[t for r in rows for t in r], [t for r in rows6(grad_targets(rows, strict=True)) for t in r]]
        self._plan = dict(npts=npts, ptn_cfg=ptn_cfg, ecc_cfg=ecc_cfg,
                          ptn_params=_ptr_array(tables[0]), ptn_grads=_ptr_array(tables[1]),
                          ecc_params=_ptr_array(tables[2]), ecc_grads=_ptr_array(tables[3]),
                          keep=tables, nf=int(ptn_cfg.fc[ptn_cfg.n_fc - 1]),
                          nout=int(ecc_cfg.nc * (ecc_cfg.nrepeats + 1) if ecc_cfg.cat_all else ecc_cfg.nc))
        return self._plan

    def _buffers(self, key, make):
        """Workspaces and activations of one step, re-used from step to step while the sizes stay the same (one stream: the
        next step overwrites them only after this one has consumed them)."""
        b = self._bufs.get(key)
        if b is None:
            b = make()
            if len(self._bufs) >= 4:       # a few batch shapes at most stay cached (training batches vary in size)
                self._bufs.pop(next(iter(self._bufs)))
            self._bufs[key] = b
        return b

    def _stage(self, training, clouds_flag, clouds, clouds_global, gc_info, buffers):
        """Stages and validates the inputs of a step and fills the StepArgs fields that training and inference share.
        buffers(s, pc, ec) -> the step's cached buffers.  -> (StepArgs, s): `s` holds what the caller still needs, and every
        tensor the library call reads -- it must stay alive until that call has been enqueued."""
        conv, fc = self.conv, self.fc
        s = types.SimpleNamespace(dev=torch.device('cuda', torch.cuda.current_device()))
        s.idx_valid, s.slot_of_row = stage_flags(clouds_flag)
        clouds = ops.upload(clouds, s.dev) if not clouds.is_cuda else clouds
        clouds_global = ops.upload(clouds_global, s.dev) if not clouds_global.is_cuda else clouds_global
        s.clouds = clouds = _req(clouds.contiguous(), torch.float32, 'clouds')
        s.B, s.N = B, N = int(clouds.shape[0]), int(clouds_flag.shape[0])
        if training and B <= 1:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size [{B}, C]')
        if B < 1:
            raise ValueError('no embeddable superpoint in the batch')
        s.plan = plan = self._tables(int(clouds.shape[2]))
        if clouds.shape[1] != plan['ptn_cfg'].nfeat:
            raise ValueError('clouds: wrong number of point features')
        s.clouds_global = clouds_global = _req(clouds_global.reshape(B, -1).contiguous(), torch.float32, 'clouds_global')
        idxn, idxe, degs, degs_gpu, edgefeats = gc_info.get_buffers()
        if idxe is not None:
            raise NotImplementedError('filter sharing (idxe) is not supported by the fused RNN-ECC path')
        s.graph = graph = gc_info.device_graph()
        s.E = E = int(graph.E)
        if graph.N != N:
            raise ValueError(f'the batched graph has {graph.N} nodes, clouds_flag has {N} rows')
        s.edgefeats = edgefeats = _req(edgefeats.contiguous().float(), torch.float32, 'edgefeats')
        if training and plan['ecc_cfg'].bnidx >= 0 and E == 1:
            raise ValueError('Expected more than 1 value per channel when training (filter-network BatchNorm over one edge)')
        s.ecc_cfg = conv._cfg_for(plan['ecc_cfg'], gc_info, N)      # (+ the batch's scene boundaries for graphs above one round)
        s.bufs = b = buffers(s, ctypes.byref(plan['ptn_cfg']), ctypes.byref(s.ecc_cfg))
        s.logits = torch.empty(N, fc.out_features, dtype=torch.float32, device=s.dev)
        a = _lib.StepArgs()
        a.ptn_cfg, a.B = ctypes.pointer(plan['ptn_cfg']), B
        a.clouds, a.clouds_global = clouds.data_ptr(), clouds_global.data_ptr()
        a.ptn_params, a.ptn_ws, a.emb = plan['ptn_params'], b['ptn_ws'].data_ptr(), b['emb'].data_ptr()
        a.N, a.nf = N, plan['nf']
        a.slot_of_row, a.idx_valid, a.desc = s.slot_of_row.data_ptr(), s.idx_valid.data_ptr(), b['desc'].data_ptr()
        a.ecc_cfg, a.E, a.graph_ws = ctypes.pointer(s.ecc_cfg), E, graph.ws.data_ptr()
        a.edgefeats = edgefeats.data_ptr() if E else None
        a.ecc_params, a.ecc_ws, a.ecc_out = plan['ecc_params'], b['ecc_ws'].data_ptr(), b['ecc_out'].data_ptr()
        a.nout, a.n_classes = plan['nout'], fc.out_features
        a.cls_W, a.cls_b, a.logits = fc.weight.data_ptr(), None if fc.bias is None else fc.bias.data_ptr(), s.logits.data_ptr()
        return a, s

    def __call__(self, clouds_flag, clouds, clouds_global, gc_info, target):
        """-> (loss [] float32, logits [N, n_classes]) on the device, detached; gradients in the arena.
        clouds_flag / clouds / clouds_global: as CloudEmbedder.run takes them; gc_info: the batch's GraphConvInfo (already on
        the device: GraphNetwork.set_info(..., cuda=True) or set_batch_device); target: int64 [N] device tensor."""
        ptn, conv, fc = self.ptn, self.conv, self.fc
        if not (ptn.training and conv.training):
            raise RuntimeError('FusedStep is a TRAINING step (model.train()); evaluate through the modules')

        def buffers(s, pc, ec):
            # (npts: the PointNet plan -- hence the workspace layout and the statistics slots -- depends on the points per cloud)
            B, N, E, ecc_cfg = s.B, s.N, s.E, s.ecc_cfg
            key = (B, N, E, s.dev, s.plan['npts'], tuple(ecc_cfg.part_ptr[:ecc_cfg.n_parts + 1]) if ecc_cfg.n_parts > 0 else ())

            def make():
                L, nf, nout, C = _lib.lib(), s.plan['nf'], s.plan['nout'], fc.out_features
                ws = _workspaces(s.dev, L.spg_pointnet_workspace_bytes(pc, B, 1), L.spg_pointnet_bwd_workspace_bytes(pc, B),
                                 L.spg_eccrnn_workspace_bytes(ec, N, E, 1), L.spg_eccrnn_bwd_workspace_bytes(ec, N, E))
                f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=s.dev)
                return dict(ptn_ws=ws[0], ptn_bwd_ws=ws[1], ecc_ws=ws[2], ecc_bwd_ws=ws[3], emb=f32(B, nf), grad_emb=f32(B, nf),
                            desc=f32(N, nf), grad_desc=f32(N, nf), ecc_out=f32(N, nout), grad_ecc_out=f32(N, nout),
                            cls_work=f32(max(1, L.spg_linear_wgrad_bias_work_floats(N, C, nout))), grad_logits=f32(N, C))
            return self._buffers(key, make)
        a, s = self._stage(True, clouds_flag, clouds, clouds_global, gc_info, buffers)
        b, N = s.bufs, s.N
        target = _req(target.contiguous(), torch.int64, 'target')
        loss_buf = torch.empty(N + 2, dtype=torch.float32, device=s.dev)
        a.bn_update_times = self.bn_times
        a.ptn_grads, a.ptn_bwd_ws, a.grad_emb = s.plan['ptn_grads'], b['ptn_bwd_ws'].data_ptr(), b['grad_emb'].data_ptr()
        a.grad_desc = b['grad_desc'].data_ptr()
        a.ecc_grads, a.ecc_bwd_ws, a.grad_ecc_out = s.plan['ecc_grads'], b['ecc_bwd_ws'].data_ptr(), b['grad_ecc_out'].data_ptr()
        if fc.weight.grad is None or not fc.weight.grad.is_contiguous() or (fc.bias is not None and fc.bias.grad is None):
            raise RuntimeError('FusedStep: the classifier has no contiguous .grad view into the gradient arena')
        a.cls_dW, a.cls_db = fc.weight.grad.data_ptr(), None if fc.bias is None else fc.bias.grad.data_ptr()
        a.cls_work, a.grad_logits = b['cls_work'].data_ptr(), b['grad_logits'].data_ptr()
        a.target = target.data_ptr()
        a.class_weight = None if self.class_weights is None else self.class_weights.data_ptr()
        a.ignore_index, a.reduction_mean, a.loss_buf = self.ignore_index, int(self.mean), loss_buf.data_ptr()
        # the statistics slots inside ptn_ws are zero after every successful step on these buffers (include/spg_hip.h)
        a.ptn_slots_clean = 1 if b.get('slots_clean') else 0
        b['slots_clean'] = False
        _lib.check(_lib.lib().spg_train_step(ctypes.byref(a), _stream()), 'spg_train_step')
        b['slots_clean'] = True
        # module-level bookkeeping the C call does not do -- only once the call has succeeded (a refused step must not advance
        # the BatchNorm batch counters or mark gradients as written)
        advance_batch_counters(ptn, self.bn_times)
        advance_batch_counters(conv._fnet)
        for m in (ptn, conv, fc):
            mark_direct_write(m)
        self._last = (s.plan['ptn_cfg'], s.B, b['ptn_ws'], s.ecc_cfg, s.graph, b['ecc_ws'], s.edgefeats)
        self.normaliser = loss_buf[N + 1:N + 2]       # sum of the labelled rows' class weights (data-parallel loss weight w_r)
        self._emb, self._slot = b['emb'], s.slot_of_row   # (the descriptors are read in place by the recurrence: see `embeddings`)
        return loss_buf[N], s.logits

    def infer(self, clouds_flag, clouds, clouds_global, gc_info):
        """-> logits [N, n_classes] of the model in EVALUATION mode (model.eval(): BatchNorm running statistics), the body of
        the evaluation loop (learning/main.py:256-262) as ONE library call (spg_infer_step); same kernels and results as
        `model.ecc(CloudEmbedder.run(...))` under torch.no_grad()."""
        if self.ptn.training or self.conv.training:
            raise RuntimeError('FusedStep.infer is the EVALUATION forward (model.eval()); train with __call__')

        def buffers(s, pc, ec):
            B, N, E = s.B, s.N, s.E

            def make():
                L, nf = _lib.lib(), s.plan['nf']
                ws = _workspaces(s.dev, L.spg_pointnet_workspace_bytes(pc, B, 0), L.spg_eccrnn_workspace_bytes(ec, N, E, 0))
                f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=s.dev)
                return dict(ptn_ws=ws[0], ecc_ws=ws[1], emb=f32(B, nf), desc=f32(N, nf), ecc_out=f32(N, s.plan['nout']))
            return self._buffers(('infer', B, N, E, s.dev), make)
        a, s = self._stage(False, clouds_flag, clouds, clouds_global, gc_info, buffers)
        a.bn_update_times = 1
        _lib.check(_lib.lib().spg_infer_step(ctypes.byref(a), _stream()), 'spg_infer_step')
        return s.logits

    def debug_states(self):
        """(PointNetState, EccRnnState) views of the LAST training step's forward workspaces -- what ops.pointnet_forward /
        ops.eccrnn_forward return on the module path; the parity tests read the kernels' ReLU / max-pool decisions out of them
        (spg_pointnet_debug_offset / spg_eccrnn_debug_offset).  Valid until the next step on the same buffers."""
        ptn_cfg, B, ptn_ws, ecc_cfg, graph, ecc_ws, edgefeats = self._last
        return (ops.PointNetState(ptn_cfg, B, None, None, ptn_ws, True), ops.EccRnnState(ecc_cfg, graph, edgefeats, ecc_ws, True))

    @property
    def embeddings(self):
        """[N, nf] superpoint descriptors of the last step (CloudEmbedder.run's return value: PointNet embeddings scattered to all
        superpoints, zero rows for the too-small ones) -- built on request: the step itself never materialises them when the
        one-launch recurrence reads the scatter in place."""
        return ops.gather_rows(self._emb, self._slot)
