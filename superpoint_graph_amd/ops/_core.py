"""What every module of the package shares: stream and pointer plumbing, the argument checkers, the uint8 workspace and the
host -> device staging ring (spg_upload / spg_upload_packed of csrc/spg_batch.hip)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from .._lib import check, lib


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


def _workspace(query, *dims, dev):
    """The uint8 buffer that a spg_*_workspace_bytes query of the library asks for at these dimensions (never empty: 256 bytes at least)."""
    return torch.empty(max(int(query(*dims)), 256), dtype=torch.uint8, device=dev)


def _raise_flagged(word, table):
    """word: an error word of a kernel, already on the host; table: {bit: (exception type, message)} in the order the bits are tested.
    Raises what the first set bit stands for."""
    for bit, (exc, message) in table.items():
        if word & bit:
            raise exc(message)


_NONFINITE = 1      # bit 0 of the error word of every scene op (and of cut_pursuit's host-side finite check)


def _raise_nonfinite(word):
    """sklearn's message for a coordinate that is NaN or infinite"""
    _raise_flagged(word, {_NONFINITE: (ValueError, 'Input contains NaN or infinity.')})


# --------------------------------------------------------------------------------------------------
# argument checkers
# --------------------------------------------------------------------------------------------------
def _checked(t, shape, name, dtype_ok=None, wanted=None):
    """The one device / dtype class / shape test behind the checkers below, in this order: RuntimeError off the GPU, TypeError for a
    dtype that dtype_ok refuses (`wanted` names what it takes), ValueError for another shape."""
    _on_gpu(t, name)
    if dtype_ok is not None and not dtype_ok(t.dtype):
        raise TypeError(f'{name} must be {wanted}, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must be {list(shape)}, got {tuple(t.shape)}')
    return t


def _as_vec(t, dtype, n, name):
    """Any device tensor converted to contiguous `dtype`, then required to be [n]."""
    return _checked(_req(t.contiguous() if t.dtype == dtype else t.to(dtype).contiguous(), dtype, name), (n,), name)


def _int_vec(t, n, dtype, name):
    """An integer [n] device tensor as contiguous `dtype` (int32: the values must fit, ids and labels below 2^31)."""
    _checked(t, (n,), name, lambda d: not (d.is_floating_point or d == torch.bool), 'an integer tensor')
    return _req(t.to(dtype).contiguous(), dtype, name)


def _indicator(t, E, name):
    """A bool / uint8 [E] device tensor as contiguous uint8 (bool is reinterpreted, not copied)."""
    t = _checked(t, (E,), name, lambda d: d in (torch.bool, torch.uint8), 'bool or uint8').contiguous()
    return _req(t.view(torch.uint8) if t.dtype == torch.bool else t, torch.uint8, name)


def _scene_array(t, shape, name):
    """A float32 device tensor of exactly this shape, made contiguous."""
    return _req(_checked(t, shape, name).contiguous(), torch.float32, name)


def _scene_xyz(xyz, who):
    """xyz as every scene op takes it: float32 [n, 3] on the device, n >= 1 -> n"""
    _req(xyz, torch.float32, 'xyz')
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f'{who}: xyz must be [n, 3] with n >= 1, got {tuple(xyz.shape)}')
    return int(xyz.shape[0])


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
