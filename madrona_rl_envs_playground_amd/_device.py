"""The bottom layer under ``simulators``: torch's current stream as a raw handle, the tensors a simulator exports, and the
checks of the tensors a caller hands in.  Every name here is also ``simulators``'.

May import: _lib, torch.
"""
import ctypes

import torch

from . import _lib
from ._lib import MrlError


# The raw handle of torch's current stream on a device.  ``torch.cuda.current_stream(d).cuda_stream`` builds a Stream
# object on every call (1.1 us measured, a fifth of a step call's host cost -- small batches are bound by that cost,
# tools/host_overhead.py); torch's own raw getter returns the same pointer as an int.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device_index):
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


_TORCH_DTYPE = {
    _lib.MRL_INT8: (torch.int8, "|i1", 1),
    _lib.MRL_UINT8: (torch.uint8, "|u1", 1),
    _lib.MRL_INT32: (torch.int32, "<i4", 4),
    _lib.MRL_FLOAT32: (torch.float32, "<f4", 4),
    _lib.MRL_UINT32: (torch.int32, "<i4", 4),  # torch has no general uint32; same bits
    _lib.MRL_FLOAT64: (torch.float64, "<f8", 8),
}


class _DeviceBlob:
    """Carrier for ``__cuda_array_interface__``; keeps the simulator alive."""

    def __init__(self, owner, ptr, shape, strides_bytes, typestr):
        self._owner = owner
        self.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
            "strides": tuple(strides_bytes),
        }


class Tensor:
    """What ``sim.*_tensor()`` returns (stands in for ``madrona::py::Tensor``)."""

    def __init__(self, sim, slot):
        desc = _lib.TensorDesc()
        _lib.check(_lib.lib().mrl_tensor(sim._handle, slot, ctypes.byref(desc)))
        self._sim = sim
        self.ptr = desc.data
        self.dtype_code = desc.dtype
        self.shape = tuple(desc.shape[i] for i in range(desc.ndim))
        self.strides = tuple(desc.strides[i] for i in range(desc.ndim))
        self.device = desc.device
        self._torch = None

    def to_torch(self):
        if self._torch is None:
            dtype, typestr, size = _TORCH_DTYPE[self.dtype_code]
            blob = _DeviceBlob(self._sim, self.ptr, self.shape, [s * size for s in self.strides], typestr)
            t = torch.as_tensor(blob, device=torch.device("cuda", self.device))
            if t.dtype != dtype:
                t = t.view(dtype)
            if t.data_ptr() != self.ptr:
                raise MrlError("torch.as_tensor copied the exported buffer instead of aliasing it")
            self._torch = t
        return self._torch


def _seat_mask(players, num_players):
    """``players`` (None: every seat; a bit mask; an iterable of seats) as the C ABI's mask"""
    mask = (1 << num_players) - 1 if players is None else players
    if not isinstance(mask, int):
        mask = sum(1 << int(seat) for seat in mask)
    return mask & 0xFFFFFFFF if 0 <= mask < 2 ** 32 else 0xFFFFFFFF


def _check_ids(sim, tensor, shape, name):
    if (not isinstance(tensor, torch.Tensor) or not tensor.is_cuda or tensor.device.index != sim.gpu_id or tensor.dtype != torch.int32 or
            tuple(tensor.shape) != tuple(shape) or not tensor.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 tensor of shape {tuple(shape)} on cuda:{sim.gpu_id}")


def _require_tensors(wanted, device):
    """``wanted``: (name, tensor, dtype, number of elements or None) each; raises unless every one is such a contiguous tensor on
    ``device``."""
    for name, tensor, dtype, numel in wanted:
        if (not isinstance(tensor, torch.Tensor) or tensor.device != device or tensor.dtype != dtype or not tensor.is_contiguous() or
                (numel is not None and tensor.numel() != numel)):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on {device}" + (f" of {numel} elements" if numel else ""))
