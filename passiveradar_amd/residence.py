"""Where a drop-in's data lives.  A front door decides once -- ``side = residence.of(X)`` -- and is
then written once: ``put`` / ``empty`` / ``scratch``, one launch on ``side.stream`` under ``with side.device():``,
``result``.

TorchSide: the caller's device tensors, zero copy, torch's allocator and torch's current stream on the tensor's device.
HostSide: NumPy arrays staged through _lib.DeviceBuffer on the null stream; ``pooled=True`` takes the buffers from
engine.staging() under the names given (grow-only, reused, per thread and device), ``pooled=False`` makes a fresh buffer per
name and holds it until the side dies -- what a chain wants, whose stages stay alive while inner calls use the pool.

A handle has ``.ptr`` and ``.nbytes`` and keeps its memory alive: a DeviceBuffer on the host side, a tensor's wrapper
(``.t``) on the torch side.  engine._ptr takes either.  ``side.torch`` is for the conventions at the edges only (what
comes back, which axis order a stack arrives in): never around an allocation or a launch."""
from __future__ import annotations

import contextlib
import math

import numpy as np

from . import _lib, engine
from ._lib import check, lib

_torch_dtypes = {}


def _torch_dtype(dtype):
    """torch's dtype of a NumPy dtype (they share their names)"""
    t = _torch_dtypes.get(dtype)
    if t is None:
        import torch
        t = _torch_dtypes[dtype] = getattr(torch, np.dtype(dtype).name)
    return t


def of(x, *others, pooled=True, mixed="arguments are all NumPy arrays or all device tensors"):
    """the side ``x`` lives on; ``others`` (None entries skipped) must live there too, else ValueError(``mixed``)"""
    dev = _lib.is_device_tensor(x)
    if others and any(o is not None and _lib.is_device_tensor(o) != dev for o in others):
        raise ValueError(mixed)
    return TorchSide(x.device) if dev else HostSide(pooled)


def shape(x):
    """the shape of an array, a tensor or a nested list as a tuple"""
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def dtype_name(x):
    """"float32", "complex64", ... of an array or a tensor"""
    return str(x.dtype).rsplit(".", 1)[-1]


def iscomplex(x):
    """np.iscomplexobj for arrays and tensors alike"""
    return x.is_complex() if hasattr(x, "is_complex") else np.iscomplexobj(x)


class _Side:
    def fetch(self, handle, shape, dtype):
        """a host copy, whatever the side: counts, info words, records"""
        out = np.empty(shape, dtype=dtype)
        check(lib().prc_memcpy_d2h(out.ctypes.data, handle.ptr, out.nbytes, self.stream))
        check(lib().prc_stream_sync(self.stream))
        return out

    def zero(self, handle, nbytes):
        check(lib().prc_memset(handle.ptr, 0, nbytes, self.stream))


class _TorchBuf:
    """a tensor as a handle"""
    __slots__ = ("t", "ptr")

    def __init__(self, t):
        self.t, self.ptr = t, t.data_ptr()

    @property
    def nbytes(self):
        return self.t.numel() * self.t.element_size()


class TorchSide(_Side):
    torch = True

    def __init__(self, device):
        import torch
        self._torch, self._device = torch, device
        self.stream = _lib.torch_stream_ptr(device)

    def device(self):
        return self._torch.cuda.device(self._device)

    def put(self, name, x, dtype):
        if isinstance(x, np.ndarray):
            x = self._torch.from_numpy(x)
        return _TorchBuf(x.to(device=self._device, dtype=_torch_dtype(dtype)).contiguous())

    def empty(self, name, shape, dtype):
        return _TorchBuf(self._torch.empty(shape, dtype=_torch_dtype(dtype), device=self._device))

    def scratch(self, name, nbytes):
        return self.empty(name, (int(nbytes),), np.uint8) if nbytes else None

    def result(self, handle, shape, dtype):
        return handle.t

    def nothing(self, shape, dtype):
        return self._torch.empty(shape, dtype=_torch_dtype(dtype), device=self._device)


class _Fresh:
    """engine.Staging's get() without the reuse: a new buffer per request, the latest of each name held"""

    def __init__(self):
        self.bufs = {}

    def get(self, name, nbytes):
        b = self.bufs[name] = _lib.DeviceBuffer(nbytes)
        return b


_NO_DEVICE = contextlib.nullcontext()
_itemsize = {}


class HostSide(_Side):
    torch = False
    stream = None
    _bufs = None                            # None until the first buffer: host checks run before a device is touched

    def __init__(self, pooled=True):
        self.pooled = pooled

    def device(self):
        return _NO_DEVICE

    def _open(self):
        _lib.require_gpu()
        self._bufs = engine.staging() if self.pooled else _Fresh()
        return self._bufs

    def put(self, name, x, dtype):
        a = np.ascontiguousarray(x, dtype=dtype)
        b = (self._bufs or self._open()).get(name, a.nbytes)
        if a.nbytes:                        # DeviceBuffer.upload without its second look at the array
            check(lib().prc_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes, None))
            check(lib().prc_stream_sync(None))
        return b

    def empty(self, name, shape, dtype):
        size = _itemsize.get(dtype) or _itemsize.setdefault(dtype, np.dtype(dtype).itemsize)
        return (self._bufs or self._open()).get(name, math.prod(shape) * size)

    def scratch(self, name, nbytes):
        return (self._bufs or self._open()).get(name, int(nbytes)) if nbytes else None

    result = _Side.fetch                    # a download on the null stream

    def nothing(self, shape, dtype):
        """the result of an empty input (a zero in ``shape``): no device is asked for it"""
        return np.zeros(shape, dtype=dtype)
