"""Drop-in for the reference's ``passiveRadar/plotting_tools.py``: ``persistence`` (the digital-phosphor sum that
simple_kalman_tracker.py and range_doppler_plot.py apply to every frame they render), on the device, plus
``persistence_stack``, every frame of that render loop in one launch.  Rendering itself (matplotlib) is not here."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, lib

__all__ = ["persistence", "persistence_stack"]


def _weak_scalar(decay):
    """NumPy >= 2 (NEP 50): a Python float / int is 'weak', so X[..., k-i] * decay**i stays float32 for a float32 X;
    a NumPy scalar (np.float64 included, although it subclasses float) is not"""
    return type(decay) in (float, int)


def _in_dtype(x_dtype, decay):
    """the device input dtype: float32 only when the reference would form float32 products"""
    return np.float32 if (x_dtype == np.float32 and _weak_scalar(decay)) else np.float64


def _check_k(k, hold, L):
    if hold > 0 and k >= L:
        raise IndexError(f"index {k} is out of bounds for axis 2 with size {L}")


def _run(frames_ptr, in_code, elems, nframes, k_first, k_count, hold, decay, out_ptr, out_code, stream):
    check(lib().prc_persistence(frames_ptr, in_code, int(elems), int(nframes), int(k_first), int(k_count), int(hold),
                                float(decay), out_ptr, out_code, stream))


def persistence(X, k, hold, decay):
    """persistence (plotting_tools.py): sum_{i < min(k+1, hold)} X[:, :, k-i] * decay**i, bitwise as the reference.
    ``X`` is numpy (H, W, L) -- only the frames the sum reads are uploaded -- and the result numpy (H, W) float64; or a
    torch device tensor [L, H, W], and the result a device [H, W] float64.  k < 0 or hold <= 0 give zeros; otherwise
    k >= L raises IndexError, as the reference's first read X[:, :, k] does."""
    k, hold = int(k), int(hold)
    if _lib.is_device_tensor(X):
        import torch
        if X.dim() != 3:
            raise ValueError("persistence takes a device stack [L, H, W]")
        want = torch.float32 if (X.dtype == torch.float32 and _weak_scalar(decay)) else torch.float64
        x = X.to(want).contiguous()
        L, H, W = x.shape
        _check_k(k, hold, L)
        out = torch.empty((H, W), dtype=torch.float64, device=x.device)
        code = _lib.REAL_F32 if want == torch.float32 else _lib.REAL_F64
        with torch.cuda.device(x.device):
            _run(x.data_ptr(), code, H * W, L, k, 1, hold, decay, out.data_ptr(), _lib.REAL_F64,
                 _lib.torch_stream_ptr(x.device))
        return out
    x = np.asarray(X)
    if x.ndim != 3:
        raise ValueError("persistence takes an (H, W, L) stack")
    H, W, L = x.shape
    _check_k(k, hold, L)
    n = max(0, min(k + 1, hold))
    dt = _in_dtype(x.dtype, decay)
    f = np.ascontiguousarray(np.moveaxis(x[:, :, k - n + 1:k + 1] if n else x[:, :, :0], 2, 0), dtype=dt)
    _lib.require_gpu()
    dx = _lib.DeviceBuffer(f.nbytes)
    if n:
        dx.upload(f)
    do = _lib.DeviceBuffer(H * W * 8)
    # the n frames read sit at 0 .. n-1; relative to them the frame asked for is n-1 (k < 0 or hold <= 0: none, zeros)
    _run(dx.ptr, _lib.REAL_F32 if dt == np.float32 else _lib.REAL_F64, H * W, n, n - 1, 1, n if n else hold, decay,
         do.ptr, _lib.REAL_F64, None)
    return do.download((H, W), np.float64)


def persistence_stack(X, hold, decay, out_dtype=np.float64):
    """persistence(X, k, hold, decay) for every k in one launch -- what the render loops of simple_kalman_tracker.py and
    range_doppler_plot.py compute frame by frame.  numpy (H, W, L) gives numpy (H, W, L); a torch device tensor
    [L, H, W] gives a device [L, H, W].  ``out_dtype`` float64 (bitwise the reference) or float32 (the float64 sum
    rounded once, for display)."""
    hold = int(hold)
    f32_out = np.dtype(out_dtype) == np.float32
    if not f32_out and np.dtype(out_dtype) != np.float64:
        raise ValueError("persistence_stack: out_dtype is float64 or float32")
    if _lib.is_device_tensor(X):
        import torch
        if X.dim() != 3:
            raise ValueError("persistence_stack takes a device stack [L, H, W]")
        want = torch.float32 if (X.dtype == torch.float32 and _weak_scalar(decay)) else torch.float64
        x = X.to(want).contiguous()
        L, H, W = x.shape
        # a float32 out holds at most PERSISTENCE_TERMS_PER_LAUNCH terms (the launches chain through a float64 out)
        narrow = f32_out and min(hold, L) > _lib.PERSISTENCE_TERMS_PER_LAUNCH
        out = torch.empty((L, H, W), dtype=torch.float32 if f32_out and not narrow else torch.float64, device=x.device)
        code = _lib.REAL_F32 if want == torch.float32 else _lib.REAL_F64
        with torch.cuda.device(x.device):
            _run(x.data_ptr(), code, H * W, L, 0, L, hold, decay, out.data_ptr(),
                 _lib.REAL_F32 if out.dtype == torch.float32 else _lib.REAL_F64, _lib.torch_stream_ptr(x.device))
        return out.to(torch.float32) if narrow else out
    x = np.asarray(X)
    if x.ndim != 3:
        raise ValueError("persistence_stack takes an (H, W, L) stack")
    H, W, L = x.shape
    dt = _in_dtype(x.dtype, decay)
    f = np.ascontiguousarray(np.moveaxis(x, 2, 0), dtype=dt)
    _lib.require_gpu()
    narrow = f32_out and min(hold, L) > _lib.PERSISTENCE_TERMS_PER_LAUNCH
    odt = np.float32 if f32_out and not narrow else np.float64
    dx = _lib.DeviceBuffer(f.nbytes)
    dx.upload(f)
    do = _lib.DeviceBuffer(L * H * W * np.dtype(odt).itemsize)
    _run(dx.ptr, _lib.REAL_F32 if dt == np.float32 else _lib.REAL_F64, H * W, L, 0, L, hold, decay, do.ptr,
         _lib.REAL_F32 if odt == np.float32 else _lib.REAL_F64, None)
    out = np.moveaxis(do.download((L, H, W), odt), 0, 2)
    return out.astype(np.float32) if narrow else out
