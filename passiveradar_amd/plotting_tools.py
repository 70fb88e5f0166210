"""Drop-in for the reference's ``passiveRadar/plotting_tools.py``: ``persistence`` (the digital-phosphor sum that
simple_kalman_tracker.py and range_doppler_plot.py apply to every frame they render), on the device, plus
``persistence_stack``, every frame of that render loop in one launch, and the rest of that loop's arithmetic:
``display_limits`` (the two ``np.percentile`` calls per frame), ``render_frames`` (``imshow``'s Normalize and colour map,
one RGBA8 pixel per cell, bit for bit what matplotlib computes) and ``render_maps`` (the whole chain from the complex
maps).  Figure decoration (axes, labels, dpi, the tracker overlay, imshow's resampling onto figure pixels) is
matplotlib's business and is not here."""
from __future__ import annotations

import numpy as np

from . import _lib, residence
from ._lib import check, lib

__all__ = ["persistence", "persistence_stack", "gnuplot2_lut", "display_limits", "render_frames", "render_maps"]


def _weak_scalar(decay):
    """NumPy >= 2 (NEP 50): a Python float / int is 'weak', so X[..., k-i] * decay**i stays float32 for a float32 X;
    a NumPy scalar (np.float64 included, although it subclasses float) is not"""
    return type(decay) in (float, int)


def _in_dtype(x, decay):
    """the device input dtype: float32 only when the reference would form float32 products"""
    return np.float32 if (residence.dtype_name(x) == "float32" and _weak_scalar(decay)) else np.float64


def _code(dtype):
    return _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64


def _stack(X, what):
    """the side a stack lives on and the stack as [L, H, W]: a torch device tensor [L, H, W] as it is, numpy (H, W, L) as
    the reference holds it with its last axis moved to the front"""
    side = residence.of(X, pooled=False)
    x = X if side.torch else np.asarray(X)
    if len(x.shape) != 3:
        raise ValueError(f"{what} takes " + ("a device stack [L, H, W]" if side.torch else "an (H, W, L) stack"))
    return side, (x if side.torch else np.moveaxis(x, 2, 0))


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
    side, x = _stack(X, "persistence")
    L, H, W = (int(v) for v in x.shape)
    _check_k(k, hold, L)
    if not side.torch:
        # only the n frames the sum reads are uploaded, to 0 .. n-1; relative to them the frame asked for is n-1 (k < 0 or
        # hold <= 0: none, zeros).  A device stack is resident as it is.
        n = max(0, min(k + 1, hold))
        x, L, k, hold = x[k + 1 - n:k + 1] if n else x[:0], n, n - 1, n or hold
    dt = _in_dtype(x, decay)
    frames = side.put("frames", x, dt)
    out = side.empty("out", (H, W), np.float64)
    with side.device():
        _run(frames.ptr, _code(dt), H * W, L, k, 1, hold, decay, out.ptr, _lib.REAL_F64, side.stream)
    return side.result(out, (H, W), np.float64)


def persistence_stack(X, hold, decay, out_dtype=np.float64):
    """persistence(X, k, hold, decay) for every k in one launch -- what the render loops of simple_kalman_tracker.py and
    range_doppler_plot.py compute frame by frame.  numpy (H, W, L) gives numpy (H, W, L); a torch device tensor
    [L, H, W] gives a device [L, H, W].  ``out_dtype`` float64 (bitwise the reference) or float32 (the float64 sum
    rounded once, for display)."""
    hold = int(hold)
    f32_out = np.dtype(out_dtype) == np.float32
    if not f32_out and np.dtype(out_dtype) != np.float64:
        raise ValueError("persistence_stack: out_dtype is float64 or float32")
    side, x = _stack(X, "persistence_stack")
    shape = L, H, W = tuple(int(v) for v in x.shape)
    dt = _in_dtype(x, decay)
    # a float32 out holds at most PERSISTENCE_TERMS_PER_LAUNCH terms (the launches chain through a float64 out)
    narrow = f32_out and min(hold, L) > _lib.PERSISTENCE_TERMS_PER_LAUNCH
    odt = np.float32 if f32_out and not narrow else np.float64
    frames = side.put("frames", x, dt)
    out = side.empty("out", shape, odt)
    with side.device():
        _run(frames.ptr, _code(dt), H * W, L, 0, L, hold, decay, out.ptr, _code(odt), side.stream)
    out = side.result(out, shape, odt)
    if side.torch:
        return out.float() if narrow else out
    out = np.moveaxis(out, 0, 2)
    return out.astype(np.float32) if narrow else out


# ---- display frames (range_doppler_plot.py:72-92) ----------------------------------------------------------------------
_ORIENT = {"plot": _lib.DISPLAY_PLOT, "stored": _lib.DISPLAY_STORED}


def gnuplot2_lut():
    """matplotlib's 'gnuplot2' as it colours bytes: uint8 (256, 4), the closed form at np.linspace(0, 1, 256) clipped to
    [0, 1], ``(lut * 255).astype(uint8)``, alpha 255 (the table prc_display_rgba builds for a NULL lut)"""
    x = np.linspace(0, 1, 256)
    r = x / 0.32 - 0.78125
    g = 2 * x - 0.84
    b = np.where(x < 0.25, 4 * x, np.where(x < 0.92, -2 * x + 1.84, x / 0.08 - 11.5))
    lut = np.clip(np.stack([r, g, b, np.ones_like(x)], axis=1), 0, 1)
    return (lut * 255).astype(np.uint8)


def _check_percentiles(p_lo, p_hi, hi_scale):
    p_lo, p_hi, hi_scale = float(p_lo), float(p_hi), float(hi_scale)
    if not (0.0 <= p_lo <= 100.0 and 0.0 <= p_hi <= 100.0):
        raise ValueError("Percentiles must be in the range [0, 100]")
    return p_lo, p_hi, hi_scale


def _check_lut(lut):
    if lut is None:
        return None
    t = np.asarray(lut)
    if t.dtype != np.uint8 or t.shape != (256, 4):
        raise ValueError("lut is a uint8 (256, 4) RGBA table")
    return np.ascontiguousarray(t)


def _check_orient(orient):
    if orient not in _ORIENT:
        raise ValueError("orient is 'plot' (fliplr(data.T), as the reference shows it) or 'stored'")
    return _ORIENT[orient]


def _check_frame_shape(H, W):
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"frames of {H} x {W}: need H, W >= 1 and H * W < 2^31")


def _display_dtype(x):
    """display frames are taken as float32 (kept) or float64 (everything else)"""
    return np.float32 if residence.dtype_name(x) == "float32" else np.float64


def _limits_arg(side, limits, L):
    """given limits, (L, 2), host array or tensor, as what ``side`` takes: a tensor as it is for torch, a float64 array
    otherwise"""
    if residence.shape(limits) != (L, 2):
        raise ValueError(f"limits is (L, 2) = ({L}, 2)")
    if side.torch and hasattr(limits, "data_ptr"):
        return limits
    return np.asarray(limits.cpu() if hasattr(limits, "cpu") else limits, dtype=np.float64)


def _limits(frames_ptr, code, elems, nframes, p_lo, p_hi, hi_scale, limits_ptr, stream):
    check(lib().prc_display_limits(frames_ptr, code, int(elems), int(nframes), p_lo, p_hi, hi_scale, limits_ptr, stream))


def _rgba(frames_ptr, code, H, W, nframes, limits_ptr, lut, orient, out_ptr, stream):
    check(lib().prc_display_rgba(frames_ptr, code, int(H), int(W), int(nframes), limits_ptr,
                                 None if lut is None else lut.ctypes.data, orient, out_ptr, stream))


def display_limits(X, p_lo=35, p_hi=99, hi_scale=1.5):
    """per frame ``(np.percentile(frame, p_lo), hi_scale * np.percentile(frame, p_hi))`` -- the vmin / vmax of
    range_doppler_plot.py:75-76 -- from exact order statistics, bit for bit NumPy's float64 result (a float32 stack is
    taken as its values widened to float64).  numpy (H, W, L) gives numpy (L, 2) float64; a torch device tensor
    [L, H, W] gives a device (L, 2) float64 on the tensor's device and torch's current stream."""
    p_lo, p_hi, hi_scale = _check_percentiles(p_lo, p_hi, hi_scale)
    side, x = _stack(X, "display_limits")
    L, H, W = (int(v) for v in x.shape)
    _check_frame_shape(H, W)
    if L == 0:
        return side.nothing((0, 2), np.float64)
    dt = _display_dtype(x)
    frames = side.put("frames", x, dt)
    lim = side.empty("limits", (L, 2), np.float64)
    with side.device():
        _limits(frames.ptr, _code(dt), H * W, L, p_lo, p_hi, hi_scale, lim.ptr, side.stream)
    return side.result(lim, (L, 2), np.float64)


def render_frames(X, lut=None, limits=None, p_lo=35, p_hi=99, hi_scale=1.5, orient="plot"):
    """``imshow(np.fliplr(frame.T), cmap=lut, vmin=limits[k, 0], vmax=limits[k, 1])`` per frame as RGBA8, one pixel per
    cell: matplotlib's ``Normalize`` then ``Colormap.__call__(bytes=True)`` in float64, byte for byte.  ``lut``: a uint8
    (256, 4) table, None = gnuplot2.  ``limits``: None = ``display_limits(X, p_lo, p_hi, hi_scale)``; else (L, 2) (host
    array or device tensor), used as they are -- one fixed scale for a whole video.  A NaN cell (or NaN limits) gives
    (0, 0, 0, 0), vmin == vmax gives lut[0]; where matplotlib raises for vmin > vmax, that frame is (0, 0, 0, 0)
    throughout and the limits show why.  ``orient``: "plot" = fliplr(frame.T), result [L, W, H, 4]; "stored" = the
    frames as they lie, [L, H, W, 4].  numpy (H, W, L) in gives numpy out; a torch device tensor [L, H, W] gives a
    device tensor on the tensor's device and torch's current stream."""
    p_lo, p_hi, hi_scale = _check_percentiles(p_lo, p_hi, hi_scale)
    lut = _check_lut(lut)
    oc = _check_orient(orient)
    side, x = _stack(X, "render_frames")
    L, H, W = (int(v) for v in x.shape)
    _check_frame_shape(H, W)
    shape = (L, W, H, 4) if oc == _lib.DISPLAY_PLOT else (L, H, W, 4)
    if limits is not None:
        limits = _limits_arg(side, limits, L)
    if L == 0:
        return side.nothing(shape, np.uint8)
    dt = _display_dtype(x)
    frames = side.put("frames", x, dt)
    lim = side.empty("limits", (L, 2), np.float64) if limits is None else side.put("limits", limits, np.float64)
    out = side.empty("out", shape, np.uint8)
    with side.device():
        if limits is None:
            _limits(frames.ptr, _code(dt), H * W, L, p_lo, p_hi, hi_scale, lim.ptr, side.stream)
        _rgba(frames.ptr, _code(dt), H, W, L, lim.ptr, lut, oc, out.ptr, side.stream)
    return side.result(out, shape, np.uint8)


RENDER_SLAB_BYTES = 1 << 28     # render_maps: float64 persistence frames alive at a time (default slab)


def render_maps(xambg, fw=18, gw=4, hold=20, decay=0.9, slab=None, cfar="mean", cfar_rank=None, **render_kw):
    """range_doppler_plot.py:43-92 as one device chain on the caller's stream: CFAR_2D(|xambg|, fw, gw) per frame
    (CFAR_2D_abs; CFAR_2D for a real magnitude stack), persistence(CF, k, hold, decay) of the float64 CFAR maps for every
    k, then ``render_frames(**render_kw)``.  ``xambg`` is a torch device tensor [L, H, W] (result: a device tensor
    [L, W, H, 4], or [L, H, W, 4] for orient="stored") or numpy (H, W, L) as the script loads it (result: numpy; the
    chain runs through torch).  The float64 persistence frames exist ``slab`` frames at a time (default: as many as fit
    RENDER_SLAB_BYTES); a slab reads the ``hold - 1`` CFAR frames before its first one.  Given ``limits`` are (L, 2).
    ``cfar="os"`` puts CFAR_2D_OS (reference scale, rank ``cfar_rank``) in the cell average's place."""
    import torch
    from .target_detection import _chain_cfar, _check_cfar
    _check_cfar(cfar)
    hold = int(hold)
    if slab is not None and int(slab) < 1:
        raise ValueError("slab is a number of frames >= 1")
    side = residence.of(xambg)
    if not side.torch:
        x = np.asarray(xambg)
        if x.ndim != 3:
            raise ValueError("render_maps takes (H, W, L) maps")
        _lib.require_gpu()
        x = np.ascontiguousarray(np.moveaxis(x, 2, 0), dtype=np.complex64 if np.iscomplexobj(x) else np.float32)
        return render_maps(torch.from_numpy(x).cuda(), fw, gw, hold, decay, slab, cfar, cfar_rank, **render_kw).cpu().numpy()
    if xambg.dim() != 3:
        raise ValueError("render_maps takes a device stack [L, H, W]")
    shape = L, H, W = tuple(int(v) for v in xambg.shape)
    _check_frame_shape(H, W)
    limits = render_kw.pop("limits", None)
    if limits is not None:
        limits = _limits_arg(side, limits, L)
        limits = (limits if hasattr(limits, "data_ptr") else torch.from_numpy(limits)).to(device=xambg.device, dtype=torch.float64)
    if L == 0:
        return render_frames(torch.empty((0, H, W), dtype=torch.float64, device=xambg.device), limits=limits, **render_kw)
    cplx = xambg.is_complex()
    maps = side.put("maps", xambg, np.complex64 if cplx else np.float32)
    cf = side.result(_chain_cfar(side, maps, shape, cplx, fw, gw, cfar, cfar_rank), shape, np.float32)
    step = int(slab) if slab is not None else max(1, RENDER_SLAB_BYTES // (H * W * 8))
    outs = []
    for s0 in range(0, L, step):
        s1 = min(L, s0 + step)
        b0 = max(0, s0 - max(hold - 1, 0))                  # the first CFAR frame this slab's sums read
        src = cf[b0:s1].to(torch.float64)                   # the reference's CF is float64: float64 products
        st = torch.empty((s1 - s0, H, W), dtype=torch.float64, device=cf.device)
        with side.device():
            _run(src.data_ptr(), _lib.REAL_F64, H * W, s1 - b0, s0 - b0, s1 - s0, hold, decay, st.data_ptr(),
                 _lib.REAL_F64, side.stream)
        outs.append(render_frames(st, limits=None if limits is None else limits[s0:s1], **render_kw))
    return outs[0] if len(outs) == 1 else torch.cat(outs)
