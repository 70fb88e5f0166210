"""Welch spectra on the device: ``psd``, ``csd`` and ``specgram`` with matplotlib.mlab's names, argument names and return
values for complex input (``sides='twosided'``, ``pad_to == NFFT``; neither is offered), and ``preview``, the arithmetic of
the reference's ``signal_preview.py`` without its figures.  One kernel family serves all three (prc_welch, include/prcore.h):
Hann-windowed (or any real window) segments transformed inside LDS, |X|^2 or conj(X) Y summed in float64 in a fixed order.

A NumPy array gives NumPy results.  A torch device tensor is read in place on torch's current stream and gives device
tensors: complex64, or -- with ``raw=True`` -- an int8 / uint8 / int16 / float32 tensor of interleaved I,Q scalars as the
recordings hold them, converted while it is loaded.  A 2-D input ``[nch, n]`` gives one more leading axis.  ``step=k``
reads every k-th complex sample (``x[0::k]``; pass ``x[1:]`` for ``x[1::k]``): two channels interleaved sample by sample
(signal_preview.py:33-34) need no de-interleaved copy."""
from __future__ import annotations

import collections
import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import check, lib

__all__ = ["psd", "csd", "specgram", "preview"]

_RAW_NUMPY = ("int8", "uint8", "int16", "float32")
_WINDOW_CACHE_ENTRIES = 16
_windows = collections.OrderedDict()     # (device, float32 window bytes) -> DeviceBuffer
_windows_lock = threading.Lock()


def _window64(window, NFFT):
    if window is None:
        return np.hanning(NFFT)
    if callable(window):
        raise ValueError("window is None (Hann) or an array of NFFT real values")
    w = np.asarray(window)
    if w.ndim != 1 or w.shape[0] != NFFT or np.iscomplexobj(w):
        raise ValueError("The window length must match the data's first dimension")     # mlab's message
    return w.astype(np.float64)


def _detrend_code(detrend):
    if detrend is None or (isinstance(detrend, str) and detrend == "none"):
        return 0
    if isinstance(detrend, str) and detrend == "mean":
        return 1
    raise ValueError("detrend is None, 'none' or 'mean'")


def _check_nfft(NFFT, noverlap):
    NFFT, noverlap = int(NFFT), int(noverlap)
    if NFFT < 64 or NFFT > 8192 or NFFT & (NFFT - 1):
        raise ValueError("NFFT is a power of two in 64 .. 8192")
    if noverlap >= NFFT:
        raise ValueError("noverlap must be less than NFFT")                               # mlab's message
    if noverlap < 0:
        raise ValueError("noverlap is not negative")
    return NFFT, noverlap


def _scale(w64, Fs, scale_by_freq):
    """mlab's scaling for a two-sided spectrum, in float64 from the float64 window"""
    if scale_by_freq is None or scale_by_freq:
        return 1.0 / (float(Fs) * float((np.abs(w64) ** 2).sum()))
    return 1.0 / float(np.abs(w64).sum() ** 2)


def _freqs(NFFT, Fs, Fc):
    f = np.fft.fftfreq(NFFT, 1 / Fs)
    return np.roll(f, -(NFFT // 2), axis=0) + Fc


def _device_window(w32, device):
    """the float32 window on the device, from a small cache keyed by its bytes"""
    key = (device, w32.tobytes())
    with _windows_lock:
        buf = _windows.get(key)
        if buf is None:
            buf = _lib.DeviceBuffer(w32.nbytes)
            buf.upload(w32)
            _windows[key] = buf
            while len(_windows) > _WINDOW_CACHE_ENTRIES:
                _windows.popitem(last=False)
        else:
            _windows.move_to_end(key)
        return buf


class _Input:
    """what prc_welch needs to know about x (and y): dtype code, samples per channel, channels, stride in complex elements"""
    __slots__ = ("code", "n", "nch", "stride", "batched", "device", "keep")


def _describe(x, raw, step, what):
    i = _Input()
    i.device = _lib.is_device_tensor(x)
    if i.device:
        import torch
        if raw:
            names = {torch.int8: "int8", torch.uint8: "uint8", torch.int16: "int16", torch.float32: "float32"}
            if x.dtype not in names:
                raise ValueError(f"{what}: raw=True takes int8, uint8, int16 or float32 interleaved I,Q scalars")
            i.code = _lib.RAW_DTYPES[names[x.dtype]]
        else:
            if x.dtype != torch.complex64:
                raise ValueError(f"{what}: a device tensor is complex64 (or raw scalars with raw=True)")
            i.code = _lib.RAW_DTYPES["complex64"]
        if x.dim() not in (1, 2):
            raise ValueError(f"{what} takes [n] or [nch, n]")
        if x.stride(-1) != 1 or (raw and x.dim() == 2 and x.stride(0) % 2):
            x = x.contiguous()
        length, i.batched = x.shape[-1], x.dim() == 2
        i.nch = x.shape[0] if i.batched else 1
        row = x.stride(0) if i.batched else length
    else:
        x = np.asarray(x)
        if raw:
            if str(x.dtype) not in _RAW_NUMPY:
                raise ValueError(f"{what}: raw=True takes int8, uint8, int16 or float32 interleaved I,Q scalars")
            i.code = _lib.RAW_DTYPES[str(x.dtype)]
            x = np.ascontiguousarray(x)
        else:
            x = np.ascontiguousarray(x, dtype=np.complex64)
            i.code = _lib.RAW_DTYPES["complex64"]
        if x.ndim not in (1, 2):
            raise ValueError(f"{what} takes [n] or [nch, n]")
        length, i.batched = x.shape[-1], x.ndim == 2
        i.nch = x.shape[0] if i.batched else 1
        row = length
    if raw:
        length, row = length // 2, row // 2
    i.n = (length + step - 1) // step
    i.stride = row
    i.keep = x
    if i.n < 1 or i.nch < 1:
        raise ValueError(f"{what}: no samples")
    return i


def _welch(x, y, NFFT, Fs, detrend, window, noverlap, scale_by_freq, navg, raw, step, what):
    """the shared body: returns (out [nch][rows][NFFT] float64 / complex128 as numpy or a device tensor, batched, nseg)"""
    NFFT, noverlap = _check_nfft(NFFT, noverlap)
    step, navg = int(step), int(navg)
    if step < 1:
        raise ValueError("step is at least 1")
    if navg < 0:
        raise ValueError("navg is not negative")
    w64 = _window64(window, NFFT)
    ix = _describe(x, raw, step, what)
    iy = None
    if y is not None:
        iy = _describe(y, raw, step, what)
        if iy.device != ix.device:
            raise ValueError(f"{what}: x and y are both NumPy arrays or both device tensors")
        if (iy.n, iy.nch) != (ix.n, ix.nch):
            raise ValueError(f"{what}: x and y have different lengths")
        if iy.code != ix.code:
            raise ValueError(f"{what}: x and y have different dtypes")
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.in_dtype, d.step = NFFT, noverlap, navg, _detrend_code(detrend), ix.code, step
    d.scale = _scale(w64, Fs, scale_by_freq)
    nseg, rows, ws = C.c_int64(0), C.c_int64(0), C.c_size_t(0)
    check(lib().prc_welch_rows(C.byref(d), ix.n, C.byref(nseg), C.byref(rows)))          # navg > nseg: ValueError
    check(lib().prc_welch_workspace_bytes(C.byref(d), ix.n, ix.nch, C.byref(ws)))
    rows, nseg = int(rows.value), int(nseg.value)
    w32 = w64.astype(np.float32)
    shape = (ix.nch, rows, NFFT)
    if ix.device:
        import torch
        xt, yt = ix.keep, (iy.keep if iy is not None else None)
        if yt is not None:
            if yt.device != xt.device:
                raise ValueError(f"{what}: x and y are on different devices")
            if iy.stride != ix.stride:       # one stride serves both: lay y out as x
                if ix.batched:
                    xt, yt = xt.contiguous(), yt.contiguous()
                    ix.stride = iy.stride = xt.shape[-1] // (2 if raw else 1)
        with torch.cuda.device(xt.device):
            wbuf = _device_window(w32, xt.device.index)
            out = torch.empty(shape, dtype=torch.float64 if yt is None else torch.complex128, device=xt.device)
            work = torch.empty(((int(ws.value) + 7) // 8,), dtype=torch.float64, device=xt.device)
            check(lib().prc_welch(C.byref(d), xt.data_ptr(), None if yt is None else yt.data_ptr(), ix.n, ix.stride, ix.nch,
                                  wbuf.ptr, out.data_ptr(), work.data_ptr(), _lib.torch_stream_ptr(xt.device)))
        return out, ix.batched, nseg
    _lib.require_gpu()
    wbuf = _device_window(w32, _lib.current_device())
    dx = _lib.DeviceBuffer(ix.keep.nbytes)
    dx.upload(ix.keep)
    dy = None
    if iy is not None:
        dy = _lib.DeviceBuffer(iy.keep.nbytes)
        dy.upload(iy.keep)
    odt = np.float64 if iy is None else np.complex128
    do = _lib.DeviceBuffer(int(np.prod(shape)) * np.dtype(odt).itemsize)
    dw = _lib.DeviceBuffer(int(ws.value))
    check(lib().prc_welch(C.byref(d), dx.ptr, None if dy is None else dy.ptr, ix.n, ix.stride, ix.nch, wbuf.ptr, do.ptr,
                          dw.ptr, None))
    return do.download(shape, odt), ix.batched, nseg


def psd(x, NFFT=256, Fs=2, detrend=None, window=None, noverlap=0, scale_by_freq=True, Fc=0, raw=False, step=1):
    """``matplotlib.mlab.psd`` for complex input: ``(Pxx, freqs)``, Pxx float64 ``(NFFT,)`` -- ``(nch, NFFT)`` for a 2-D
    input -- with the frequency axis centred, ``freqs`` mlab's array plus ``Fc`` as ``plt.psd`` shows it.  ``window``: None
    (``np.hanning(NFFT)``) or NFFT real values; ``detrend``: None, 'none' or 'mean'."""
    out, batched, _ = _welch(x, None, NFFT, Fs, detrend, window, noverlap, scale_by_freq, 0, raw, step, "psd")
    return (out[:, 0] if batched else out[0, 0]), _freqs(int(NFFT), Fs, Fc)


def csd(x, y, NFFT=256, Fs=2, detrend=None, window=None, noverlap=0, scale_by_freq=True, Fc=0, raw=False, step=1):
    """``matplotlib.mlab.csd`` for complex input: ``(Pxy, freqs)``, Pxy complex128, the mean of conj(X) Y.  Inputs of
    different length raise ValueError."""
    out, batched, _ = _welch(x, y, NFFT, Fs, detrend, window, noverlap, scale_by_freq, 0, raw, step, "csd")
    return (out[:, 0] if batched else out[0, 0]), _freqs(int(NFFT), Fs, Fc)


def specgram(x, NFFT=256, Fs=2, detrend=None, window=None, noverlap=128, scale_by_freq=True, navg=1, Fc=0, raw=False,
             step=1):
    """``matplotlib.mlab.specgram`` (mode 'psd') for complex input: ``(spec, freqs, t)``, spec float64 ``(NFFT, rows)`` as
    mlab returns it (a transposed view of the device layout; ``(nch, NFFT, rows)`` for a 2-D input).  ``navg=k`` averages k
    consecutive segments into one row (a waterfall of a long recording; segments left over are dropped) and ``t`` is then
    the mean of their times; ``navg=0`` is one row of all segments; more than there are segments raises ValueError."""
    out, batched, nseg = _welch(x, None, NFFT, Fs, detrend, window, noverlap, scale_by_freq, navg, raw, step, "specgram")
    NFFT, noverlap, navg = int(NFFT), int(noverlap), int(navg)
    # mlab: arange(NFFT / 2, len(x) - NFFT / 2 + 1, NFFT - noverlap) / Fs, one time per segment (a short x is padded to NFFT)
    t = (NFFT / 2 + np.arange(nseg) * (NFFT - noverlap)) / Fs
    if navg != 1:
        k = nseg if navg == 0 else navg
        t = t[:(nseg // k) * k].reshape(-1, k).mean(axis=1)
    spec = out.transpose(1, 2) if _lib.is_device_tensor(out) else np.swapaxes(out, 1, 2)
    return (spec if batched else spec[0]), _freqs(NFFT, Fs, Fc), t


def preview(config, raw_ref, raw_srv=None):
    """signal_preview.py:28-82 without the figures.  ``raw_ref`` / ``raw_srv``: the raw recordings (interleaved I,Q
    scalars); with ``config['interleaved_input_channels']`` ``raw_ref`` holds both channels sample by sample.  Returns a
    dict: ``offset`` (find_channel_offset(ref, srv, 4, 50000)), ``input_psd`` (2, 8192) in dB with ``input_freqs``,
    ``channel_psd`` (2, 2048) in dB of the tuned and resampled channels with ``channel_freqs``, ``xcorr_lags`` and
    ``xcorr_abs``.  The spectra of the raw channels read the raw scalars (2 bytes per int8 sample)."""
    from .signal_utils import deinterleave_IQ, find_channel_offset, frequency_shift, resample, xcorr
    icl = int(config["input_chunk_length"])
    fs_in, fc_in = config["input_sample_rate"], config["input_center_freq"]
    if config["interleaved_input_channels"]:
        data = np.ascontiguousarray(np.asarray(raw_ref)[0:icl])
        iq = deinterleave_IQ(data)
        ref, srv = iq[0::2], iq[1::2]
        raw_spectra = [(data, 2), (data[2:], 2)]
    else:
        if raw_srv is None:
            raise ValueError("preview: raw_srv is needed unless config['interleaved_input_channels'] is set")
        a, b = np.ascontiguousarray(np.asarray(raw_ref)[0:icl]), np.ascontiguousarray(np.asarray(raw_srv)[0:icl])
        ref, srv = deinterleave_IQ(a), deinterleave_IQ(b)
        raw_spectra = [(a, 1), (b, 1)]
    raw_ok = all(str(r.dtype) in _RAW_NUMPY for r, _ in raw_spectra)
    offset = find_channel_offset(ref, srv, 4, 50000)
    pin = []
    for (r, step), z in zip(raw_spectra, (ref, srv)):
        p, f_in = psd(r, NFFT=8192, Fs=fs_in, Fc=fc_in, raw=True, step=step) if raw_ok else psd(z, NFFT=8192, Fs=fs_in, Fc=fc_in)
        pin.append(p)
    pch = []
    for z in (ref, srv):
        zz = resample(frequency_shift(z, config["offset_freq"], fs_in), config["resamp_up"], config["resamp_dn"])
        p, f_ch = psd(zz, NFFT=2048, Fs=config["channel_bandwidth"], Fc=config["channel_freq"])
        pch.append(p)
    with np.errstate(divide="ignore"):
        return dict(offset=offset, input_psd=10 * np.log10(np.stack(pin)), input_freqs=f_in,
                    channel_psd=10 * np.log10(np.stack(pch)), channel_freqs=f_ch,
                    xcorr_lags=np.arange(-2000, 2001), xcorr_abs=np.abs(xcorr(ref, srv, 2000, 2000)))
