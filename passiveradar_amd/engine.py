"""Thin Python owners of the libprcore plans (device-pointer level).

Everything here takes raw device pointers (ints) + a hipStream_t, so it works both for the
NumPy-facing drop-in functions (which stage through ``_lib.DeviceBuffer``) and for callers that
already hold torch device tensors (``tensor.data_ptr()``; bench.py, stream.py).
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib
from ._lib import check, lib


def _ptr(x):
    """int / c_void_p / DeviceBuffer or another handle of residence.py (``.ptr``) / torch tensor -> c_void_p"""
    if x is None:
        return None
    if hasattr(x, "ptr"):
        return C.c_void_p(x.ptr)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    if isinstance(x, C.c_void_p):
        return x
    return C.c_void_p(int(x))


class CafPlan:
    """prc_caf_plan: fast_xambg for up to ``max_frames`` frames per launch."""

    def __init__(self, n, range_bins, freq_bins, max_frames=1, method=_lib.CAF_AUTO,
                 doppler=_lib.DOPPLER_AUTO, taps=None, multi=_lib.CAF_MULTI_AUTO):
        self.n, self.range_bins, self.freq_bins = int(n), int(range_bins), int(freq_bins)
        self.max_frames = int(max_frames)
        d = _lib.CafDesc()
        d.n, d.range_bins, d.freq_bins = self.n, self.range_bins, self.freq_bins
        d.max_frames, d.method, d.doppler = self.max_frames, int(method), int(doppler)
        d.multi = _lib.CAF_MULTI_MODES[multi] if isinstance(multi, str) else int(multi)
        self._taps = None
        if taps is not None:
            self._taps = np.ascontiguousarray(taps, dtype=np.float32)
            d.ntaps = self._taps.size
            d.taps_host = self._taps.ctypes.data_as(C.POINTER(C.c_float))
        else:
            d.ntaps = 0
            d.taps_host = None
        h = C.c_void_p()
        check(lib().prc_caf_plan_create(C.byref(h), C.byref(d)))
        self._h = h
        m, dp, ws = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().prc_caf_plan_info(self._h, C.byref(m), C.byref(dp), C.byref(ws)))
        self.method, self.doppler, self.workspace_bytes = m.value, dp.value, ws.value
        mm = C.c_int32()
        check(lib().prc_caf_plan_multi_mode(self._h, C.byref(mm)))
        self.multi = mm.value               # what AUTO resolved to (turns / shared / pairs)

    @property
    def out_shape(self):
        return (self.freq_bins, self.range_bins + 1)

    def execute(self, ref, srv, out, nframes=1, frame_stride=None, n_valid=None, window=None,
                stream=None):
        check(lib().prc_caf_execute(self._h, _ptr(ref), _ptr(srv),
                                    self.n if frame_stride is None else int(frame_stride),
                                    self.n if n_valid is None else int(n_valid),
                                    _ptr(window), _ptr(out), int(nframes), stream))

    def execute_multi(self, refs, srv, outs, nframes=1, frame_stride=None, n_valid=None, window=None, stream=None):
        """prc_caf_execute_multi: every reference channel of ``refs`` against ONE surveillance channel in one call;
        ``outs[i]`` receives what ``execute(refs[i], srv, ...)`` would write (len(refs) * nframes <= max_frames)."""
        nref = len(refs)
        rp = (C.c_void_p * nref)(*[_ptr(r) for r in refs])
        op = (C.c_void_p * nref)(*[_ptr(o) for o in outs])
        check(lib().prc_caf_execute_multi(self._h, rp, nref, _ptr(srv),
                                          self.n if frame_stride is None else int(frame_stride),
                                          self.n if n_valid is None else int(n_valid),
                                          _ptr(window), op, int(nframes), stream))

    def execute_segments(self, ref, srv, nframes=1, frame_stride=None, n_valid=None, window=None,
                         stream=None):
        check(lib().prc_caf_execute_segments(self._h, _ptr(ref), _ptr(srv),
                                             self.n if frame_stride is None else int(frame_stride),
                                             self.n if n_valid is None else int(n_valid),
                                             _ptr(window), int(nframes), stream))

    def execute_doppler(self, out, nframes=1, stream=None):
        check(lib().prc_caf_execute_doppler(self._h, _ptr(out), int(nframes), stream))

    def close(self):
        if getattr(self, "_h", None):
            lib().prc_caf_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LsPlan:
    """prc_ls_plan: LS_Filter_Toeplitz / LS_Filter_Multiple / LS_Filter on up to max_blocks blocks."""

    def __init__(self, n, filter_len, peek=10, circular=False, max_blocks=1, method=0):
        self.n, self.filter_len, self.peek = int(n), int(filter_len), int(peek)
        self.ntaps = self.filter_len + self.peek
        self.max_blocks = int(max_blocks)
        d = _lib.LsDesc()
        d.n, d.filter_len, d.peek = self.n, self.filter_len, self.peek
        d.circular, d.max_blocks, d.method = int(bool(circular)), self.max_blocks, int(method)
        h = C.c_void_p()
        check(lib().prc_ls_plan_create(C.byref(h), C.byref(d)))
        self._h = h

    def execute(self, ref, srv, out, nblocks=1, stride=None, out_stride=None, sample_rate=1.0,
                doppler_bins=(0,), reg=0.0, taps_out=None, stream=None):
        bins = (C.c_double * len(doppler_bins))(*[float(b) for b in doppler_bins])
        check(lib().prc_ls_execute(self._h, _ptr(ref), _ptr(srv),
                                   self.n if stride is None else int(stride), _ptr(out),
                                   self.n if out_stride is None else int(out_stride), int(nblocks),
                                   float(sample_rate), bins, len(doppler_bins), float(reg),
                                   _ptr(taps_out), stream))

    def set_profiling(self, enable=True):
        check(lib().prc_ls_set_profiling(self._h, int(bool(enable))))

    def get_profile(self):
        """((ms_corr, ms_solve, ms_fir), (launches_corr, launches_solve, launches_fir)) of the last
        execute; in the cached chain the correlation of bin i+1 runs inside the FIR kernel of bin i"""
        ms = (C.c_double * 3)()
        k = (C.c_int32 * 3)()
        check(lib().prc_ls_get_profile(self._h, ms, k))
        return (ms[0], ms[1], ms[2]), (k[0], k[1], k[2])

    def close(self):
        if getattr(self, "_h", None):
            lib().prc_ls_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cheby1_lowpass_zpk(order, rp, wn):
    """Digital Chebyshev type-I low-pass as scipy.signal.cheby1(order, rp, wn, output='zpk') designs it:
    analog prototype poles -sinh(mu + j theta_m), cut-off pre-warped to 4 tan(pi wn / 2) (fs = 2), bilinear
    transform; all zeros at z = -1.  Returns (zeros, poles, gain)."""
    eps = np.sqrt(10.0 ** (0.1 * rp) - 1.0)
    mu = np.arcsinh(1.0 / eps) / order
    theta = np.pi * np.arange(-order + 1, order, 2) / (2 * order)
    p = -np.sinh(mu + 1j * theta)
    k = np.prod(-p).real
    if order % 2 == 0:
        k /= np.sqrt(1.0 + eps * eps)
    warped = 4.0 * np.tan(np.pi * wn / 2.0)
    p = p * warped
    k = k * warped ** order
    pz = (4.0 + p) / (4.0 - p)
    kz = k * np.real(1.0 / np.prod(4.0 - p))
    return -np.ones(order, dtype=np.complex128), pz, float(kz)


class IirDecimator:
    """prc_iir_desc of scipy.signal.decimate(x, q) with its defaults (ftype='iir', n=8, zero_phase=True):
    cheby1(8, 0.05, 0.8/q) through sosfiltfilt, whose odd extension is 3*(2*4+1) = 27 samples."""

    def __init__(self, q, order=8):
        if int(q) != q or q < 1:
            raise ValueError("q must be a positive integer")       # scipy: operator.index(q)
        z, p, k = cheby1_lowpass_zpk(order, 0.05, 0.8 / int(q))
        nsec = (order + 1) // 2
        self.q = int(q)
        self.padlen = 3 * (2 * nsec + 1)
        # |pole|^settle < 1e-9: the recursion's memory, replaced by an explicit constant extension
        self.settle = int(np.ceil(np.log(1e-9) / np.log(np.abs(p).max()) / 64.0)) * 64
        self._z = np.ascontiguousarray(np.stack([z.real, z.imag], -1).reshape(-1))
        self._p = np.ascontiguousarray(np.stack([p.real, p.imag], -1).reshape(-1))
        d = _lib.IirDesc()
        d.q, d.padlen, d.settle, d.nzeros, d.npoles, d.gain = self.q, self.padlen, self.settle, z.size, p.size, k
        d.zeros_host = self._z.ctypes.data_as(C.POINTER(C.c_double))
        d.poles_host = self._p.ctypes.data_as(C.POINTER(C.c_double))
        self.desc = d

    def out_len(self, n):
        return -(-int(n) // self.q)

    def decimate(self, x, n, y, stream=None):
        """y[j] = sosfiltfilt(x)[j q] (complex64 device buffers)"""
        check(lib().prc_decimate_iir(_ptr(x), int(n), C.byref(self.desc), _ptr(y), stream))

    def channel_offset(self, s1, n1, s2, n2, nl, xc_out=None, stream=None):
        """(argmax index, number of lags) of |correlate(decimate(s1), pad(decimate(s2), nl), 'valid')|"""
        n_xc, am = C.c_int64(), C.c_int64()
        check(lib().prc_channel_offset(_ptr(s1), int(n1), _ptr(s2), int(n2), C.byref(self.desc), int(nl),
                                       _ptr(xc_out), C.byref(n_xc), C.byref(am), stream))
        return am.value, n_xc.value

    def n_lags(self, n1, n2, nl):
        return self.out_len(n2) + 2 * int(nl) - self.out_len(n1) + 1

    def close(self):
        """nothing device-side to release (the plan cache calls this on eviction)"""


def resample_design(up, dn):
    """scipy.signal.resample_poly's filter and alignment for signal_utils.resample (signal_utils.py:15-17):
    returns (taps with n_pre_pad leading zeros, float32; n_pre_remove; up; dn) with up/dn reduced."""
    from math import gcd
    from scipy.signal import firwin
    g = gcd(int(up), int(dn))
    up, dn = int(up) // g, int(dn) // g
    max_rate = max(up, dn)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up
    n_pre_pad = dn - half_len % dn
    taps = np.concatenate((np.zeros(n_pre_pad), h)).astype(np.float32)
    return taps, (half_len + n_pre_pad) // dn, up, dn


class FrontendPlan:
    """prc_frontend_plan: deinterleave -> tune (block phase) -> resample, fused, up to max_blocks blocks."""

    def __init__(self, n_in, raw_dtype, up, dn, max_blocks=1):
        taps, npr, up, dn = resample_design(up, dn)
        self.n_in, self.up, self.dn = int(n_in), up, dn
        self.raw_is_complex = str(raw_dtype) == "complex64"     # raw_stride then counts complex samples
        self._taps = np.ascontiguousarray(taps)
        d = _lib.FrontendDesc()
        d.n_in, d.raw_dtype, d.up, d.down = self.n_in, _lib.RAW_DTYPES[str(raw_dtype)], up, dn
        d.ntaps, d.n_pre_remove, d.max_blocks = self._taps.size, npr, int(max_blocks)
        d.taps_host = self._taps.ctypes.data_as(C.POINTER(C.c_float))
        h = C.c_void_p()
        check(lib().prc_frontend_plan_create(C.byref(h), C.byref(d)))
        self._h = h
        n = C.c_int64()
        check(lib().prc_frontend_out_len(self._h, C.byref(n)))
        self.n_out = n.value

    def execute(self, raw, out, nblocks=1, raw_stride=None, out_stride=None, fc=0.0, fs=1.0, phases=None,
                mix=True, stream=None):
        ph = None
        if phases is not None:
            ph = (C.c_double * nblocks)(*[float(p) for p in phases])
        itemscalars = 1 if self.raw_is_complex else 2
        check(lib().prc_frontend_execute(self._h, _ptr(raw),
                                         int(self.n_in * itemscalars if raw_stride is None else raw_stride),
                                         int(bool(mix)), float(fc), float(fs), ph, _ptr(out),
                                         int(self.n_out if out_stride is None else out_stride), int(nblocks), stream))

    def execute2(self, raw_a, raw_b, out_a, out_b, nblocks=1, raw_stride=None, out_stride=None, fc=0.0, fs=1.0,
                 phases=None, mix=True, stream=None):
        """prc_frontend_execute2: both channels of every block in one launch (same strides, same phases)"""
        ph = None
        if phases is not None:
            ph = (C.c_double * nblocks)(*[float(p) for p in phases])
        itemscalars = 1 if self.raw_is_complex else 2
        check(lib().prc_frontend_execute2(self._h, _ptr(raw_a), _ptr(raw_b),
                                          int(self.n_in * itemscalars if raw_stride is None else raw_stride),
                                          int(bool(mix)), float(fc), float(fs), ph, _ptr(out_a), _ptr(out_b),
                                          int(self.n_out if out_stride is None else out_stride), int(nblocks), stream))

    def close(self):
        if getattr(self, "_h", None):
            lib().prc_frontend_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nlms_execute(ref, srv, out, n, filter_len, mu, peek=10, taps_in=None, taps_out=None,
                 nstreams=1, stride=None, out_stride=None, stream=None):
    check(lib().prc_nlms_execute(_ptr(ref), _ptr(srv), int(n), int(n if stride is None else stride),
                                 int(filter_len), int(peek), float(mu), _ptr(taps_in), _ptr(out),
                                 int(n if out_stride is None else out_stride), _ptr(taps_out),
                                 int(nstreams), stream))


def gal_workspace_bytes(delay_len, nstreams=1):
    """device bytes prc_gal_execute needs for ``nstreams`` streams of ``delay_len`` taps (0 up to 2048 taps)"""
    nb = C.c_size_t(0)
    check(lib().prc_gal_workspace_bytes(int(delay_len), int(nstreams), C.byref(nb)))
    return int(nb.value)


def gal_execute(ref, srv, out, n, lattice_len, delay_len, mu1, mu2, peek=10, k_out=None, h_out=None,
                nstreams=1, stride=None, out_stride=None, workspace=None, stream=None):
    """GAL_JPE over ``nstreams`` independent streams (device buffers or torch tensors); ``workspace``: a device buffer of
    gal_workspace_bytes(delay_len, nstreams) bytes when that is non-zero.  ``stream``: the torch stream's handle."""
    check(lib().prc_gal_execute(_ptr(ref), _ptr(srv), int(n), int(n if stride is None else stride), int(lattice_len),
                                int(delay_len), int(peek), float(mu1), float(mu2), _ptr(out),
                                int(n if out_stride is None else out_stride), _ptr(k_out), _ptr(h_out), int(nstreams),
                                _ptr(workspace), stream))


def ls_svd_workspace_bytes(n, filter_len, peek=10, nblocks=1):
    """device bytes prc_ls_svd_execute needs for ``nblocks`` blocks of ``n`` samples and filter_len + peek taps"""
    nb = C.c_size_t(0)
    check(lib().prc_ls_svd_workspace_bytes(int(n), int(filter_len), int(peek), int(nblocks), C.byref(nb)))
    return int(nb.value)


def ls_svd_execute(ref, srv, out, n, filter_len, peek=10, rcond=None, nblocks=1, stride=None, out_stride=None,
                   taps_out=None, sv_out=None, info_out=None, workspace=None, stream=None):
    """LS_Filter_SVD over ``nblocks`` independent blocks (device buffers or torch tensors).  ``rcond``: None = the default
    cut 4 sqrt(T) 2^-26 (include/prcore.h).  ``taps_out`` complex128 [nblocks][T], ``sv_out`` float64 [nblocks][T],
    ``info_out`` int32 [nblocks][3] (kept, sweeps, converged); ``workspace``: ls_svd_workspace_bytes(...) device bytes.
    Synchronises ``stream`` once per Jacobi sweep."""
    check(lib().prc_ls_svd_execute(_ptr(ref), _ptr(srv), int(n), int(n if stride is None else stride), int(filter_len),
                                   int(peek), -1.0 if rcond is None else float(rcond), int(nblocks), _ptr(out),
                                   int(n if out_stride is None else out_stride), _ptr(taps_out), _ptr(sv_out),
                                   _ptr(info_out), _ptr(workspace), stream))


def ls_svd_set_profiling(enable=True):
    check(lib().prc_ls_svd_set_profiling(int(bool(enable))))


def ls_svd_get_profile():
    """((ms_correlate, ms_jacobi, ms_taps, ms_apply), sweeps launched) of the last ls_svd_execute under set_profiling"""
    ms = (C.c_double * 4)()
    k = C.c_int32()
    check(lib().prc_ls_svd_get_profile(ms, C.byref(k)))
    return tuple(ms), k.value


def eca_workspace_bytes(n, filter_len, peek=10, nbins=1, nblocks=1):
    """device bytes prc_eca_execute needs for ``nblocks`` blocks of ``n`` samples, ``nbins`` bins and filter_len + peek taps each"""
    nb = C.c_size_t(0)
    check(lib().prc_eca_workspace_bytes(int(n), int(filter_len), int(peek), int(nbins), int(nblocks), C.byref(nb)))
    return int(nb.value)


def eca_execute(ref, srv, out, n, filter_len, peek=10, sample_rate=1.0, doppler_bins=(0,), reg=0.0, nblocks=1, stride=None,
                out_stride=None, taps_out=None, info_out=None, workspace=None, stream=None):
    """ECA_Filter over ``nblocks`` independent blocks (device buffers or torch tensors): the taps of every Doppler bin from one
    least-squares problem (include/prcore.h).  ``taps_out`` complex128 [nblocks][nbins][T], ``info_out`` int32 [nblocks] (1: the
    block's recursion broke down, its taps are zero and out = srv); ``workspace``: eca_workspace_bytes(...) device bytes.
    Neither allocates nor synchronises."""
    bins = (C.c_double * max(len(doppler_bins), 1))(*[float(b) for b in doppler_bins])
    check(lib().prc_eca_execute(_ptr(ref), _ptr(srv), int(n), int(n if stride is None else stride), int(filter_len), int(peek),
                                float(sample_rate), bins, len(doppler_bins), float(reg), int(nblocks), _ptr(out),
                                int(n if out_stride is None else out_stride), _ptr(taps_out), _ptr(info_out), _ptr(workspace),
                                stream))


def eca_set_profiling(enable=True):
    check(lib().prc_eca_set_profiling(int(bool(enable))))


def eca_get_profile():
    """(ms_correlate, ms_solve, ms_apply) of the last eca_execute under set_profiling"""
    ms = (C.c_double * 3)()
    check(lib().prc_eca_get_profile(ms))
    return tuple(ms)


def patch_desc(n, nlags, ndoppler, sample_rate, doppler_step, wrap=True, nframes=1, frame_stride=None):
    """prc_patch_desc of include/prcore.h"""
    d = _lib.PatchDesc()
    d.n, d.frame_stride, d.nframes = int(n), int(n if frame_stride is None else frame_stride), int(nframes)
    d.nlags, d.ndoppler, d.wrap = int(nlags), int(ndoppler), int(bool(wrap))
    d.sample_rate, d.doppler_step = float(sample_rate), float(doppler_step)
    return d


def xambg_patch_workspace_bytes(desc, npatches):
    """device bytes prc_xambg_patch needs in ``workspace`` for ``npatches`` patches of desc's shape"""
    nb = C.c_size_t(0)
    check(lib().prc_xambg_patch_workspace_bytes(C.byref(desc), int(npatches), C.byref(nb)))
    return int(nb.value)


def xambg_patch_execute(desc, ref, srv, window, patches, npatches, out, workspace, stream=None):
    """exact cross-ambiguity patches (device buffers or torch tensors; ``patches``: DEVICE prc_patch records)"""
    check(lib().prc_xambg_patch(C.byref(desc), _ptr(ref), _ptr(srv), _ptr(window), _ptr(patches), int(npatches), _ptr(out),
                                _ptr(workspace), stream))


def xambg_patch_peaks(desc, patches, npatches, X, peaks, stream=None):
    """argmax + parabolic refinement per patch (``peaks``: DEVICE prc_patch_peak records)"""
    check(lib().prc_xambg_patch_peaks(C.byref(desc), _ptr(patches), int(npatches), _ptr(X), _ptr(peaks), stream))


def patch_list(lags, dopplers, frame=None, nframes=1, n=None):
    """HOST prc_patch records from patch origins, validated as the header asks of a host-built list: ValueError for a
    frame outside [0, nframes), |lag0| >= n or a Doppler that is not finite"""
    lags = np.atleast_1d(np.asarray(lags))
    dopplers = np.atleast_1d(np.asarray(dopplers, dtype=np.float64))
    if lags.ndim != 1 or lags.shape != dopplers.shape:
        raise ValueError("lags and dopplers must be one-dimensional and of the same length")
    if lags.size and not np.all(lags == np.rint(lags)):
        raise ValueError("patch lags are whole samples")
    frames = np.zeros(lags.shape, np.int64) if frame is None else np.broadcast_to(np.asarray(frame, dtype=np.int64), lags.shape)
    if np.any(frames < 0) or np.any(frames >= nframes):
        raise ValueError(f"patch frame outside [0, {nframes})")
    if n is not None and np.any(np.abs(lags.astype(np.int64)) >= n):
        raise ValueError(f"patch lag origin outside (-{n}, {n})")
    if not np.all(np.isfinite(dopplers)):
        raise ValueError("patch Doppler origins must be finite")
    rec = np.zeros(lags.shape[0], dtype=_lib.PATCH_DTYPE)
    rec["frame"], rec["lag0"], rec["doppler0"] = frames, lags.astype(np.int64), dopplers
    return rec


def echo_desc(n, sample_rate, max_atoms, nframes=1, wrap=False, ramp=True, refine=2, reg=0.0, frame_stride=None, out_stride=None):
    """prc_echo_desc of include/prcore.h, validated on the host (ValueError) before a device is touched"""
    d = _lib.EchoDesc()
    d.n, d.nframes, d.max_atoms = int(n), int(nframes), int(max_atoms)
    d.frame_stride = int(n if frame_stride is None else frame_stride)
    d.out_stride = int(n if out_stride is None else out_stride)
    d.wrap, d.ramp, d.refine = int(bool(wrap)), int(bool(ramp)), int(refine)
    d.sample_rate, d.reg = float(sample_rate), float(reg)
    echo_workspace_bytes(d)
    return d


def echo_workspace_bytes(desc):
    """device bytes prc_echo_cancel needs in ``workspace``; every descriptor check of prc_echo_cancel (host arithmetic)"""
    nb = C.c_size_t(0)
    check(lib().prc_echo_cancel_workspace_bytes(C.byref(desc), C.byref(nb)))
    return int(nb.value)


def echo_execute(desc, ref, srv, atoms, counts, out, fit, info, workspace, stream=None):
    """joint least-squares removal of the listed echoes (device buffers or torch tensors; ``atoms``: DEVICE prc_echo_atom
    [nframes][max_atoms], ``counts``: int32 [nframes], ``fit``: DEVICE prc_echo_fit records, ``info``: int32 [nframes]).
    Neither allocates nor synchronises."""
    check(lib().prc_echo_cancel(C.byref(desc), _ptr(ref), _ptr(srv), _ptr(atoms), _ptr(counts), _ptr(out), _ptr(fit), _ptr(info),
                                _ptr(workspace), stream))


def cfar_training_cells(fw, gw):
    """training cells of CFAR_2D's (fw, gw) window: fw^2 - (e2 - e1)^2 (prc_cfar_training_cells; host arithmetic)"""
    n = C.c_int32(0)
    check(lib().prc_cfar_training_cells(int(fw), int(gw), C.byref(n)))
    return int(n.value)


def cfar_os_desc(H, W, fw, gw, rank=None, scale="reference", complex_input=False, thresh=None):
    """prc_cfar_os_desc of include/prcore.h (rank None: the library's default, ceil(0.75 Nt))"""
    if scale not in _lib.CFAR_SCALES:
        raise ValueError(f"scale is one of {sorted(_lib.CFAR_SCALES)}, not {scale!r}")
    if rank is not None and int(rank) < 1:
        raise ValueError("rank counts from 1")
    d = _lib.CfarOsDesc()
    d.H, d.W, d.fw, d.gw = int(H), int(W), int(fw), int(gw)
    d.rank = 0 if rank is None else int(rank)
    d.scale, d.input = _lib.CFAR_SCALES[scale], int(bool(complex_input))
    d.use_thresh, d.thresh = int(thresh is not None), float(thresh or 0.0)
    return d


def cfar_os_workspace_bytes(desc, nframes):
    """device bytes prc_cfar_os needs in ``workspace`` (0 for the plain scale); validates the descriptor on the host"""
    nb = C.c_size_t(0)
    check(lib().prc_cfar_os_workspace_bytes(C.byref(desc), int(nframes), C.byref(nb)))
    return int(nb.value)


def cfar_os_execute(desc, X, out, noise, nframes, workspace, stream=None):
    """order-statistic CFAR of a stack (device buffers or torch tensors; ``noise`` and, for the plain scale, ``workspace``
    may be None)"""
    check(lib().prc_cfar_os(C.byref(desc), _ptr(X), _ptr(out), _ptr(noise), int(nframes), _ptr(workspace), stream))


def plots_desc(H, W, thresh, frame_extent, connectivity=8, range_guard=8, doppler_guard=4, max_cells=None, capacity=512,
               complex_weight=False):
    """prc_plots_desc of include/prcore.h (max_cells None: PRC_PLOTS_LDS_CELLS, the most the LDS path holds)"""
    d = _lib.PlotsDesc()
    d.H, d.W, d.connectivity = int(H), int(W), int(connectivity)
    d.range_guard, d.doppler_guard = int(range_guard), int(doppler_guard)
    d.max_cells = _lib.PLOTS_LDS_CELLS if max_cells is None else int(max_cells)
    d.capacity, d.weight_input, d.thresh = int(capacity), int(bool(complex_weight)), float(thresh)
    d.doppler_extent, d.range_extent = float(frame_extent[0]), float(frame_extent[1])
    return d


def plots_workspace_bytes(desc, nframes):
    """device bytes prc_plots needs in ``workspace`` (0 up to PRC_PLOTS_LDS_CELLS cells); validates the descriptor on the host"""
    nb = C.c_size_t(0)
    check(lib().prc_plots_workspace_bytes(C.byref(desc), int(nframes), C.byref(nb)))
    return int(nb.value)


def plots_execute(desc, stat, weight, nframes, counts, ncells, cands, info, workspace, stream=None):
    """plot extraction of a stack (device buffers or torch tensors; ``weight``, ``info`` and, on the LDS path, ``workspace``
    may be None)"""
    check(lib().prc_plots(C.byref(desc), _ptr(stat), _ptr(weight), int(nframes), _ptr(counts), _ptr(ncells), _ptr(cands),
                          _ptr(info), _ptr(workspace), stream))


def tbd_desc(H, W, alpha=0.9, doppler_reach=1, range_reach=1, clip=None, range_guard=8, doppler_guard=4):
    """prc_tbd_desc of include/prcore.h (clip None: +Inf, no clipping)"""
    d = _lib.TbdDesc()
    d.H, d.W, d.doppler_reach, d.range_reach = int(H), int(W), int(doppler_reach), int(range_reach)
    d.range_guard, d.doppler_guard = int(range_guard), int(doppler_guard)
    d.alpha, d.clip = float(alpha), float("inf") if clip is None else float(clip)
    return d


def tbd_execute(desc, stat, row_shift, prev, nframes, score, back, stream=None, frames_per_launch=None, band_rows=None):
    """track-before-detect scores (and back pointers) of a stack (device buffers or torch tensors; ``row_shift``, ``prev`` and
    ``back`` may be None).  ``frames_per_launch`` / ``band_rows`` (tests and tools only) set PRC_OPT_TBD_FRAMES /
    PRC_OPT_TBD_ROWS for this call: 1 = one frame per launch, 2 .. 32 = the time-blocked form; the bytes out do not change."""
    old = []
    try:
        for opt, v in ((_lib.OPT_TBD_FRAMES, frames_per_launch), (_lib.OPT_TBD_ROWS, band_rows)):
            if v is not None:
                old.append((opt, _lib.set_option(opt, v)))
        check(lib().prc_tbd(C.byref(desc), _ptr(stat), _ptr(row_shift), _ptr(prev), int(nframes), _ptr(score), _ptr(back), stream))
    finally:
        for opt, v in old:
            _lib.set_option(opt, v)


def tbd_trace(desc, back, row_shift, nframes, ends, nends, depth, paths, stream=None):
    """paths [nends][depth] of storage cells read back through ``back`` from ``ends`` [nends][2] = (frame, cell); -1 from
    where a path stops"""
    check(lib().prc_tbd_trace(C.byref(desc), _ptr(back), _ptr(row_shift), int(nframes), _ptr(ends), int(nends), int(depth),
                              _ptr(paths), stream))


def fuse_desc(nillum, H, W, grid, velocities, rx, z=0.0, combine=_lib.FUSE_SUM, form=None):
    """prc_fuse_desc of include/prcore.h: ``grid`` = (x0, dx, nx, y0, dy, ny), ``velocities`` = (vx0, dvx, nvx, vy0, dvy, nvy),
    ``rx`` the receiver's three coordinates; form None: the shipped choice"""
    d = _lib.FuseDesc()
    d.nillum, d.H, d.W = int(nillum), int(H), int(W)
    d.x0, d.dx, d.nx, d.y0, d.dy, d.ny = float(grid[0]), float(grid[1]), int(grid[2]), float(grid[3]), float(grid[4]), int(grid[5])
    d.vx0, d.dvx, d.nvx = float(velocities[0]), float(velocities[1]), int(velocities[2])
    d.vy0, d.dvy, d.nvy = float(velocities[3]), float(velocities[4]), int(velocities[5])
    d.z, d.combine, d.form = float(z), int(combine), _lib.FUSE_FORM_AUTO if form is None else int(form)
    d.rx[0], d.rx[1], d.rx[2] = (float(v) for v in rx)
    return d


def fuse_execute(desc, illum, stat, illum_stride, frame_stride, nframes, best, vel, stream=None):
    """prc_fuse: ``illum`` is a host float64 array [nillum, 9] (None only passes the null pointer on); ``stat``, ``best`` and
    ``vel`` are device buffers or torch tensors (``vel`` may be None); the strides are in elements"""
    if illum is not None:
        illum = np.ascontiguousarray(illum, dtype=np.float64)
        ip = illum.ctypes.data_as(C.POINTER(C.c_double))
    else:
        ip = None
    check(lib().prc_fuse(C.byref(desc), ip, _ptr(stat), int(illum_stride), int(frame_stride), int(nframes), _ptr(best), _ptr(vel),
                         stream))


def batch_xambg_desc(n, batch_len, range_bins, freq_bins, hop=None, start=0, filter=_lib.BATCH_RECIPROCAL, floor=0.1):
    """prc_batch_xambg_desc of include/prcore.h (hop None: batch_len, batches end to end)"""
    d = _lib.BatchXambgDesc()
    d.n, d.start, d.hop = int(n), int(start), int(batch_len if hop is None else hop)
    d.batch_len, d.range_bins, d.freq_bins = int(batch_len), int(range_bins), int(freq_bins)
    d.filter, d.floor = int(filter), float(floor)
    return d


def batch_xambg_workspace_bytes(desc, nframes):
    """device bytes prc_batch_xambg needs in ``workspace`` (its slow-time buffer); validates the descriptor on the host"""
    nb = C.c_size_t(0)
    check(lib().prc_batch_xambg_workspace_bytes(C.byref(desc), int(nframes), C.byref(nb)))
    return int(nb.value)


def batch_xambg_execute(desc, ref, srv, frame_stride, window, out, nframes, workspace, stream=None):
    """batches-algorithm surfaces of ``nframes`` frames (device buffers or torch tensors; ``window`` may be None)"""
    check(lib().prc_batch_xambg(C.byref(desc), _ptr(ref), _ptr(srv), int(frame_stride), _ptr(window), _ptr(out), int(nframes),
                                _ptr(workspace), stream))


def ofdm_timing(ref, n, nfft, cp, nsym, metric, start, stream=None):
    """prc_ofdm_timing: the cyclic-prefix metric (device float64 [nfft + cp]) and its argmax (device int32) of ``ref``"""
    check(lib().prc_ofdm_timing(_ptr(ref), int(n), int(nfft), int(cp), int(nsym), _ptr(metric), _ptr(start), stream))


# ---- per-thread plan cache (dask-style concurrent callers each get their own plans) ------
_tls = threading.local()


def cached_plan(key, factory, limit=8, stream=None):
    """One plan per (thread, device, stream, shape key): a plan's workspaces live on the device that was current
    when it was made, and its single slow-time / tap workspace must not be shared by launches on two streams."""
    key = (_lib.current_device(), getattr(stream, "value", stream)) + tuple(key)
    cache = getattr(_tls, "plans", None)
    if cache is None:
        cache = _tls.plans = {}
    plan = cache.get(key)
    if plan is None:
        if len(cache) >= limit:
            old_key = next(iter(cache))
            cache.pop(old_key).close()
        plan = cache[key] = factory()
    return plan


class Staging:
    """Per-thread grow-only device scratch for the NumPy-facing functions."""

    def __init__(self):
        self.bufs = {}

    def get(self, name, nbytes):
        b = self.bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.bufs[name] = _lib.DeviceBuffer(nbytes)
        return b


def staging():
    """per thread and per device"""
    per_dev = getattr(_tls, "staging", None)
    if per_dev is None:
        per_dev = _tls.staging = {}
    dev = _lib.current_device()
    st = per_dev.get(dev)
    if st is None:
        st = per_dev[dev] = Staging()
    return st
