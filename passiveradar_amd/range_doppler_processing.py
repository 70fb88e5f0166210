"""Drop-in for the reference's ``passiveRadar/range_doppler_processing.py`` on MI355X.

``fast_xambg`` keeps the reference signature, argument meaning, return shape/dtype and the
ValueError on mismatched inputs (range_doppler_processing.py:12-90) and runs on the HIP kernels
behind libprcore.so.  Inputs may be NumPy arrays (staged to the GPU and back) or torch device
tensors (zero copy, result returned as a torch tensor on the same device).
"""
from __future__ import annotations

import functools

import numpy as np

from . import _lib, engine, residence

__all__ = ["fast_xambg", "fast_xambg_multi", "direct_xambg", "caf_plan_for", "set_default_methods", "xambg_patch",
           "patch_origins", "clean_xambg", "batch_xambg", "ofdm_symbol_start"]

# Kernel selection used by fast_xambg (0 = let the plan decide).  Not part of the reference
# signature; tests flip it to run the same cases through every kernel family.
_DEFAULTS = {"caf": _lib.CAF_AUTO, "doppler": _lib.DOPPLER_AUTO}


def set_default_methods(caf=None, doppler=None):
    """caf: 0 auto | 1 direct | 2 fft (1024-point) | 3 fft (4096-point team);
    doppler: 0 auto | 1 transpose + rocfft + shift | 2 one column-FFT kernel (freq_bins 256..4096, powers of two)."""
    if caf is not None:
        _DEFAULTS["caf"] = int(caf)
    if doppler is not None:
        _DEFAULTS["doppler"] = int(doppler)


@functools.lru_cache(maxsize=16)
def _named_window(spec, n):
    # range_doppler_processing.py:57-58 -- host side, computed once per (spec, length)
    from scipy.signal import get_window
    return np.ascontiguousarray(get_window(spec, n), dtype=np.float32)


@functools.lru_cache(maxsize=4)
def _long_taps(q):
    # range_doppler_processing.py:76 -- flat-top FIR of 10q+1 taps (shortFilt=False)
    from scipy.signal import firwin
    return np.ascontiguousarray(firwin(10 * q + 1, 1.0 / q, window="flattop"), dtype=np.float32)


def caf_plan_for(n, rangeBins, freqBins, shortFilt=True, max_frames=1, method=None, doppler=None, stream=None,
                 multi=_lib.CAF_MULTI_AUTO):
    method = _DEFAULTS["caf"] if method is None else method
    doppler = _DEFAULTS["doppler"] if doppler is None else doppler
    if not shortFilt and (method == _lib.CAF_FFT4096 or (method == _lib.CAF_FFT and rangeBins + 1 > 769)):
        method = _lib.CAF_AUTO          # the long FIR runs on the 1024-point FFT kernel up to 769 lags, else time-domain
    q = int(n / freqBins) if freqBins else 0
    multi = _lib.CAF_MULTI_MODES[multi] if isinstance(multi, str) else int(multi)
    # plans copy the process-wide options when they are made: a cached plan must not outlive a change of them
    opts = (_lib.get_option(_lib.OPT_CAF_MULTI_MODE), _lib.get_option(_lib.OPT_CAF_GROUP_MB))
    key = ("caf", n, rangeBins, freqBins, bool(shortFilt), max_frames, method, doppler, multi) + opts
    taps = None if shortFilt else _long_taps(q)
    return engine.cached_plan(key, lambda: engine.CafPlan(n, rangeBins, freqBins, max_frames,
                                                          method, doppler, taps, multi), stream=stream)


def fast_xambg(refChannel, srvChannel, rangeBins, freqBins, inputLen=None, window=None,
               shortFilt=True):
    """Fast cross-ambiguity function (same contract as the reference, :12-90).

    Returns an array of shape (freqBins, rangeBins+1, 1), complex64: column k is delay
    rangeBins-k samples, rows are fftshift-ed Doppler bins.
    """
    if tuple(refChannel.shape) != tuple(srvChannel.shape):                  # :46-49
        raise ValueError("Input vectors must have the same length")
    n_in = int(refChannel.shape[0])
    n = n_in if inputLen is None else int(inputLen)
    if n_in > n:
        raise ValueError("index can't contain negative values")              # np.pad at :53
    if isinstance(window, (tuple, str)):
        window = _named_window(window, n)
    elif window is not None and not _lib.is_device_tensor(window):
        window = np.ascontiguousarray(window, dtype=np.float32)
        if window.shape[0] != n:
            raise ValueError(f"operands could not be broadcast together with shapes ({n},) "
                             f"({window.shape[0]},)")
    if _lib.is_device_tensor(refChannel):
        import torch
        # everything on the tensors' own device and on torch's current stream THERE (not on whatever device
        # happens to be current): the plan, its workspaces and the launch
        with torch.cuda.device(refChannel.device):
            st = _lib.torch_stream_ptr(refChannel.device)
            plan = caf_plan_for(n, int(rangeBins), int(freqBins), shortFilt, stream=st)
            ref = refChannel.to(torch.complex64).contiguous()
            srv = srvChannel.to(device=ref.device, dtype=torch.complex64).contiguous()
            win = None
            if window is not None:
                win = window if _lib.is_device_tensor(window) else torch.from_numpy(window)
                win = win.to(device=ref.device, dtype=torch.float32).contiguous()
            out = torch.empty((int(freqBins), int(rangeBins) + 1, 1), dtype=torch.complex64,
                              device=ref.device)
            plan.execute(ref, srv, out, 1, n, n_in, win, stream=st)
        return out

    plan = caf_plan_for(n, int(rangeBins), int(freqBins), shortFilt)
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64)   # complex128 srv is narrowed
    st = engine.staging()
    d_ref = st.get("caf_ref", 8 * n_in)
    d_srv = st.get("caf_srv", 8 * n_in)
    d_out = st.get("caf_out", 8 * int(freqBins) * (int(rangeBins) + 1))
    d_ref.upload(ref)
    d_srv.upload(srv)
    d_win = None
    if window is not None:
        d_win = st.get("caf_win", 4 * n)
        d_win.upload(window)
    plan.execute(d_ref, d_srv, d_out, 1, n, n_in, d_win)
    return d_out.download((int(freqBins), int(rangeBins) + 1, 1), np.complex64)


def direct_xambg(refChannel, srvChannel, rangeBins, freqBins, sampleRate):
    """Direct (time-domain) cross-ambiguity function, range_doppler_processing.py:93-124: for every Doppler bin i the
    reference is shifted by (i - freqBins/2) / CPI Hz (frequency_shift, float32 phase ramp) and correlated with the
    surveillance channel at lags 0..rangeBins (xcorr).  The reference never calls it on its processing path (SURVEY 8a:
    an independent peak check); it is here so that swapping the import line never raises.  A thin composition of
    prc_frequency_shift + prc_xcorr on device buffers: both channels go up once, the surface comes down once.

    Returns (freqBins, rangeBins+1, 1) complex64; row i is Doppler (i - freqBins/2)/CPI (NOT mirrored like
    fast_xambg's rows), column k is delay rangeBins - k."""
    if tuple(refChannel.shape) != tuple(srvChannel.shape):                  # :107-108
        raise ValueError("Input vectors must have the same length")
    ref = np.ascontiguousarray(refChannel.cpu().numpy() if _lib.is_device_tensor(refChannel) else refChannel, dtype=np.complex64)
    srv = np.ascontiguousarray(srvChannel.cpu().numpy() if _lib.is_device_tensor(srvChannel) else srvChannel, dtype=np.complex64)
    if ref.ndim != 1:
        raise ValueError("direct_xambg takes one-dimensional channels")
    n, R, F = ref.shape[0], int(rangeBins), int(freqBins)
    if R < 0:
        raise ValueError("index can't contain negative values")              # np.pad inside xcorr
    cpi = n / sampleRate                                                     # :111
    st = engine.staging()
    d_ref = st.get("dx_ref", 8 * n)
    d_srv = st.get("dx_srv", 8 * n)
    d_shift = st.get("dx_shift", 8 * n)
    d_out = st.get("dx_out", 8 * max(F, 1) * (R + 1))
    d_ref.upload(ref)
    d_srv.upload(srv)
    L = _lib.lib()
    for i in range(F):
        df = (i - 0.5 * F) / cpi                                             # :119
        _lib.check(L.prc_frequency_shift(d_ref.ptr, d_shift.ptr, n, float(df), float(sampleRate), 0.0, None))
        _lib.check(L.prc_xcorr(d_shift.ptr, d_srv.ptr, n, R, 0, d_out.ptr + 8 * i * (R + 1), None))   # :123
    return d_out.download((F, R + 1, 1), np.complex64)


def fast_xambg_multi(refChannels, srvChannel, rangeBins, freqBins, inputLen=None, window=None, shortFilt=True,
                     mode="auto"):
    """``[fast_xambg(r, srvChannel, ...) for r in refChannels]`` in one call: several illuminators against ONE
    surveillance channel (BASELINE config 5).  The reference calls fast_xambg once per (reference, surveillance) pair
    (range_doppler_processing.py:12-90); the pairs of one frame share the surveillance channel and the window, so the
    device can transform the surveillance pieces once per segment for all of them (prc_caf_execute_multi; ``mode``:
    "auto" = the library's measured choice, "turns" = one single-reference pass per illuminator, "shared" / "pairs" =
    surveillance spectra shared by all / by pairs of illuminators -- prc_caf_desc.multi).  Same argument
    meaning, errors and per-surface result as fast_xambg; returns a list of (freqBins, rangeBins+1, 1) complex64."""
    refs = list(refChannels)
    if not refs:
        return []
    if len(refs) > _lib.CAF_MAX_REFS:
        out = []
        for i in range(0, len(refs), _lib.CAF_MAX_REFS):
            out += fast_xambg_multi(refs[i:i + _lib.CAF_MAX_REFS], srvChannel, rangeBins, freqBins, inputLen, window,
                                    shortFilt, mode)
        return out
    for r in refs:
        if tuple(r.shape) != tuple(srvChannel.shape):                         # :46-49
            raise ValueError("Input vectors must have the same length")
    n_in = int(srvChannel.shape[0])
    n = n_in if inputLen is None else int(inputLen)
    if n_in > n:
        raise ValueError("index can't contain negative values")
    if isinstance(window, (tuple, str)):
        window = _named_window(window, n)
    elif window is not None and not _lib.is_device_tensor(window):
        window = np.ascontiguousarray(window, dtype=np.float32)
        if window.shape[0] != n:
            raise ValueError(f"operands could not be broadcast together with shapes ({n},) ({window.shape[0]},)")
    nref, F, R = len(refs), int(freqBins), int(rangeBins)
    if _lib.is_device_tensor(srvChannel):
        import torch
        dev = srvChannel.device
        with torch.cuda.device(dev):
            st = _lib.torch_stream_ptr(dev)
            plan = caf_plan_for(n, R, F, shortFilt, max_frames=nref, stream=st, multi=mode)
            srv = srvChannel.to(torch.complex64).contiguous()
            rr = [r.to(device=dev, dtype=torch.complex64).contiguous() for r in refs]
            win = None
            if window is not None:
                win = window if _lib.is_device_tensor(window) else torch.from_numpy(window)
                win = win.to(device=dev, dtype=torch.float32).contiguous()
            outs = [torch.empty((F, R + 1, 1), dtype=torch.complex64, device=dev) for _ in refs]
            plan.execute_multi(rr, srv, outs, 1, n, n_in, win, stream=st)
        return outs
    plan = caf_plan_for(n, R, F, shortFilt, max_frames=nref, multi=mode)
    st = engine.staging()
    d_srv = st.get("caf_srv", 8 * n_in)
    d_srv.upload(np.ascontiguousarray(srvChannel, dtype=np.complex64))
    d_refs = st.get("caf_refs", 8 * n_in * nref)
    d_outs = st.get("caf_outs", 8 * F * (R + 1) * nref)
    for i, r in enumerate(refs):
        d_refs.upload(np.ascontiguousarray(r, dtype=np.complex64), offset_bytes=8 * n_in * i)
    d_win = None
    if window is not None:
        d_win = st.get("caf_win", 4 * n)
        d_win.upload(window)
    plan.execute_multi([d_refs.ptr + 8 * n_in * i for i in range(nref)], d_srv,
                       [d_outs.ptr + 8 * F * (R + 1) * i for i in range(nref)], 1, n, n_in, d_win)
    return [d_outs.download((F, R + 1, 1), np.complex64, offset_bytes=8 * F * (R + 1) * i) for i in range(nref)]


def patch_origins(rows, cols, rangeBins, freqBins, n, sampleRate, nlags, ndoppler, doppler_step):
    """(lags, dopplers): the origins that centre an ``ndoppler`` x ``nlags`` patch of spacing ``doppler_step`` on the
    ``fast_xambg`` cells (rows, cols).  Cell (row, col) is lag rangeBins - col and -- rows are mirrored and fftshift-ed --
    Doppler (freqBins/2 - row) / CPI (scene.expected_peak_cell is the inverse); the centre is patch cell
    (ndoppler // 2, nlags // 2).  Host arithmetic only."""
    rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int64))
    cpi = n / float(sampleRate)
    lags = (int(rangeBins) - cols) - int(nlags) // 2
    dopplers = (0.5 * int(freqBins) - rows) / cpi - (int(ndoppler) // 2) * float(doppler_step)
    return lags, dopplers


def xambg_patch(refChannel, srvChannel, sampleRate, lags, dopplers, nlags=16, ndoppler=16, doppler_step=None, window=None,
                wrap=True, frame=None):
    """Exact (un-decimated) cross-ambiguity function on lag x Doppler patches -- the "zoom" step after a detector:

        X[p, d, l] = sum_i w[i] ref[i] conj(srv[idx(i + lags[p] + l)]) exp(+j 2 pi (dopplers[p] + d doppler_step) i / sampleRate)

    ``wrap=True``: idx(m) = m mod n (fast_xambg's np.roll convention, negative lags allowed); ``wrap=False``: terms outside
    the frame are dropped (direct_xambg / xcorr).  An echo srv[i] = ref[i - D] exp(+j 2 pi f i / Fs) peaks at lag D, Doppler
    +f: direct_xambg's row sense, the mirror of fast_xambg's rows (``patch_origins`` maps fast_xambg cells to origins).  No
    decimator, so no droop, and the phase is exact (no float32 ramp): prc_xambg_patch of include/prcore.h.

    Channels are 1-D or [nframes, n] stacks, NumPy (staged) or torch device tensors (zero copy, on torch's current stream,
    nothing returns to the host; a row-strided view is taken as it is).  ``frame``: frame index per patch (default 0).
    ``doppler_step=None``: 0.25 sampleRate / n, a quarter of a fast_xambg cell.  ``window``: as fast_xambg's.
    Returns complex64 [npatches, ndoppler, nlags]."""
    if tuple(refChannel.shape) != tuple(srvChannel.shape):
        raise ValueError("Input vectors must have the same length")
    if len(refChannel.shape) not in (1, 2):
        raise ValueError("xambg_patch takes one-dimensional channels or [nframes, n] stacks")
    n = int(refChannel.shape[-1])
    nframes = 1 if len(refChannel.shape) == 1 else int(refChannel.shape[0])
    if n < 1 or nframes < 1:
        raise ValueError("xambg_patch: empty channels")
    nlags, ndoppler = int(nlags), int(ndoppler)
    step = 0.25 * float(sampleRate) / n if doppler_step is None else float(doppler_step)
    if isinstance(window, (tuple, str)):
        window = _named_window(window, n)
    elif window is not None and not _lib.is_device_tensor(window):
        window = np.ascontiguousarray(window, dtype=np.float32)
    if window is not None and (len(window.shape) != 1 or window.shape[0] != n):
        raise ValueError(f"operands could not be broadcast together with shapes ({n},) {tuple(window.shape)}")
    rec = engine.patch_list(lags, dopplers, frame, nframes, n)
    npatches = rec.shape[0]
    if _lib.is_device_tensor(refChannel):
        import torch
        with torch.cuda.device(refChannel.device):
            st = _lib.torch_stream_ptr(refChannel.device)
            ref = refChannel.to(torch.complex64)
            srv = srvChannel.to(device=ref.device, dtype=torch.complex64)
            stride = n
            if nframes > 1:
                # one stride for both: a row-strided view of a larger buffer stays where it is
                if not (ref.stride(1) == 1 and srv.stride(1) == 1 and ref.stride(0) == srv.stride(0) and ref.stride(0) >= n):
                    ref, srv = ref.contiguous(), srv.contiguous()
                stride = ref.stride(0)
            else:
                ref, srv = ref.contiguous(), srv.contiguous()
            desc = engine.patch_desc(n, nlags, ndoppler, sampleRate, step, wrap, nframes, stride)
            nws = engine.xambg_patch_workspace_bytes(desc, npatches)
            out = torch.empty((npatches, ndoppler, nlags), dtype=torch.complex64, device=ref.device)
            if npatches == 0:
                return out
            win = None
            if window is not None:
                win = window if _lib.is_device_tensor(window) else torch.from_numpy(window)
                win = win.to(device=ref.device, dtype=torch.float32).contiguous()
            d_rec = torch.from_numpy(rec.view(np.uint8)).to(ref.device)
            ws = torch.empty(nws, dtype=torch.uint8, device=ref.device)
            engine.xambg_patch_execute(desc, ref, srv, win, d_rec, npatches, out, ws, st)
        return out
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64)
    desc = engine.patch_desc(n, nlags, ndoppler, sampleRate, step, wrap, nframes, n)
    nws = engine.xambg_patch_workspace_bytes(desc, npatches)
    if npatches == 0:
        return np.zeros((0, ndoppler, nlags), np.complex64)
    _lib.require_gpu()
    st = engine.staging()
    d_ref = st.get("xp_ref", ref.nbytes)
    d_srv = st.get("xp_srv", srv.nbytes)
    d_rec = st.get("xp_rec", rec.nbytes)
    d_out = st.get("xp_out", 8 * npatches * ndoppler * nlags)
    d_ws = st.get("xp_ws", nws)
    d_ref.upload(ref)
    d_srv.upload(srv)
    d_rec.upload(rec.view(np.uint8))
    d_win = None
    if window is not None:
        d_win = st.get("xp_win", 4 * n)
        d_win.upload(window)
    engine.xambg_patch_execute(desc, d_ref, d_srv, d_win, d_rec, npatches, d_out, d_ws)
    return d_out.download((npatches, ndoppler, nlags), np.complex64)


# the records clean_xambg returns: one per atom it removed
ECHO_RECORD_DTYPE = np.dtype([("lag", "<i4"), ("doppler", "<f8"), ("amplitude", "<c16")])


def _strongest_cells(mag, npeaks, doppler_guard, half_rows, half_cols):
    """(rows, cols) of the ``npeaks`` strongest cells of |X| [F, R + 1] outside the +-doppler_guard rows around zero Doppler
    (row F // 2), one per neighbourhood: a picked cell takes the box of +-half_rows x +-half_cols around it out of the
    running.  ``mag`` is a NumPy array or a device tensor (then only the picked indices come to the host: one small copy)."""
    F, W = (int(v) for v in mag.shape)
    lo, hi = max(F // 2 - doppler_guard, 0), F // 2 + doppler_guard + 1
    if _lib.is_device_tensor(mag):
        import torch
        m = mag.clone()
        if doppler_guard >= 0:
            m[lo:hi, :] = -1.0
        ri, ci = torch.arange(F, device=m.device), torch.arange(W, device=m.device)
        picked = []
        for _ in range(int(npeaks)):
            k = m.argmax()
            picked.append(k)
            box = ((ri - k // W).abs() <= half_rows)[:, None] & ((ci - k % W).abs() <= half_cols)[None, :]
            m.masked_fill_(box, -1.0)
        picked = torch.stack(picked).cpu().numpy().astype(np.int64)
        return picked // W, picked % W
    m = np.array(mag, dtype=np.float32)
    if doppler_guard >= 0:
        m[lo:hi, :] = -1.0
    rows, cols = [], []
    for _ in range(int(npeaks)):
        r, c = divmod(int(m.argmax()), W)
        rows.append(r)
        cols.append(c)
        m[max(r - half_rows, 0):r + half_rows + 1, max(c - half_cols, 0):c + half_cols + 1] = -1.0
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)


def clean_xambg(ref, srv, sampleRate, rangeBins, freqBins, *, npeaks=4, doppler_guard=2, lag_span=0, patch=(16, 16),
                oversample=4, **cancel_kw):
    """The range-Doppler surface with its strongest echoes removed from the surveillance stream first (CLEAN): a strong
    moving echo of a noise-like illuminator lifts the whole surface by 1 / sqrt(B T) of its peak and hides every weaker
    target under it.  Steps: (1) ``fast_xambg`` of the raw stream; (2) the ``npeaks`` strongest cells outside the
    +-``doppler_guard`` rows around zero Doppler (what stands there is the cancellers' business; a negative guard keeps every
    row), one per patch-sized neighbourhood -- this needs one small device-to-host copy, the picked cell indices (the peak
    records of step 4 and cancel_echoes' breakdown flags and fit are small copies of the same kind: the atom list is built on
    the host); (3) patches of
    ``patch`` = (Doppler rows, lags) at 1 / ``oversample`` of a cell, centred on them (``patch_origins``); (4) ``xambg_patch``
    and ``refine_peaks`` give each echo's lag and sub-cell Doppler; (5) ``cancel_echoes`` fits and subtracts them (``cancel_kw``:
    ramp, refine, reg, wrap); (6) ``fast_xambg`` of the cleaned stream.  ``lag_span`` = h adds atoms at lags D - h .. D + h
    around each echo, for oversampled signals whose echoes fall between samples; npeaks (2 h + 1) is at most 32.

    One-dimensional channels, NumPy or torch device tensors.  Returns (surface, echoes): the cleaned surface as fast_xambg
    returns it, and one ECHO_RECORD_DTYPE record (lag, Doppler in Hz, complex amplitude) per removed atom, on the host, so
    that a caller can put the removed echoes back into its detections."""
    from .clutter_removal import cancel_echoes
    from .target_detection import refine_peaks
    if len(ref.shape) != 1:
        raise ValueError("clean_xambg takes one-dimensional channels")
    npeaks, lag_span, oversample = int(npeaks), int(lag_span), int(oversample)
    nd, nl = (int(v) for v in patch)
    if npeaks < 0 or lag_span < 0 or oversample < 1 or nd < 3 or nl < 3:
        raise ValueError("clean_xambg: npeaks and lag_span are >= 0, oversample >= 1 and a patch has at least 3 x 3 cells")
    if npeaks * (2 * lag_span + 1) > _lib.ECHO_MAX_ATOMS:
        raise ValueError(f"clean_xambg: npeaks (2 lag_span + 1) = {npeaks * (2 * lag_span + 1)} atoms, at most {_lib.ECHO_MAX_ATOMS}")
    n, R, F = int(ref.shape[0]), int(rangeBins), int(freqBins)
    X = fast_xambg(ref, srv, R, F)
    if npeaks == 0:
        return X, np.zeros(0, ECHO_RECORD_DTYPE)
    mag = X[:, :, 0].abs() if _lib.is_device_tensor(X) else np.abs(X[:, :, 0])
    rows, cols = _strongest_cells(mag, npeaks, int(doppler_guard), -(-nd // (2 * oversample)), nl // 2)
    step = float(sampleRate) / n / oversample
    lags0, dops0 = patch_origins(rows, cols, R, F, n, sampleRate, nl, nd, step)
    wrap = bool(cancel_kw.get("wrap", False))
    P = xambg_patch(ref, srv, sampleRate, lags0, dops0, nl, nd, step, wrap=wrap)
    pk = refine_peaks(P, lags0, dops0, step)
    if _lib.is_device_tensor(P):
        pk_lag, pk_dop = pk["lag"].cpu().numpy(), pk["doppler"].cpu().numpy()
    else:
        pk_lag, pk_dop = pk["lag"], pk["doppler"]
    centre = np.rint(pk_lag).astype(np.int64)
    lags = (centre[:, None] + np.arange(-lag_span, lag_span + 1)[None, :]).reshape(-1)
    dops = np.repeat(np.asarray(pk_dop, dtype=np.float64), 2 * lag_span + 1)
    cleaned, f, amp, _, _ = cancel_echoes(ref, srv, sampleRate, lags, dops, return_fit=True, **cancel_kw)
    rec = np.zeros(lags.shape[0], ECHO_RECORD_DTYPE)
    rec["lag"], rec["doppler"], rec["amplitude"] = lags, f, amp
    return fast_xambg(ref, cleaned, R, F), rec


def batch_xambg(refChannel, srvChannel, rangeBins, freqBins, batchLen, *, hop=None, start=0, filter="reciprocal", floor=0.1,
                window=None):
    """Range-Doppler map by the batches algorithm with a matched or a RECIPROCAL filter, for QAM-OFDM illuminators (DVB-T/T2,
    DAB, LTE, 5G): prc_batch_xambg of include/prcore.h, DESIGN.md section 28.  Batch j = 0 .. freqBins - 1 is the ``batchLen``
    (1024 or 4096) samples from ``start + j hop`` of both channels (``hop`` None: batchLen); each surveillance batch is
    correlated with its reference batch through their spectra -- ``filter="matched"`` multiplies by conj(R), as fast_xambg
    does; ``"reciprocal"`` divides by R, with |R|^2 held above ``floor``^2 times the batch's energy --, lags 0 .. rangeBins are
    kept, and a transform over the batches (freqBins: 256, 512, 1024, 2048 or 4096) gives the Doppler axis.  No wrap and no
    zero padding: the last batch must end inside the channels.

    The reciprocal filter turns every echo into one clean impulse per batch, so the data-dependent pedestal that a matched
    filter leaves on a noise-like illuminator (about 1 / sqrt(B T) of every strong echo's peak) is not there: with batches
    aligned to the useful parts of the symbols -- ``start = ofdm_symbol_start(ref, nfft, cp) + cp``, ``hop = nfft + cp``,
    ``batchLen = nfft`` -- an echo ``a ref(t - d)``, d <= cp, peaks at ``a freqBins (occupied carriers / batchLen)``.
    Two limits: on constant-modulus carriers (QPSK) the two filters coincide up to scale, and with batches that are not
    aligned to the symbols the reciprocal filter is no better than the matched one.  A Doppler shift also rotates the
    carriers inside a batch: echoes lose sinc(f_d batchLen / Fs) and leak between carriers, as in every batches algorithm.

    Channels are 1-D (returns (freqBins, rangeBins + 1, 1), so it drops in where fast_xambg stood) or [nframes, n] stacks
    (returns (nframes, freqBins, rangeBins + 1)), NumPy arrays or torch device tensors (zero copy, torch's current stream).
    Column k is delay rangeBins - k, rows are mirrored and fftshift-ed as fast_xambg's; scene.expected_peak_cell holds with
    the CPI taken as freqBins hop samples.  ``window``: a name or tuple for scipy's get_window over the freqBins batches, or an
    array of freqBins values (slow-time taper)."""
    if tuple(refChannel.shape) != tuple(srvChannel.shape):
        raise ValueError("Input vectors must have the same length")
    shape = residence.shape(refChannel)
    if len(shape) not in (1, 2):
        raise ValueError("batch_xambg takes one-dimensional channels or [nframes, n] stacks")
    if filter not in _lib.BATCH_FILTERS:
        raise ValueError(f"filter is 'reciprocal' or 'matched', not {filter!r}")
    n, nframes = int(shape[-1]), (1 if len(shape) == 1 else int(shape[0]))
    L, R, F = int(batchLen), int(rangeBins), int(freqBins)
    hop, start, floor = (L if hop is None else int(hop)), int(start), float(floor)
    if L not in _lib.BATCH_LENGTHS:
        raise NotImplementedError(f"batch_xambg: batchLen = {L}: batches of {' or '.join(map(str, _lib.BATCH_LENGTHS))} samples")
    if F not in _lib.BATCH_FREQ_BINS:
        raise NotImplementedError(f"batch_xambg: freqBins = {F}: one of {', '.join(map(str, _lib.BATCH_FREQ_BINS))}")
    if start < 0 or hop < 1:
        raise ValueError(f"batch_xambg: start = {start} and hop = {hop}: start >= 0 and hop >= 1")
    if not 0 <= R < L:
        raise ValueError(f"batch_xambg: rangeBins = {R}: not in 0 .. batchLen - 1 = {L - 1}")
    if start + (F - 1) * hop + L > n:
        raise ValueError(f"batch_xambg: the last batch ends at start + (freqBins - 1) hop + batchLen = {start + (F - 1) * hop + L}, "
                         f"beyond the {n} samples of a channel")
    if not (floor >= 0.0 and np.isfinite(floor)):
        raise ValueError(f"batch_xambg: floor = {floor}: a finite number >= 0")
    if isinstance(window, (tuple, str)):
        window = _named_window(window, F)
    if window is not None and tuple(residence.shape(window)) != (F,):
        raise ValueError(f"operands could not be broadcast together with shapes ({F},) {tuple(residence.shape(window))}")
    side = residence.of(refChannel, srvChannel, mixed="the channels are both NumPy arrays or both device tensors")
    if window is not None and _lib.is_device_tensor(window) and not side.torch:
        raise ValueError("a device-tensor window goes with device-tensor channels")
    desc = engine.batch_xambg_desc(n, L, R, F, hop, start, _lib.BATCH_FILTERS[filter], floor)
    nws = engine.batch_xambg_workspace_bytes(desc, nframes)      # the library's own checks, still on the host
    oshape = (F, R + 1, 1) if len(shape) == 1 else (nframes, F, R + 1)
    if nframes == 0:
        return side.nothing(oshape, np.complex64)
    with side.device():
        ref = side.put("bx_ref", refChannel, np.complex64)
        srv = side.put("bx_srv", srvChannel, np.complex64)
        win = None if window is None else side.put("bx_win", window, np.float32)
        out = side.empty("bx_out", oshape, np.complex64)
        ws = side.scratch("bx_ws", nws)
        engine.batch_xambg_execute(desc, ref, srv, n, win, out, nframes, ws, side.stream)
    return side.result(out, oshape, np.complex64)


def ofdm_symbol_start(ref, nfft, cp, nsym=None, return_metric=False):
    """Where the OFDM symbols of ``ref`` start, modulo nfft + cp, from the cyclic prefix (prc_ofdm_timing): for every offset
    o = 0 .. nfft + cp - 1 the correlation of the ``cp`` samples from ``o + s (nfft + cp)`` with the samples ``nfft`` later is
    summed over ``nsym`` symbols (float64 sums of the float32 products) and the offset of the largest magnitude is returned,
    the lowest on ties.  The batches of ``batch_xambg`` are aligned with ``start = ofdm_symbol_start(...) + cp``,
    ``hop = nfft + cp``, ``batchLen = nfft``.  ``nsym`` None: as many symbols as the length allows, 4096 at most.
    ``ref`` is a 1-D NumPy array or torch device tensor; returns a Python int -- one small device-to-host copy -- and, with
    ``return_metric``, the float64 metric [nfft + cp] beside it (an array, or a tensor on the caller's device)."""
    shape = residence.shape(ref)
    if len(shape) != 1:
        raise ValueError("ofdm_symbol_start takes a one-dimensional channel")
    n, nfft, cp = int(shape[0]), int(nfft), int(cp)
    if nfft < 2 or not 1 <= cp < nfft:
        raise ValueError(f"ofdm_symbol_start: nfft = {nfft}, cp = {cp}: nfft >= 2 and 1 <= cp < nfft")
    sym = nfft + cp
    most = (n - nfft) // sym - 1
    nsym = min(most, 4096) if nsym is None else int(nsym)
    if nsym < 1 or nsym > most:
        raise ValueError(f"ofdm_symbol_start: (nsym + 1) (nfft + cp) + nfft = {(max(nsym, 1) + 1) * sym + nfft} samples are needed, "
                         f"the channel has {n}")
    side = residence.of(ref)
    with side.device():
        x = side.put("ot_ref", ref, np.complex64)
        metric = side.empty("ot_metric", (sym,), np.float64)
        where = side.empty("ot_start", (1,), np.int32)
        engine.ofdm_timing(x, n, nfft, cp, nsym, metric, where, side.stream)
        at = int(side.fetch(where, (1,), np.int32)[0])
    return (at, side.result(metric, (sym,), np.float64)) if return_metric else at
