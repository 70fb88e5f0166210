"""Drop-ins for ``passiveRadar/signal_utils.py``: every function of the module, on the device."""
from __future__ import annotations

import collections
import ctypes as C
import operator
import threading

import numpy as np

from . import _lib, engine, residence
from ._lib import check, lib

__all__ = ["xcorr", "frequency_shift", "deinterleave_IQ", "resample", "front_end", "find_channel_offset",
           "decimate_iir", "decimate", "channel_preprocessing", "channelize", "shift", "offset_compensation", "normalize"]


def _xcorr_equal_lengths(s1, s2, nlead, nlag):
    """xcorr of two signals of different lengths as the equal-length sum on zero-extended copies (host logic, no device
    call): returns (e1, e2, nlead', nlag') with xcorr(s1, s2, nlead, nlag) == xcorr(e1, e2, nlead', nlag')"""
    n1, n2 = s1.shape[0], s2.shape[0]
    m = n2 + nlag + nlead
    K = abs(m - n1)
    if m >= n1:
        # offsets K - nlag - i of s2 against s1: lead' = K - nlag (when negative, s2 is delayed by that much first)
        lead = K - nlag
        front = max(-lead, 0)
        e2 = np.zeros(max(n1, n2 + front), np.complex64)
        e2[front:front + n2] = s2
        e1 = np.zeros(e2.shape[0], np.complex64)
        e1[:n1] = s1
        return e1, e2, lead + front, K - (lead + front)
    e2 = np.zeros(n1, np.complex64)                         # the padded s2, zero-extended to len(s1)
    e2[nlag:nlag + n2] = s2
    return s1, e2, 0, K


def xcorr(s1, s2, nlead, nlag):
    """signal_utils.py:29-32: ``correlate(s1, pad(s2, (nlag, nlead)), mode='valid')``, complex64.

    Equal lengths (every call site of the reference): z[i] = sum_n s1[n] conj(s2[n-(i-nlead)]), i = 0..nlag+nlead.
    The reference's expression accepts ANY two lengths; with m = len(s2) + nlag + nlead and K = |m - len(s1)| SciPy's
    'valid' mode returns K + 1 values:
      m >= len(s1):  z[i] = sum_l s1[l]   conj(s2[l + K - i - nlag]),  i = 0..K   (the padded s2 slides over s1)
      m <  len(s1):  z[k] = sum_l s1[l+k] conj(s2[l - nlag]),          k = 0..K   (s1 slides over the padded s2)
    Both are the equal-length sum on zero-extended copies (zeros add nothing), which is how they reach prc_xcorr."""
    s1 = np.ascontiguousarray(s1, dtype=np.complex64)
    s2 = np.ascontiguousarray(s2, dtype=np.complex64)
    if s1.ndim != 1 or s2.ndim != 1:
        raise ValueError("xcorr takes one-dimensional signals")
    nlead, nlag = int(nlead), int(nlag)
    if nlead < 0 or nlag < 0:
        raise ValueError("index can't contain negative values")          # np.pad's complaint about (nlag, nlead)
    if s1.shape[0] != s2.shape[0]:
        s1, s2, nlead, nlag = _xcorr_equal_lengths(s1, s2, nlead, nlag)
    n1 = s1.shape[0]
    n = n1
    st = engine.staging()
    d1 = st.get("xc_1", 8 * n)
    d2 = st.get("xc_2", 8 * n)
    do = st.get("xc_o", 8 * (nlag + nlead + 1))
    d1.upload(s1)
    d2.upload(s2)
    check(lib().prc_xcorr(d1.ptr, d2.ptr, n, nlead, nlag, do.ptr, None))
    return do.download((nlag + nlead + 1,), np.complex64)


def frequency_shift(x, fc, Fs, phase_offset=0):
    """signal_utils.py:24-27 with the reference's float32 phase ramp.  phase_offset: a scalar (complex64 result), or an
    array NumPy broadcasts against x -- one value (main.py:133-149: the starting phase of a dask block) or one per
    sample; a float64 / integer array promotes the result to complex128 (float32 ramp + double phase, exponential in
    double), a float32 array keeps it complex64, as in the reference."""
    if np.ndim(phase_offset) != 0:
        ph = np.asarray(phase_offset)
        x = np.ascontiguousarray(x, dtype=np.complex64)
        n = x.shape[0]
        if ph.ndim != 1 or ph.shape[0] not in (1, n) or x.ndim != 1:
            raise ValueError(f"operands could not be broadcast together with shapes ({n},) {ph.shape}")
        f32 = ph.dtype in (np.float32, np.float16)
        st = engine.staging()
        dx = st.get("fs_x", 8 * n)
        dx.upload(x)
        if ph.shape[0] == 1 and not f32:
            dy = st.get("fs_y128", 16 * n)
            check(lib().prc_frequency_shift_block(dx.ptr, dy.ptr, n, float(fc), float(Fs), float(ph[0]), None))
            return dy.download((n,), np.complex128)
        ph = np.ascontiguousarray(np.broadcast_to(ph, (n,)), dtype=np.float32 if f32 else np.float64)
        dp = st.get("fs_ph", ph.nbytes)
        dp.upload(ph)
        dy = st.get("fs_y128", (8 if f32 else 16) * n)
        check(lib().prc_frequency_shift_phases(dx.ptr, dy.ptr, n, float(fc), float(Fs), dp.ptr, int(f32), None))
        return dy.download((n,), np.complex64 if f32 else np.complex128)
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n = x.shape[0]
    st = engine.staging()
    dx = st.get("fs_x", 8 * n)
    dy = st.get("fs_y", 8 * n)
    dx.upload(x)
    check(lib().prc_frequency_shift(dx.ptr, dy.ptr, n, float(fc), float(Fs), float(phase_offset), None))
    return dy.download((n,), np.complex64)


def deinterleave_IQ(interleavedIQ):
    """signal_utils.py:19-22: interleaved I,Q scalars (int8 / uint8 / int16 / float32) -> complex64."""
    raw = np.ascontiguousarray(interleavedIQ)
    if str(raw.dtype) not in ("int8", "uint8", "int16", "float32"):
        raw = raw.astype(np.float32)
    n = raw.shape[0] // 2
    st = engine.staging()
    dr = st.get("di_raw", raw.nbytes)
    do = st.get("di_out", 8 * max(n, 1))
    dr.upload(raw)
    check(lib().prc_deinterleave(dr.ptr, _lib.RAW_DTYPES[str(raw.dtype)], n, do.ptr, None))
    return do.download((n,), np.complex64)


def decimate_iir(x, q):
    """scipy.signal.decimate(x, q) with its defaults, as find_channel_offset uses it (signal_utils.py:75-76):
    zero-phase order-8 Chebyshev-I low-pass, every q-th sample, complex64."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n = x.shape[0]
    dec = engine.cached_plan(("iirdec", int(q)), lambda: engine.IirDecimator(q))
    st = engine.staging()
    dx = st.get("dec_x", 8 * max(n, 1))
    dy = st.get("dec_y", 8 * max(dec.out_len(n), 1))
    dx.upload(x)
    dec.decimate(dx, n, dy)
    return dy.download((dec.out_len(n),), np.complex64)


def find_channel_offset(s1, s2, nd, nl, return_xc=False):
    """signal_utils.py:73-78: (argmax|correlate(decimate(s1, nd), pad(decimate(s2, nd), nl), 'valid')| - nl)*nd.
    With ``return_xc`` also the correlation magnitudes (float32, m2 + 2 nl - m1 + 1 lags)."""
    s1 = np.ascontiguousarray(s1, dtype=np.complex64)
    s2 = np.ascontiguousarray(s2, dtype=np.complex64)
    if s1.ndim != 1 or s2.ndim != 1:
        raise ValueError("find_channel_offset takes one-dimensional signals")
    nl = int(nl)
    dec = engine.cached_plan(("iirdec", int(nd)), lambda: engine.IirDecimator(nd))
    n1, n2 = s1.shape[0], s2.shape[0]
    st = engine.staging()
    d1 = st.get("co_1", 8 * max(n1, 1))
    d2 = st.get("co_2", 8 * max(n2, 1))
    d1.upload(s1)
    d2.upload(s2)
    dxc = None
    if return_xc:
        dxc = st.get("co_xc", 4 * max(dec.n_lags(n1, n2, nl), 1))
    am, n_xc = dec.channel_offset(d1, n1, d2, n2, nl, dxc)
    offset = (am - nl) * int(nd)
    if return_xc:
        return offset, dxc.download((n_xc,), np.float32)
    return offset


def resample(x, up, dn):
    """signal_utils.py:15-17: rational resampling, scipy.signal.resample_poly(x, up, dn, padtype='line').
    The stream is complex64 on the device; the result is returned in the input's dtype (the reference
    keeps complex128 when fed the tuned complex128 stream)."""
    xin = np.asarray(x)
    from math import gcd
    g = gcd(int(up), int(dn))
    if int(up) // g == 1 and int(dn) // g == 1:
        return xin.copy()                                  # scipy.signal.resample_poly: up == down -> a copy
    xc = np.ascontiguousarray(xin, dtype=np.complex64)
    n = xc.shape[0]
    plan = engine.cached_plan(("fe", n, "complex64", int(up), int(dn)),
                              lambda: engine.FrontendPlan(n, "complex64", up, dn, 1))
    st = engine.staging()
    dx = st.get("rs_x", 8 * n)
    do = st.get("rs_o", 8 * plan.n_out)
    dx.upload(xc)
    plan.execute(dx, do, 1, n, plan.n_out, mix=False)
    y = do.download((plan.n_out,), np.complex64)
    return y.astype(xin.dtype) if np.iscomplexobj(xin) else y.real.astype(xin.dtype)


def front_end(raw, input_chunk_length, offset_freq, input_sample_rate, up, dn, max_blocks=16):
    """main.py:105-166 for one channel: per block of ``input_chunk_length`` raw scalars
    deinterleave -> tune by ``offset_freq`` with the block starting phase (main.py:125-130) ->
    resample(up, dn), ONE fused kernel per batch of blocks.  Returns the concatenated complex64 IF stream."""
    raw = np.ascontiguousarray(raw)
    if str(raw.dtype) not in ("int8", "uint8", "int16", "float32"):
        raw = raw.astype(np.float32)
    icl = int(input_chunk_length)
    nblocks = raw.shape[0] // icl
    n_in = icl // 2
    mod_period = input_sample_rate // offset_freq
    per_block = n_in % mod_period
    phases = 2 * np.pi * np.arange(nblocks) * per_block * (offset_freq / input_sample_rate)
    plan = engine.cached_plan(("fe", n_in, str(raw.dtype), int(up), int(dn), max_blocks),
                              lambda: engine.FrontendPlan(n_in, str(raw.dtype), up, dn, max_blocks))
    st = engine.staging()
    dr = st.get("fe_raw", raw.nbytes)
    do = st.get("fe_out", 8 * plan.n_out * max(nblocks, 1))
    dr.upload(raw)
    isz = raw.dtype.itemsize
    for b0 in range(0, nblocks, max_blocks):
        nb = min(max_blocks, nblocks - b0)
        plan.execute(dr.ptr + b0 * icl * isz, do.ptr + 8 * b0 * plan.n_out, nb, icl, plan.n_out,
                     offset_freq, input_sample_rate, phases[b0:b0 + nb], True)
    return do.download((nblocks * plan.n_out,), np.complex64)


# ---- decimate, channel_preprocessing, shift, offset_compensation, normalize (signal_utils.py:7-13, 34-71, 80-85) -------
_RAW_NUMPY = ("int8", "uint8", "int16", "float32")
_TAP_CACHE_ENTRIES = 16
_taps = collections.OrderedDict()        # (device, q) -> DeviceBuffer of the float32 taps
_taps_lock = threading.Lock()
_MAX_CHANNELS = 65535                    # channels per prc_fir_decimate launch


def _decimate_taps(q):
    """scipy.signal.decimate's FIR for ftype='fir', n = 20 q: firwin(20 q + 1, 1 / q, window='hamming'), as float32.
    q == 1 raises firwin's ValueError (a cut-off at Nyquist), as in the reference."""
    from scipy.signal import firwin
    if q < 1:
        raise ValueError("q must be a positive integer")
    return firwin(20 * q + 1, 1.0 / q, window="hamming").astype(np.float32)


def _device_taps(q, device):
    """decimate's float32 taps on the device, from a small cache keyed by q"""
    return _device_table((device, q), lambda: _decimate_taps(q))


def _device_table(key, make):
    """a small constant table (``make()``: a NumPy array) on the device, from the cache of the decimation taps"""
    with _taps_lock:
        buf = _taps.get(key)
        if buf is None:
            h = make()
            buf = _lib.DeviceBuffer(h.nbytes)
            buf.upload(h)
            _taps[key] = buf
            while len(_taps) > _TAP_CACHE_ENTRIES:
                _taps.popitem(last=False)
        else:
            _taps.move_to_end(key)
        return buf


def _result_dtype(dtype):
    """what NumPy / SciPy return for an input of this dtype: complex64, complex128, float32 and float64 stay, the rest
    (integers, bool, float16) is float64"""
    dtype = np.dtype(dtype)
    if dtype in (np.complex64, np.complex128, np.float32, np.float64):
        return dtype
    if dtype.kind == "c":
        return np.dtype(np.complex128)
    return np.dtype(np.float64)


def _fir_decimate(q, code, mix, fc, Fs, x_ptr, x_scalar_bytes, n, k, out_ptr, taps_ptr, stream):
    """prc_fir_decimate on an (n, k) C-order input and a (ceil(n / q), k) complex64 output, 65535 channels per launch"""
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix = q, 20 * q + 1, code, int(mix)
    d.fc, d.fs, d.phase_offset = float(fc), float(Fs), 0.0
    for c0 in range(0, k, _MAX_CHANNELS):
        nch = min(_MAX_CHANNELS, k - c0)
        check(lib().prc_fir_decimate(C.byref(d), taps_ptr, x_ptr + c0 * x_scalar_bytes, n, k, 1, nch, out_ptr + 8 * c0, k, 1,
                                     stream))


def _torch_raw_code(x, what):
    import torch
    names = {torch.int8: "int8", torch.uint8: "uint8", torch.int16: "int16", torch.float32: "float32"}
    if x.dtype not in names:
        raise ValueError(f"{what}: a device tensor holds int8, uint8, int16 or float32 interleaved I,Q scalars")
    return _lib.RAW_DTYPES[names[x.dtype]]


def decimate(x, q):
    """signal_utils.py:11-13: ``scipy.signal.decimate(x, q, 20*q, ftype='fir', axis=0)`` -- the zero-phase Hamming FIR of
    20 q + 1 taps with zero padding, every q-th sample, along axis 0 (every trailing index is a channel of its own).
    The device computes in complex64 with float32 taps; the result comes back in the reference's dtype (complex64,
    complex128, float32 and float64 stay, integers give float64), so a complex128 or float64 result carries float32
    accuracy.  A complex64 torch device tensor is read in place on torch's current stream and gives a device tensor."""
    q = operator.index(q)                                   # TypeError for a float, as scipy.signal.decimate
    h_check = _decimate_taps(q)                             # ValueError for q == 1, before any device call
    del h_check
    if _lib.is_device_tensor(x):
        import torch
        if x.dtype != torch.complex64:
            raise ValueError("decimate: a device tensor is complex64")
        if x.dim() < 1:
            raise ValueError("decimate: x has no axis 0")
        n, trail = int(x.shape[0]), tuple(x.shape[1:])
        k = int(np.prod(trail, dtype=np.int64))
        out = torch.empty((-(-n // q),) + trail, dtype=torch.complex64, device=x.device)
        if n == 0 or k == 0:
            return out
        with torch.cuda.device(x.device):
            xc = x.contiguous()
            taps = _device_taps(q, x.device.index)
            _fir_decimate(q, _lib.RAW_DTYPES["complex64"], 0, 0.0, 1.0, xc.data_ptr(), 8, n, k, out.data_ptr(), taps.ptr,
                          _lib.torch_stream_ptr(x.device))
        return out
    xin = np.asarray(x)
    if xin.ndim < 1:
        raise ValueError("decimate: x has no axis 0")
    odt = _result_dtype(xin.dtype)
    n, trail = xin.shape[0], xin.shape[1:]
    k = int(np.prod(trail, dtype=np.int64))
    n_out = -(-n // q)
    if n == 0 or k == 0:
        return np.zeros((n_out,) + trail, odt)
    xc = np.ascontiguousarray(xin, dtype=np.complex64)
    _lib.require_gpu()
    taps = _device_taps(q, _lib.current_device())
    st = engine.staging()
    dx = st.get("fd_x", xc.nbytes)
    do = st.get("fd_o", 8 * n_out * k)
    dx.upload(xc)
    _fir_decimate(q, _lib.RAW_DTYPES["complex64"], 0, 0.0, 1.0, dx.ptr, 8, n, k, do.ptr, taps.ptr, None)
    y = do.download((n_out,) + trail, np.complex64)
    return y.astype(odt) if odt.kind == "c" else y.real.astype(odt)


def channel_preprocessing(sig, dec, fc, Fs):
    """signal_utils.py:80-85: ``decimate(frequency_shift(deinterleave_IQ(sig), fc, Fs), dec)``, complex64 of length
    ceil((len(sig) // 2) / dec), in ONE launch: the raw int8 / uint8 / int16 / float32 scalars are converted and rotated
    (the reference's float32 phase ramp) while a tile is staged, and the tuned stream never reaches memory.  Other dtypes are
    taken as float32.  A raw torch device tensor is read in place on torch's current stream and gives a device tensor."""
    dec = operator.index(dec)
    h_check = _decimate_taps(dec)
    del h_check
    if float(Fs) == 0.0:
        raise ZeroDivisionError("channel_preprocessing: Fs is zero")
    if _lib.is_device_tensor(sig):
        import torch
        code = _torch_raw_code(sig, "channel_preprocessing")
        if sig.dim() != 1:
            raise ValueError("channel_preprocessing takes a one-dimensional array of interleaved I,Q scalars")
        n = int(sig.shape[0]) // 2
        out = torch.empty((-(-n // dec),), dtype=torch.complex64, device=sig.device)
        if n == 0:
            return out
        with torch.cuda.device(sig.device):
            raw = sig.contiguous()
            taps = _device_taps(dec, sig.device.index)
            _fir_decimate(dec, code, 1, fc, Fs, raw.data_ptr(), raw.element_size(), n, 1, out.data_ptr(), taps.ptr,
                          _lib.torch_stream_ptr(sig.device))
        return out
    raw = np.ascontiguousarray(sig)
    if raw.ndim != 1:
        raise ValueError("channel_preprocessing takes a one-dimensional array of interleaved I,Q scalars")
    if str(raw.dtype) not in _RAW_NUMPY:
        raw = raw.astype(np.float32)
    n = raw.shape[0] // 2
    n_out = -(-n // dec)
    if n == 0:
        return np.zeros((0,), np.complex64)
    _lib.require_gpu()
    taps = _device_taps(dec, _lib.current_device())
    st = engine.staging()
    dr = st.get("cp_raw", raw.nbytes)
    do = st.get("cp_out", 8 * n_out)
    dr.upload(raw)
    _fir_decimate(dec, _lib.RAW_DTYPES[str(raw.dtype)], 1, fc, Fs, dr.ptr, raw.dtype.itemsize, n, 1, do.ptr, taps.ptr, None)
    return do.download((n_out,), np.complex64)


def _twiddles(nchan):
    """(cos, sin)(2 pi r / M), r < M: float64 on the host, rounded to float32 -- the only rotation channelize applies"""
    ang = 2.0 * np.pi * np.arange(nchan, dtype=np.float64) / nchan
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


def _channelize_input(sig):
    """(raw dtype name, samples) of channelize's input: interleaved I,Q scalars as channel_preprocessing takes them (other
    real dtypes are taken as float32, a trailing odd scalar is ignored) or a complex stream, taken as complex64"""
    if sig.ndim != 1:
        raise ValueError("channelize takes a one-dimensional array of interleaved I,Q scalars or a complex64 stream")
    name = residence.dtype_name(sig)
    if residence.iscomplex(sig):
        if _lib.is_device_tensor(sig) and name != "complex64":
            raise ValueError("channelize: a complex device tensor is complex64")
        return "complex64", int(sig.shape[0])
    if name not in _RAW_NUMPY:
        if _lib.is_device_tensor(sig):
            raise ValueError("channelize: a device tensor holds int8, uint8, int16 or float32 interleaved I,Q scalars, or complex64")
        name = "float32"
    return name, int(sig.shape[0]) // 2


def channelize(sig, nchan, dec, channels=None, *, taps=None, start=0):
    """Uniform polyphase filter bank: the channels ``channels`` (default: all, 0 .. nchan - 1) of ``nchan`` centred at
    k Fs / nchan, low-passed by ``taps`` and decimated by ``dec``, out of ONE pass over the raw recording; complex64 of shape
    (K, ceil(n / dec)).  With c = (L - 1) / 2 and x[start + .] the stream,

        y[i][j] = sum_t taps[t] x[j dec + c - t] exp(-2 pi i ((k_i (start + j dec + c - t)) mod nchan) / nchan)

    -- with the default taps (decimate's firwin(20 dec + 1, 1 / dec), float32) row i is
    ``channel_preprocessing(sig, dec, -k_i Fs / nchan, Fs)`` with an exact phase: the exponent is an integer reduced modulo
    nchan and the rotation a table of nchan float32 twiddles, so ``start`` = 2^40 is as accurate as 0 and a later block of a
    stream, passed with its own ``start``, continues the earlier one.  dec need not equal, divide or be divided by nchan.
    ``sig``: interleaved I,Q scalars typed as channel_preprocessing takes them, or a complex64 stream; NumPy, or a torch
    device tensor, which is read in place on torch's current stream and gives a device tensor.  A channel is an integer in
    [-nchan / 2, nchan): k and k - nchan are the same; duplicates are allowed and the bits of a row do not depend on the
    other rows asked for.  ``taps``: real, odd length."""
    M, D, start = operator.index(nchan), operator.index(dec), operator.index(start)
    if not 2 <= M <= _lib.CHANNELIZE_MAX_CHAN:
        raise ValueError(f"channelize: nchan = {M} outside 2 .. {_lib.CHANNELIZE_MAX_CHAN}")
    if taps is None:
        if D < 2:
            raise ValueError("channelize: dec must be 2 or more with the default taps (pass taps for dec = 1)")
        h, L = None, 20 * D + 1
    else:
        h = np.ascontiguousarray(taps, dtype=np.float32)
        if h.ndim != 1 or h.shape[0] % 2 == 0:
            raise ValueError("channelize: taps are one-dimensional, of odd length")
        if D < 1:
            raise ValueError("channelize: dec must be a positive integer")
        L = h.shape[0]
    if not -2 ** 63 <= start < 2 ** 63:
        raise ValueError("channelize: start is an int64 stream index")
    if channels is None:
        ch = np.arange(M, dtype=np.int32)
    else:
        ch = np.asarray(channels)
        if ch.ndim != 1 or (ch.size and ch.dtype.kind not in "iu"):
            raise ValueError("channelize: channels is a one-dimensional list of integers")
        if ch.size and (np.any(2 * ch.astype(np.int64) < -M) or np.any(ch.astype(np.int64) >= M)):
            raise ValueError(f"channelize: a channel outside [-{M}/2, {M})")
        ch = ch.astype(np.int32)
    side = residence.of(sig)
    if not side.torch:
        sig = np.asarray(sig)
    name, n = _channelize_input(sig)
    K, n_out = int(ch.shape[0]), -(-n // D)
    if n == 0 or K == 0:
        return side.nothing((K, n_out), np.complex64)
    with side.device():
        x = side.put("cz_x", sig, name)
        dev = sig.device.index if side.torch else _lib.current_device()
        dtaps = _device_taps(D, dev) if h is None else side.put("cz_taps", h, np.float32)
        dtw = _device_table((dev, "twiddles", M), lambda: _twiddles(M))
        dch = side.put("cz_ch", ch, np.int32)
        out = side.empty("cz_out", (K, n_out), np.complex64)
        d = _lib.ChannelizeDesc()
        d.nchan, d.dec, d.ntaps, d.raw_dtype, d.start = M, D, L, _lib.RAW_DTYPES[name], start
        for k0 in range(0, K, _lib.CHANNELIZE_MAX_SEL):              # 64 rows per launch
            d.nsel = min(_lib.CHANNELIZE_MAX_SEL, K - k0)
            check(lib().prc_channelize(C.byref(d), dtaps.ptr, dtw.ptr, dch.ptr + 4 * k0, x.ptr, n, out.ptr + 8 * k0 * n_out, n_out,
                                       side.stream))
    return side.result(out, (K, n_out), np.complex64)


def shift(x, n):
    """signal_utils.py:34-47: x delayed by n samples along axis 0 (n < 0: advanced), zeros where nothing arrives; dtype
    and shape are kept, ``n == 0`` returns x itself.  A torch device tensor gives a device tensor."""
    if n == 0:
        return x
    n = operator.index(n)
    if _lib.is_device_tensor(x):
        import torch
        if x.dim() < 1:
            raise ValueError("shift: x has no axis 0")
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        rows = int(x.shape[0])
        row_bytes = (x.numel() // rows) * x.element_size() if rows else 0
        if rows == 0 or row_bytes == 0:
            return out
        with torch.cuda.device(x.device):
            xc = x.contiguous()
            check(lib().prc_shift(xc.data_ptr(), out.data_ptr(), rows, row_bytes, n, _lib.torch_stream_ptr(x.device)))
        return out
    xin = np.ascontiguousarray(x)
    if xin.ndim < 1:
        raise ValueError("shift: x has no axis 0")
    if xin.dtype.hasobject:
        raise ValueError("shift: object arrays have no device form")
    rows = xin.shape[0]
    row_bytes = (xin.size // rows) * xin.dtype.itemsize if rows else 0
    if rows == 0 or row_bytes == 0:
        return np.zeros_like(xin)
    _lib.require_gpu()
    st = engine.staging()
    dx = st.get("sh_x", xin.nbytes)
    dy = st.get("sh_y", xin.nbytes)
    dx.upload(xin)
    check(lib().prc_shift(dx.ptr, dy.ptr, rows, row_bytes, n, None))
    return dy.download(xin.shape, xin.dtype)


def offset_compensation(x1, x2, ns, ndec, nlag=2000):
    """signal_utils.py:49-71: the offset of x2 against x1 from find_channel_offset on their first ``int(ns)`` samples,
    then x2 shifted so that it lines up with x1 (zeros at the edge); x2 itself when the offset is 0.  Device tensors stay
    on their device; finding the offset synchronises, as find_channel_offset does."""
    ns = int(ns)
    if _lib.is_device_tensor(x1) and _lib.is_device_tensor(x2):
        import torch
        with torch.cuda.device(x2.device):
            s1 = x1[0:ns].to(device=x2.device, dtype=torch.complex64).contiguous()
            s2 = x2[0:ns].to(torch.complex64).contiguous()
            if s1.dim() != 1 or s2.dim() != 1:
                raise ValueError("find_channel_offset takes one-dimensional signals")
            dec = engine.cached_plan(("iirdec", int(ndec)), lambda: engine.IirDecimator(ndec))
            am, _ = dec.channel_offset(s1, s1.shape[0], s2, s2.shape[0], int(nlag), None,
                                       stream=_lib.torch_stream_ptr(x2.device))
        os_ = (am - int(nlag)) * int(ndec)
    else:
        os_ = find_channel_offset(x1[0:ns], x2[0:ns], ndec, nlag)
    if os_ == 0:
        return x2
    return shift(x2, os_)


def normalize(x):
    """signal_utils.py:7-9: ``x / mean(|x|)`` over all elements, any shape.  |x| is summed in float64 on the device and the
    division is float32 (complex64); the result comes back in the reference's dtype (complex64, complex128, float32 and
    float64 stay, integers give float64).  A float32 or complex64 torch device tensor gives a device tensor."""
    if _lib.is_device_tensor(x):
        import torch
        if x.dtype not in (torch.float32, torch.complex64):
            raise ValueError("normalize: a device tensor is float32 or complex64")
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        n = x.numel()
        if n == 0:
            return out
        with torch.cuda.device(x.device):
            xc = x.contiguous()
            ws = C.c_size_t(0)
            check(lib().prc_normalize_workspace_bytes(n, C.byref(ws)))
            work = torch.empty((int(ws.value) // 8,), dtype=torch.float64, device=x.device)
            check(lib().prc_normalize(xc.data_ptr(), out.data_ptr(), n, int(x.dtype == torch.complex64), work.data_ptr(),
                                      _lib.torch_stream_ptr(x.device)))
        return out
    xin = np.asarray(x)
    odt = _result_dtype(xin.dtype)
    n = xin.size
    if n == 0:
        return np.zeros(xin.shape, odt)
    cplx = odt.kind == "c"
    xc = np.ascontiguousarray(xin, dtype=np.complex64 if cplx else np.float32)
    _lib.require_gpu()
    ws = C.c_size_t(0)
    check(lib().prc_normalize_workspace_bytes(n, C.byref(ws)))
    st = engine.staging()
    dx = st.get("nz_x", xc.nbytes)
    dw = st.get("nz_w", int(ws.value))
    dx.upload(xc)
    check(lib().prc_normalize(dx.ptr, dx.ptr, n, int(cplx), dw.ptr, None))
    return dx.download(xin.shape, xc.dtype).astype(odt)
