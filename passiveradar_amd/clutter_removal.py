"""Drop-in for the clutter filters of the reference's ``passiveRadar/clutter_removal.py`` that
are on the north-star path: LS_Filter (:6-56), LS_Filter_Toeplitz (:109-160),
LS_Filter_Multiple (:162-187), NLMS_filter (:189-249), and GAL_JPE (:251-365), and for LS_Filter_SVD
(:58-107), which the reference never calls itself.  Same signatures, return dtypes and ValueError on
mismatched inputs; the arithmetic runs in libprcore.so (complex64 streams, complex128 Levinson solve
on device).  LS_Filter_SVD is the truncated-SVD form through the float64 Gram matrix of the circulant
data matrix (csrc/ls_svd.hip); it adds a relative cut ``rcond`` to the reference's absolute one.
ECA_Filter is not in the reference: LS_Filter_Multiple's bins solved jointly instead of one after another (csrc/eca.hip).
Nor is cancel_echoes: the joint least-squares removal of strong echoes at any (lag, Doppler) (csrc/echo.hip).
"""
from __future__ import annotations

import numpy as np

from . import _lib, engine, residence

__all__ = ["LS_Filter", "LS_Filter_SVD", "LS_Filter_Toeplitz", "LS_Filter_Multiple", "ECA_Filter", "NLMS_filter", "GAL_JPE",
           "cancel_echoes", "set_default_ls_method"]

_LS_METHOD = {"m": 0}     # 0 auto | 1 time-domain kernels | 2 FFT kernels (tests flip it)


def set_default_ls_method(method):
    _LS_METHOD["m"] = int(method)


def _check_same(ref, srv):
    if tuple(ref.shape) != tuple(srv.shape):
        raise ValueError("Input vectors must have the same length")


def _ls_run(ref, srv, filterLen, peek, circular, sampleRate, bins, reg, want_taps):
    ref = np.ascontiguousarray(ref, dtype=np.complex64)
    srv = np.ascontiguousarray(srv, dtype=np.complex64)
    n = ref.shape[0]
    T = int(filterLen) + int(peek)
    meth = _LS_METHOD["m"]
    plan = engine.cached_plan(("ls", n, int(filterLen), int(peek), bool(circular), meth),
                              lambda: engine.LsPlan(n, filterLen, peek, circular, 1, meth))
    st = engine.staging()
    d_ref = st.get("ls_ref", 8 * n)
    d_srv = st.get("ls_srv", 8 * n)
    d_out = st.get("ls_out", 8 * n)
    d_taps = st.get("ls_taps", 16 * T)
    d_ref.upload(ref)
    d_srv.upload(srv)
    plan.execute(d_ref, d_srv, d_out, 1, n, n, sampleRate, bins, reg, d_taps)
    out = d_out.download((n,), np.complex64)
    taps = d_taps.download((T,), np.complex128) if want_taps else None
    return out, taps


def LS_Filter_Toeplitz(refChannel, srvChannel, filterLen, peek=10, return_filter=False):
    """Block LS canceller, Toeplitz/Levinson form (:109-160).  Returns complex128 like the reference
    (values are the device's complex64 stream; taps are complex128 from the fp64 solve)."""
    _check_same(refChannel, srvChannel)
    out, taps = _ls_run(refChannel, srvChannel, filterLen, peek, False, 1.0, (0.0,), 0.0, return_filter)
    out = out.astype(np.complex128)
    return (out, taps) if return_filter else out


def LS_Filter_Multiple(refChannel, srvChannel, filterLen, sampleRate, dopplerBins=[0]):
    """LS_Filter_Toeplitz chained over Doppler bins (:162-187); the whole chain stays on the GPU."""
    _check_same(refChannel, srvChannel)
    bins = [float(b) for b in dopplerBins]
    if not bins:
        return srvChannel
    out, _ = _ls_run(refChannel, srvChannel, filterLen, 10, False, float(sampleRate), bins, 0.0, False)
    return out.astype(np.complex128)


def LS_Filter(refChannel, srvChannel, filterLen, reg=1.0, peek=10, return_filter=False):
    """Direct-matrix block LS (:6-56) without forming the N x T matrix: its Gram matrix is the
    circular-autocorrelation Toeplitz matrix, so this is the Toeplitz path with circular indexing
    and ``reg`` on the diagonal.  complex64 out and taps, like the reference."""
    _check_same(refChannel, srvChannel)
    out, taps = _ls_run(refChannel, srvChannel, filterLen, peek, True, 1.0, (0.0,), float(reg),
                        return_filter)
    return (out, taps.astype(np.complex64)) if return_filter else out


def LS_Filter_SVD(refChannel, srvChannel, filterLen, peek=10, return_filter=False, *, rcond=None,
                  return_singular_values=False):
    """Block LS canceller by truncated SVD (:58-107) without forming the N x T matrix of circular shifts A: its Gram
    matrix is the circular-autocorrelation Toeplitz matrix, accumulated in float64 and diagonalised by one-sided Jacobi
    in float64 on the GPU; h = V S^+ U^H srv, out = srv - A h.  complex64 out and taps, like the reference.

    Cut rule: a singular value is dropped when sigma < max(1e-10, rcond * sigma_max).  The reference has the absolute
    1e-10 alone, which its own float32 SVD rarely reaches: on a band-limited reference it inverts singular values of
    1e-8 sigma_max and returns noise.  ``rcond=None`` is 4 sqrt(T) 2^-26 with T = filterLen + peek (3.0e-7 at 26 taps):
    what a Gram matrix accumulated in float64 cannot tell from its own rounding.  ``rcond=0`` is the reference's rule.

    Returns out, then the taps with ``return_filter``, then the singular values of A (float64, descending) with
    ``return_singular_values``.  Raises PrcoreError if the Jacobi sweeps did not converge within their cap (30)."""
    _check_same(refChannel, srvChannel)
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64).reshape(-1)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64).reshape(-1)
    n = ref.shape[0]
    T = int(filterLen) + int(peek)
    wsb = engine.ls_svd_workspace_bytes(n, filterLen, peek, 1)      # the size limits (1 <= T < n, T <= 4096): ValueError
    st = engine.staging()
    d_ref = st.get("svd_ref", 8 * n)
    d_srv = st.get("svd_srv", 8 * n)
    d_out = st.get("svd_out", 8 * n)
    d_taps = st.get("svd_taps", 16 * T)
    d_sv = st.get("svd_sv", 8 * T)
    d_info = st.get("svd_info", 12)
    d_ws = st.get("svd_ws", wsb)
    d_ref.upload(ref)
    d_srv.upload(srv)
    engine.ls_svd_execute(d_ref, d_srv, d_out, n, filterLen, peek, rcond, 1, n, n, d_taps, d_sv, d_info, d_ws)
    kept, sweeps, converged = (int(v) for v in d_info.download((3,), np.int32))
    if not converged:
        raise _lib.PrcoreError(_lib.PRC_EUNSUPPORTED, f"LS_Filter_SVD: the Jacobi sweeps did not converge within {sweeps} sweeps")
    res = [d_out.download((n,), np.complex64).reshape(np.shape(srvChannel))]
    if return_filter:
        res.append(d_taps.download((T,), np.complex128).astype(np.complex64))
    if return_singular_values:
        res.append(d_sv.download((T,), np.float64))
    return res[0] if len(res) == 1 else tuple(res)


def ECA_Filter(refChannel, srvChannel, filterLen, sampleRate, dopplerBins=[0], peek=10, reg=0.0, return_filter=False):
    """Joint multi-Doppler least-squares canceller (the extensive cancellation algorithm of Colone et al.): the taps of every
    bin of ``dopplerBins`` from ONE least-squares problem, where LS_Filter_Multiple cancels one bin after another on the
    previous bin's output -- one Gauss-Seidel sweep over subspaces that are far from orthogonal (a 1 Hz shift over a 0.5 s
    block correlates at 0.64 with its neighbour), which leaves some 20 dB of slowly fluctuating clutter behind.

    Regressors r_a = roll(frequency_shift(ref, f_a, sampleRate), -peek), normal equations and output in
    LS_Filter_Toeplitz's convention (csrc/eca.hip); with one bin this is LS_Filter_Multiple(..., [f]).  ``reg`` >= 0 is added
    to the diagonal of the normal equations.  Bins closer than 1 / (block duration) make them ill-conditioned: that is what
    ``reg`` is for; duplicate bins or an all-zero reference with reg = 0 break the recursion down and raise PrcoreError.

    Returns complex128 values of the device's complex64 stream, like LS_Filter_Multiple; with ``return_filter`` also the
    taps, complex128 (len(dopplerBins), filterLen + peek).  Empty ``dopplerBins`` return srvChannel."""
    _check_same(refChannel, srvChannel)
    bins = [float(b) for b in dopplerBins]
    if not bins:
        return srvChannel
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64).reshape(-1)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64).reshape(-1)
    n, B = ref.shape[0], len(bins)
    T = int(filterLen) + int(peek)
    wsb = engine.eca_workspace_bytes(n, filterLen, peek, B, 1)      # the size limits: ValueError
    st = engine.staging()
    d_ref = st.get("eca_ref", 8 * n)
    d_srv = st.get("eca_srv", 8 * n)
    d_out = st.get("eca_out", 8 * n)
    d_taps = st.get("eca_taps", 16 * B * T)
    d_info = st.get("eca_info", 4)
    d_ws = st.get("eca_ws", wsb)
    d_ref.upload(ref)
    d_srv.upload(srv)
    engine.eca_execute(d_ref, d_srv, d_out, n, filterLen, peek, float(sampleRate), bins, float(reg), 1, n, n, d_taps, d_info, d_ws)
    if int(d_info.download((1,), np.int32)[0]):
        raise _lib.PrcoreError(_lib.PRC_EUNSUPPORTED, "ECA_Filter: the block Levinson recursion broke down (singular normal "
                               "equations: duplicate bins or a silent reference); pass reg > 0")
    out = d_out.download((n,), np.complex64).reshape(np.shape(srvChannel)).astype(np.complex128)
    if return_filter:
        return out, d_taps.download((B, T), np.complex128)
    return out


def _echo_lists(lags, dopplers, nframes, n, stacked):
    """HOST prc_echo_atom records [nframes, max_atoms] and counts from per-frame lists, validated as the header asks of a
    host-built list: ValueError for lags that are not whole samples, |lag| >= n or a Doppler that is not finite"""
    if not stacked:
        lags, dopplers = [lags], [dopplers]
    if len(lags) != nframes or len(dopplers) != nframes:
        raise ValueError(f"a stack of {nframes} frames takes {nframes} lists of lags and of dopplers")
    per = []
    for l, f in zip(lags, dopplers):
        l = np.atleast_1d(np.asarray(l))
        f = np.atleast_1d(np.asarray(f, dtype=np.float64))
        if l.ndim != 1 or l.shape != f.shape:
            raise ValueError("lags and dopplers must be one-dimensional and of the same length")
        if l.size and not np.all(l == np.rint(l)):
            raise ValueError("echo lags are whole samples")
        l = l.astype(np.int64)
        if np.any(np.abs(l) >= n):
            raise ValueError(f"echo lag outside (-{n}, {n})")
        if not np.all(np.isfinite(f)):
            raise ValueError("echo Dopplers must be finite")
        per.append((l, f))
    M = max(l.size for l, _ in per)
    rec = np.zeros((nframes, max(M, 1)), dtype=_lib.ECHO_ATOM_DTYPE)
    counts = np.zeros(nframes, np.int32)
    for b, (l, f) in enumerate(per):
        rec["lag"][b, :l.size], rec["doppler"][b, :l.size], counts[b] = l, f, l.size
    return rec, counts, M


def cancel_echoes(refChannel, srvChannel, sampleRate, lags, dopplers, *, ramp=True, refine=2, reg=0.0, wrap=False,
                  return_fit=False):
    """Joint least-squares removal of strong echoes from the surveillance stream (CLEAN; prc_echo_cancel of include/prcore.h,
    csrc/echo.hip).  A strong moving echo of a noise-like illuminator lifts the whole range-Doppler surface by 1 / sqrt(B T)
    of its peak; the LS cancellers only reach low Doppler and short delay.  Atom k is ref delayed by ``lags[k]`` whole samples
    and shifted by ``dopplers[k]`` Hz -- an echo that refine_peaks reports at (lag, doppler) is atom (round(lag), doppler).
    All atoms are fitted at once in float64 normal equations.  ``ramp``: a Doppler-slope column (i/n - 1/2) a_k beside every
    atom, which absorbs a Doppler error of a fraction of a cell; ``refine``: Gauss-Newton updates of the Dopplers from the
    slope amplitudes before the final fit (needs ramp; from whole cells one update reaches the noise floor).  ``reg`` >= 0 is
    added to the diagonal.  ``wrap``: circular delays (fast_xambg's convention) instead of zeros from outside the frame.

    Channels are 1-D, or [nframes, n] stacks with per-frame lists ``lags`` / ``dopplers``; NumPy arrays (staged) or torch
    device tensors (zero copy, torch's current stream).  Returns the cleaned stream, complex64, of the same kind and shape;
    with ``return_fit`` also the refined Dopplers, the complex128 amplitudes and slopes and the flags (host arrays; lists of
    them for a stack).  At most 32 atoms per frame.  Duplicate atoms or a silent reference with reg = 0 break the solve down and
    raise PrcoreError (reading that costs one small device-to-host copy).  Empty lists return srvChannel."""
    _check_same(refChannel, srvChannel)
    if len(refChannel.shape) not in (1, 2):
        raise ValueError("cancel_echoes takes one-dimensional channels or [nframes, n] stacks")
    stacked = len(refChannel.shape) == 2
    n = int(refChannel.shape[-1])
    nframes = int(refChannel.shape[0]) if stacked else 1
    if n < 1 or nframes < 1:
        raise ValueError("cancel_echoes: empty channels")
    rec, counts, M = _echo_lists(lags, dopplers, nframes, n, stacked)
    if M == 0:
        return srvChannel
    desc = engine.echo_desc(n, sampleRate, M, nframes, wrap, ramp, refine, reg)      # the option checks: ValueError
    nws = engine.echo_workspace_bytes(desc)
    side = residence.of(refChannel)
    shape = tuple(srvChannel.shape)
    ref = side.put("echo_ref", refChannel, np.complex64)
    srv = side.put("echo_srv", srvChannel, np.complex64)
    out = side.empty("echo_out", shape, np.complex64)
    d_rec = side.put("echo_rec", rec.view(np.uint8).reshape(-1), np.uint8)
    d_cnt = side.put("echo_cnt", counts, np.int32)
    d_fit = side.scratch("echo_fit", nframes * M * _lib.ECHO_FIT_DTYPE.itemsize)
    d_info = side.empty("echo_info", (nframes,), np.int32)
    ws = side.scratch("echo_ws", nws)
    with side.device():
        engine.echo_execute(desc, ref, srv, d_rec, d_cnt, out, d_fit, d_info, ws, side.stream)
        info = side.fetch(d_info, (nframes,), np.int32)
        out = side.result(out, shape, np.complex64)
        fit = side.fetch(d_fit, (nframes, M), _lib.ECHO_FIT_DTYPE) if return_fit else None
    if info.any():
        raise _lib.PrcoreError(_lib.PRC_EUNSUPPORTED, "cancel_echoes: the Cholesky factorisation broke down (singular normal "
                               "equations: duplicate atoms or a silent reference); pass reg > 0")
    if not return_fit:
        return out
    per = [tuple(np.array(fit[b, :counts[b]][k]) for k in ("doppler", "amp", "slope", "flags")) for b in range(nframes)]
    if not stacked:
        return (out,) + per[0]
    return (out,) + tuple([p[i] for p in per] for i in range(4))


def NLMS_filter(refChannel, srvChannel, filterLen, mu, peek=10, initialTaps=None, returnFilter=False):
    """Normalised LMS canceller (:189-249), one wavefront on the GPU.  complex64 out/taps."""
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64)
    if ref.shape[0] < srv.shape[0]:
        raise IndexError("refChannel shorter than srvChannel")
    n = srv.shape[0]
    st = engine.staging()
    d_tin = None
    if initialTaps is not None:                               # :218-225
        taps0 = np.ascontiguousarray(initialTaps, dtype=np.complex64)
        filterLen = taps0.shape[0] - peek
        d_tin = st.get("nlms_tin", 8 * taps0.shape[0])
        d_tin.upload(taps0)
    T = int(filterLen) + int(peek)
    d_ref = st.get("nlms_ref", 8 * n)
    d_srv = st.get("nlms_srv", 8 * n)
    d_out = st.get("nlms_out", 8 * n)
    d_tout = st.get("nlms_tout", 8 * T)
    d_ref.upload(ref[:n])
    d_srv.upload(srv)
    engine.nlms_execute(d_ref, d_srv, d_out, n, filterLen, mu, peek, d_tin, d_tout, 1)
    out = d_out.download((n,), np.complex64)
    if returnFilter:
        return out, d_tout.download((T,), np.complex64)
    return out


def _gal_check(refChannel, srvChannel, latticeLen, delayLineLen):
    """the reference's argument errors (:294-303), raised before the library is touched"""
    _check_same(refChannel, srvChannel)
    if int(latticeLen) > int(delayLineLen):
        raise ValueError("Delay line order must be greater than or equal to the lattice filter order")
    if int(latticeLen) < 1:
        # the reference fails on a NumPy broadcast error here (b[latticeLen:] = bo[latticeLen-1:-1])
        raise ValueError(f"latticeLen must be at least 1, got {latticeLen}")


def GAL_JPE(refChannel, srvChannel, latticeLen, delayLineLen, mu1, mu2, peek=10, return_filter=False):
    """Gradient adaptive lattice joint-process estimator (:251-365), one wavefront per call on the GPU
    (a workgroup beyond 2048 delay-line taps).  Inputs are cast to complex64, as NLMS_filter does; out,
    and with ``return_filter`` the reflection coefficients k and transversal taps h (length
    delayLineLen each), are complex64 like the reference's."""
    _gal_check(refChannel, srvChannel, latticeLen, delayLineLen)
    ref = np.ascontiguousarray(refChannel, dtype=np.complex64).reshape(-1)
    srv = np.ascontiguousarray(srvChannel, dtype=np.complex64).reshape(-1)
    n = ref.shape[0]
    L, D = int(latticeLen), int(delayLineLen)
    if n == 0:
        out = np.zeros(0, np.complex64)
        zk = np.zeros(D, np.complex64)
        return (out, zk, zk.copy()) if return_filter else out
    st = engine.staging()
    d_ref = st.get("gal_ref", 8 * n)
    d_srv = st.get("gal_srv", 8 * n)
    d_out = st.get("gal_out", 8 * n)
    d_k = st.get("gal_k", 8 * D) if return_filter else None
    d_h = st.get("gal_h", 8 * D) if return_filter else None
    wsb = engine.gal_workspace_bytes(D, 1)
    d_ws = st.get("gal_ws", wsb) if wsb else None
    d_ref.upload(ref)
    d_srv.upload(srv)
    engine.gal_execute(d_ref, d_srv, d_out, n, L, D, mu1, mu2, int(peek), d_k, d_h, 1, workspace=d_ws)
    out = d_out.download((n,), np.complex64).reshape(np.shape(srvChannel))
    if return_filter:
        return out, d_k.download((D,), np.complex64), d_h.download((D,), np.complex64)
    return out
