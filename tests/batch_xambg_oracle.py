"""The definition of prc_batch_xambg and prc_ofdm_timing (include/prcore.h) in float64 NumPy, a float32 emulation of the
surface, and the cases the host and GPU tests share.

    batch j:   r_j[t] = ref[start + j hop + t], s_j likewise, t = 0 .. L - 1;  Rj = DFT_L(r_j), Sj = DFT_L(s_j);
               P_j = sum_t |r_j[t]|^2;  G_j(f) = 1 (matched) or 1 / max(|Rj(f)|^2, floor^2 P_j), 0 where that maximum is 0;
               c_j(d) = (1 / L) sum_f G_j(f) Rj(f) conj(Sj(f)) e^{-2 pi i f d / L},  d = 0 .. R
    surface:   y[j][k] = w[j] c_j(R - k);  out = fftshift_rows(DFT_F over j of y), (F, R + 1)

``surface`` is that with scipy.fft in float64: what every test holds the device to.  ``surface_direct`` is the same definition
by direct summation -- every DFT a sum over its index in ascending order, complex products written out in real arithmetic --
and ``surface_brute`` the scalar loops over (j, d, f) with the same twiddle table: the two agree bit for bit (the vectorised
index algebra against the loops), and ``surface`` agrees with them to rounding (tests/test_batch_xambg_host.py).

``emulate32`` follows the device's number formats: complex64 transforms (scipy.fft keeps single precision), float32 P, G and
pointwise products.  On the design scene it differs from ``surface`` by 0.4e-7 (L = 1024) to 1.2e-7 (L = 4096, matched) of the
peak; GPU_BAR = 2e-6 is the project's CAF parity bar, and the host test holds the emulation to a quarter of it.
Timing: every product of two float32 values is exact in float64 and the sums run in float64, so the metric does not depend
on the order of the sums beyond a few units of 2^-53 of the sum of the magnitudes: TIMING_BAR = 1e-10 of the metric's peak."""
import functools

import numpy as np
import scipy.fft

GPU_BAR = 2e-6
TIMING_BAR = 1e-10
MATCHED, RECIPROCAL = "matched", "reciprocal"


def rel_err(got, want):
    """max|got - want| / max|want|"""
    got, want = np.asarray(got), np.asarray(want)
    return float(np.abs(got - want).max() / np.abs(want).max())


def _batches(x, L, hop, start, F, dtype):
    x = np.asarray(x)
    assert x.ndim == 1 and start >= 0 and hop >= 1 and start + (F - 1) * hop + L <= x.shape[0]
    return np.stack([x[start + j * hop:start + j * hop + L] for j in range(F)]).astype(dtype)


def profiles(ref, srv, L, hop, start, F, R, filt=RECIPROCAL, floor=0.1):
    """c_j(d), complex128 [F, R + 1]"""
    assert 0 <= R < L and filt in (MATCHED, RECIPROCAL)
    r, s = _batches(ref, L, hop, start, F, np.complex128), _batches(srv, L, hop, start, F, np.complex128)
    Rj, Sj = scipy.fft.fft(r, axis=1), scipy.fft.fft(s, axis=1)
    G = np.ones((F, L))
    if filt == RECIPROCAL:
        P = np.sum(np.abs(r) ** 2, axis=1)
        m = np.maximum(np.abs(Rj) ** 2, (float(floor) ** 2 * P)[:, None])
        G = np.divide(1.0, m, out=np.zeros_like(m), where=m > 0)
    # (1 / L) sum_f X(f) e^{-2 pi i f d / L} = conj(ifft(conj(X)))[d]
    return np.conj(scipy.fft.ifft(G * np.conj(Rj) * Sj, axis=1))[:, :R + 1]


def doppler(c, window=None):
    """the surface of the batch profiles c [F, R + 1]: columns reversed, windowed, DFT over the batches, rows fftshift-ed"""
    y = c[:, ::-1]
    if window is not None:
        y = y * np.asarray(window, dtype=np.float32).astype(np.float64)[:, None]
    return np.fft.fftshift(scipy.fft.fft(y, axis=0), axes=0)


def surface(ref, srv, L, F, R, hop=None, start=0, filt=RECIPROCAL, floor=0.1, window=None):
    """the definition: complex128 [F, R + 1]"""
    return doppler(profiles(ref, srv, L, L if hop is None else hop, start, F, R, filt, floor), window)


def stack(ref, srv, *a, **kw):
    """``surface`` per frame of [nframes, n] stacks"""
    return np.stack([surface(r, s, *a, **kw) for r, s in zip(ref, srv)])


def emulate32(ref, srv, L, F, R, hop=None, start=0, filt=RECIPROCAL, floor=0.1, window=None):
    """the surface in the device's number formats: complex64 transforms, float32 P, G and pointwise products"""
    hop = L if hop is None else hop
    r, s = _batches(ref, L, hop, start, F, np.complex64), _batches(srv, L, hop, start, F, np.complex64)
    Rj, Sj = scipy.fft.fft(r, axis=1), scipy.fft.fft(s, axis=1)
    assert Rj.dtype == np.complex64
    g = np.full((F, L), np.float32(1.0 / L), np.float32)
    if filt == RECIPROCAL:
        P = np.sum(r.real * r.real + r.imag * r.imag, axis=1, dtype=np.float32)
        m = np.maximum(Rj.real * Rj.real + Rj.imag * Rj.imag, (np.float32(floor) * np.float32(floor) * P)[:, None])
        g = np.divide(np.float32(1.0 / L), m, out=np.zeros_like(m), where=m > 0)
    W = (np.conj(Rj) * Sj) * g
    c = np.conj(scipy.fft.ifft(W, axis=1) * np.float32(L))[:, :R + 1]
    y = c[:, ::-1]
    if window is not None:
        y = y * np.asarray(window, dtype=np.float32)[:, None]
    out = np.fft.fftshift(scipy.fft.fft(np.ascontiguousarray(y, dtype=np.complex64), axis=0), axes=0)
    assert out.dtype == np.complex64
    return out


# ---- the same definition by direct summation (tiny sizes) ------------------------------------------------------------------
def twiddles(N):
    """(cos, sin) of 2 pi m / N, m = 0 .. N - 1: the table both direct forms index"""
    a = 2.0 * np.pi * np.arange(N) / N
    return np.cos(a), np.sin(a)


def _dft_seq(xr, xi, sign, cs, sn):
    """X[..., k] = sum_t x[..., t] e^{sign 2 pi i k t / N}, the sum over t in ascending order, products in real arithmetic"""
    N = xr.shape[-1]
    k = np.arange(N)
    Xr, Xi = np.zeros(xr.shape), np.zeros(xr.shape)
    for t in range(N):
        c, s = cs[(k * t) % N], sign * sn[(k * t) % N]
        a, b = xr[..., t:t + 1], xi[..., t:t + 1]
        Xr = Xr + (a * c - b * s)
        Xi = Xi + (a * s + b * c)
    return Xr, Xi


def surface_direct(ref, srv, L, F, R, hop=None, start=0, filt=RECIPROCAL, floor=0.1, window=None):
    hop = L if hop is None else hop
    r, s = _batches(ref, L, hop, start, F, np.complex128), _batches(srv, L, hop, start, F, np.complex128)
    cs, sn = twiddles(L)
    Rr, Ri = _dft_seq(r.real.copy(), r.imag.copy(), -1.0, cs, sn)
    Sr, Si = _dft_seq(s.real.copy(), s.imag.copy(), -1.0, cs, sn)
    G = np.ones((F, L))
    if filt == RECIPROCAL:
        P = np.zeros(F)
        for t in range(L):
            P = P + (r.real[:, t] * r.real[:, t] + r.imag[:, t] * r.imag[:, t])
        m = np.maximum(Rr * Rr + Ri * Ri, (float(floor) * float(floor) * P)[:, None])
        G = np.divide(1.0, m, out=np.zeros_like(m), where=m > 0)
    # X = G R conj(S);  c(d) = (1 / L) sum_f X(f) e^{-2 pi i f d / L}
    Xr, Xi = G * (Rr * Sr + Ri * Si), G * (Ri * Sr - Rr * Si)
    cr, ci = _dft_seq(Xr, Xi, -1.0, cs, sn)
    cr, ci = cr[:, :R + 1] / L, ci[:, :R + 1] / L
    w = np.ones(F) if window is None else np.asarray(window, dtype=np.float32).astype(np.float64)
    yr, yi = (cr[:, ::-1] * w[:, None]).T.copy(), (ci[:, ::-1] * w[:, None]).T.copy()     # [k][j]
    cf, sf = twiddles(F)
    Yr, Yi = _dft_seq(yr, yi, -1.0, cf, sf)
    return np.ascontiguousarray(np.fft.fftshift((Yr + 1j * Yi).T, axes=0))


def surface_brute(ref, srv, L, F, R, hop=None, start=0, filt=RECIPROCAL, floor=0.1, window=None):
    """scalar loops over (j, d, f) and (row, k, j): Python floats, the same table, the same order of every sum"""
    hop = L if hop is None else hop
    ref, srv = np.asarray(ref).astype(np.complex128), np.asarray(srv).astype(np.complex128)
    cs, sn = (v.tolist() for v in twiddles(L))
    cf, sf = (v.tolist() for v in twiddles(F))
    fl2 = float(floor) * float(floor)
    c = [[None] * (R + 1) for _ in range(F)]
    for j in range(F):
        base = start + j * hop
        r = [(float(ref[base + t].real), float(ref[base + t].imag)) for t in range(L)]
        s = [(float(srv[base + t].real), float(srv[base + t].imag)) for t in range(L)]
        X = []
        P = 0.0
        for t in range(L):
            P = P + (r[t][0] * r[t][0] + r[t][1] * r[t][1])
        for f in range(L):
            Rr = Ri = Sr = Si = 0.0
            for t in range(L):
                co, si = cs[(f * t) % L], -1.0 * sn[(f * t) % L]
                Rr, Ri = Rr + (r[t][0] * co - r[t][1] * si), Ri + (r[t][0] * si + r[t][1] * co)
                Sr, Si = Sr + (s[t][0] * co - s[t][1] * si), Si + (s[t][0] * si + s[t][1] * co)
            g = 1.0
            if filt == RECIPROCAL:
                m = max(Rr * Rr + Ri * Ri, fl2 * P)
                g = 1.0 / m if m > 0 else 0.0
            X.append((g * (Rr * Sr + Ri * Si), g * (Ri * Sr - Rr * Si)))
        for d in range(R + 1):
            ar = ai = 0.0
            for f in range(L):
                co, si = cs[(d * f) % L], -1.0 * sn[(d * f) % L]
                ar, ai = ar + (X[f][0] * co - X[f][1] * si), ai + (X[f][0] * si + X[f][1] * co)
            c[j][d] = (ar / L, ai / L)
    w = [1.0] * F if window is None else [float(np.float32(v)) for v in window]
    out = np.zeros((F, R + 1), np.complex128)
    for row in range(F):
        for k in range(R + 1):
            ar = ai = 0.0
            for j in range(F):
                yr, yi = c[j][R - k][0] * w[j], c[j][R - k][1] * w[j]
                co, si = cf[(row * j) % F], -1.0 * sf[(row * j) % F]
                ar, ai = ar + (yr * co - yi * si), ai + (yr * si + yi * co)
            out[(row + F // 2) % F, k] = complex(ar, ai)
    return out


# ---- symbol timing --------------------------------------------------------------------------------------------------------
def timing_metric(ref, nfft, cp, nsym):
    """metric[o] = |sum_{s < nsym} sum_{t < cp} ref[o + s (nfft + cp) + t] conj(ref[o + s (nfft + cp) + t + nfft])|, float64"""
    ref = np.asarray(ref).astype(np.complex128)
    sym = nfft + cp
    assert nfft >= 2 and 1 <= cp < nfft and nsym >= 1 and (nsym + 1) * sym + nfft <= ref.shape[0]
    span = nsym * sym + cp
    p = ref[:span] * np.conj(ref[nfft:nfft + span])
    acc = np.zeros(sym, np.complex128)
    for s in range(nsym):
        for t in range(cp):
            acc += p[s * sym + t:s * sym + t + sym]
    return np.abs(acc)


def symbol_start(ref, nfft, cp, nsym):
    return int(np.argmax(timing_metric(ref, nfft, cp, nsym)))


# ---- shared inputs --------------------------------------------------------------------------------------------------------
def white(n, seed):
    """unit-power complex white noise, complex64"""
    g = np.random.default_rng(seed)
    return ((g.standard_normal(n) + 1j * g.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


DESIGN = dict(n=256 * 1152 + 1024, fs=1e6, R=64, F=256, L=1024, cp=128, hop=1152, symbol_start=37, seed=5,
              delays=(20, 40), bins=(3, -37), amps=(1.0, 0.003))


@functools.lru_cache(maxsize=4)
def design_scene(order=8):
    """(ref, srv) of the design scene: 64-QAM (order 8) or QPSK (order 2), a unit echo and one 50 dB below it"""
    from passiveradar_amd import scene
    D = DESIGN
    binhz = D["fs"] / (D["F"] * D["hop"])
    tg = [(d, b * binhz, a) for d, b, a in zip(D["delays"], D["bins"], D["amps"])]
    ref, srv = scene.make_qam_ofdm_scene(D["n"], D["fs"], D["R"], D["seed"], symbol_start=D["symbol_start"], order=order, targets=tg,
                                         clutter=[], noise_amp=1e-4)
    ref.setflags(write=False)
    srv.setflags(write=False)
    return ref, srv


def design_cells():
    """the cells of the strong and of the weak echo"""
    from passiveradar_amd import scene
    D = DESIGN
    binhz = D["fs"] / (D["F"] * D["hop"])
    return [scene.expected_peak_cell(d, b * binhz, D["F"] * D["hop"], D["fs"], D["R"], D["F"]) for d, b in zip(D["delays"], D["bins"])]


def design_args(filt=RECIPROCAL, floor=0.1):
    D = DESIGN
    return dict(L=D["L"], F=D["F"], R=D["R"], hop=D["hop"], start=D["symbol_start"] + D["cp"], filt=filt, floor=floor)


def design_conditions(X_recip, X_matched):
    """the figures the design scene is held to, from the two filters' surfaces [F, R + 1]"""
    D = DESIGN
    strong, weak = design_cells()
    A, M = np.abs(np.asarray(X_recip)), np.abs(np.asarray(X_matched))
    masked = A.copy()                                   # without the strong echo's rows (+-2) and its columns (+-1): the range
    masked[max(strong[0] - 2, 0):strong[0] + 3, :] = 0.0    # side lobes of the occupied band lie along its row, the Doppler side
    masked[:, max(strong[1] - 1, 0):strong[1] + 2] = 0.0    # lobes along its column
    return dict(peak_recip=tuple(int(v) for v in np.unravel_index(np.argmax(A), A.shape)),
                peak_matched=tuple(int(v) for v in np.unravel_index(np.argmax(M), M.shape)),
                strong=strong, weak=weak, level=float(A.max() / D["F"]),
                weak_over_median_recip=float(A[weak] / np.median(A)), weak_over_median_matched=float(M[weak] / np.median(M)),
                second=tuple(int(v) for v in np.unravel_index(np.argmax(masked), masked.shape)))


def check_design(c):
    """the design scene's conditions (tests/test_batch_xambg_host.py on the oracle, tests/test_gpu_recip_xambg.py on the device)"""
    assert c["peak_recip"] == c["strong"] and c["peak_matched"] == c["strong"], c
    assert abs(c["level"] - 769 / 1024) <= 0.02 * 769 / 1024, c
    assert c["weak_over_median_recip"] >= 20.0 and c["second"] == c["weak"], c
    assert c["weak_over_median_matched"] <= 5.0, c


def release_device_leftovers():
    """free this thread's pooled staging buffers of batch_xambg (bx_*) and ofdm_symbol_start (ot_*), so that the tests after a
    module meet the allocator as they would without it (the front doors cache no tables of their own)"""
    from passiveradar_amd import engine
    bufs = engine.staging().bufs
    for name in [n for n in bufs if n.startswith(("bx_", "ot_"))]:
        bufs.pop(name).free()
