"""NumPy float64 restatement of prc_echo_cancel (include/prcore.h): joint least-squares removal of echoes at given
(lag, Doppler) with a Doppler-slope column per atom and Gauss-Newton refinement of the Dopplers.  It imports neither the
product nor the reference; tests/test_echo_host.py holds it to the figures the feature was designed on."""
import numpy as np

SKIPPED, CLAMPED, BROKE_DOWN = 1, 2, 4
FIT_DTYPE = np.dtype([("doppler", "<f8"), ("amp", "<c16"), ("slope", "<c16"), ("flags", "<u4"), ("reserved", "<u4")])


def atom(ref, lag, doppler, sample_rate, wrap):
    """a[i] = ref[idx(i - lag)] exp(+j 2 pi doppler i / sample_rate) in float64; the phase argument is reduced exactly"""
    n = ref.shape[0]
    i = np.arange(n)
    m = i - int(lag)
    if wrap:
        v = ref[m % n].astype(np.complex128)
    else:
        ok = (m >= 0) & (m < n)
        v = np.where(ok, ref[np.clip(m, 0, n - 1)], 0).astype(np.complex128)
    # turns = frac(f i / Fs) without losing digits at large f i: f / Fs is reduced first, the product is split
    ft = np.float64(doppler) / np.float64(sample_rate)
    ft = ft - np.rint(ft)
    return v * np.exp(2j * np.pi * _frac_product(ft, i))


def _frac_product(ft, i):
    """frac(ft * i) for integer i, via longdouble (64-bit mantissa on x86; n < 2^31 leaves 2^-33 turns at worst)"""
    p = np.longdouble(ft) * i.astype(np.longdouble)
    return (p - np.rint(p)).astype(np.float64)


def columns(ref, lags, dopplers, sample_rate, wrap, ramp):
    n = ref.shape[0]
    x = np.arange(n) / n - 0.5
    cols = []
    for lag, f in zip(lags, dopplers):
        a = atom(ref, lag, f, sample_rate, wrap)
        cols.append(a)
        if ramp:
            cols.append(x * a)
    return np.stack(cols, axis=1) if cols else np.zeros((n, 0), np.complex128)


def gram(A, srv, reg):
    G = A.conj().T @ A + reg * np.eye(A.shape[1])
    g = A.conj().T @ srv.astype(np.complex128)
    return G, g


def pivots_ok(G):
    """the breakdown rule of the definition: every Cholesky pivot finite and above 2^-40 of its own diagonal entry of G (in
    exact arithmetic: > 0)"""
    C = G.shape[0]
    L = np.zeros_like(G)
    for j in range(C):
        d = (G[j, j] - np.sum(L[j, :j] * np.conj(L[j, :j]))).real
        if not np.isfinite(d) or not d > 2.0 ** -40 * G[j, j].real:
            return False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (G[j + 1:, j] - L[j + 1:, :j] @ np.conj(L[j, :j])) / L[j, j]
    return True


def cancel(ref, srv, sample_rate, lags, dopplers, wrap=False, ramp=True, refine=2, reg=0.0, return_cond=False):
    """One frame.  Returns (out complex64, fit records [len(lags)] in the caller's order, info).  Atoms with |lag| >= n or
    a Doppler that is not finite are skipped (flag bit 0) and the rest fitted as if they were not listed."""
    n = ref.shape[0]
    lags = [int(v) for v in lags]
    dopplers = [float(v) for v in dopplers]
    fit = np.zeros(len(lags), FIT_DTYPE)
    good = [j for j in range(len(lags)) if abs(lags[j]) < n and np.isfinite(dopplers[j])]
    for j in range(len(lags)):
        if j not in good:
            fit["flags"][j] |= SKIPPED
    if refine > 0 and not ramp:
        raise ValueError("refine needs ramp")
    if not good:
        return (srv.astype(np.complex64).copy(), fit, 0) + ((1.0,) if return_cond else ())
    L = [lags[j] for j in good]
    f = np.array([dopplers[j] for j in good], np.float64)
    clamped = np.zeros(len(good), bool)
    step = 2 if ramp else 1
    cond = 1.0
    for it in range(refine + 1):
        A = columns(ref, L, f, sample_rate, wrap, ramp)
        G, g = gram(A, srv, reg)
        cond = max(cond, float(np.linalg.cond(G))) if np.all(np.isfinite(G)) else np.inf
        broke = False
        broke = not pivots_ok(G)
        if not broke:
            c = np.linalg.solve(G, g)
            broke = not np.all(np.isfinite(c))
        if broke:
            fit["flags"][good] |= BROKE_DOWN
            return (srv.astype(np.complex64).copy(), fit, 1) + ((cond,) if return_cond else ())
        if it == refine:
            break
        ca, cs = c[0::2], c[1::2]
        for k in range(len(good)):
            if ca[k] == 0 or not np.isfinite(ca[k]):
                continue
            d = (cs[k] / ca[k]).imag / (2 * np.pi)
            if not np.isfinite(d):
                continue
            if abs(d) > 0.5:
                d = 0.5 if d > 0 else -0.5
                clamped[k] = True
            f[k] += d * sample_rate / n
    out = (srv.astype(np.complex128) - A @ c).astype(np.complex64)
    fit["doppler"][good] = f
    fit["amp"][good] = c[0::step]
    if ramp:
        fit["slope"][good] = c[1::2]
    fit["flags"][good] |= np.where(clamped, CLAMPED, 0).astype(np.uint32)
    return (out, fit, 0) + ((cond,) if return_cond else ())


def implied_dopplers(fit, sample_rate, n):
    """what the final fit says the Dopplers are: the record's Doppler plus the update its own slope amplitude asks for"""
    with np.errstate(all="ignore"):
        d = np.where(fit["amp"] != 0, (fit["slope"] / np.where(fit["amp"] != 0, fit["amp"], 1)).imag / (2 * np.pi), 0.0)
    return fit["doppler"] + d * sample_rate / n


def echo(ref, lag, doppler, sample_rate, amp=1.0, wrap=False):
    """the echo of the definition's convention at a real amplitude (complex128)"""
    return amp * atom(ref, lag, doppler, sample_rate, wrap)


def surface(ref, srv, sample_rate, lags, dopplers):
    """|X| on whole (lag, Doppler) cells by direct correlation: X[d, l] = sum_i srv[i] conj(ref[i - lag_l]) e^{-j 2 pi f_d i / Fs}
    (an echo at (lag, f) peaks at its own cell), circular lags"""
    n = ref.shape[0]
    i = np.arange(n)
    s = srv.astype(np.complex128)
    r = ref.astype(np.complex128)
    out = np.empty((len(dopplers), len(lags)))
    prods = [s * np.conj(np.roll(r, int(l))) for l in lags]
    for a, f in enumerate(dopplers):
        w = np.exp(-2j * np.pi * f * i / sample_rate)
        for b, p in enumerate(prods):
            out[a, b] = abs(np.dot(p, w))
    return out


def design_scene(seed=5, n=6001):
    """The scene the feature was designed on: white complex64 reference, Fs = n Hz (one Doppler cell is 1 Hz); a unit echo
    at (7, 3.3 Hz) and a 0.5 echo at (12, -2.7 Hz) mask a 4e-3 echo at (9, -5.6 Hz); noise at 1e-3."""
    rng = np.random.default_rng(seed)
    fs = float(n)
    ref = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    noise = 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    srv = (echo(ref, 7, 3.3, fs, 1.0, True) + echo(ref, 12, -2.7, fs, 0.5, True) + echo(ref, 9, -5.6, fs, 4e-3, True) + noise)
    return ref, srv.astype(np.complex64), fs
