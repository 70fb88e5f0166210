"""NumPy model of the block arithmetic of the cached-spectrum LS chain (passiveradar_amd/csrc/ls_fft.hip,
ls_fft_team_cached.hip, ls_fft_team_corr_cached.hip): pieces of B = P - E samples with the slot origin E >= T - 1
(E = T - 1 on the 1024-point kernels, T - 1 rounded up to 16 samples on the 4096-point ones), the block spectrum
X_p = FFT(rho[n0 - E : n0 + B]) shared by the overlap-save FIR and by the "roles swapped" correlations
    sum_n s[n] conj(rho[n - k]) = sum_p IFFT( FFT(s piece in slots [E, E + cnt)) conj(X_p) )[k],   k <= T - 1,
for rho = roll(ref, -peek) taken with zeros before the block and the <= peek wrapped samples added at its end
(clutter_removal.py:139-155).  Checks the identities the kernels rely on against direct evaluation -- including that
extra history slots (E > T - 1) and the assignment of pieces to teams change nothing.  No GPU."""
import numpy as np
import pytest


def _pieces(n, B):
    return [(p * B, min(B, n - p * B)) for p in range((n + B - 1) // B)]


def _block(rho_lin, n0, E, P):
    """slots 0..P-1 <-> rho_lin[n0 - E + idx], zero outside [0, n)"""
    idx = n0 - E + np.arange(P)
    ok = (idx >= 0) & (idx < rho_lin.size)
    x = np.zeros(P, complex)
    x[ok] = rho_lin[idx[ok]]
    return x


@pytest.mark.parametrize("n,T,peek,P,E", [
    (5000, 40, 10, 1024, 39),        # 1024-point kernels: E = T - 1
    (5000, 266, 10, 1024, 265),
    (24234 + 5, 58, 10, 4096, 64),   # 4096-point kernels: E = T - 1 rounded up to 16; last piece shorter than peek
    (30000, 266, 10, 4096, 272),
    (30000, 266, 0, 4096, 272),      # peek = 0: no wrapped samples
    (9000, 769, 10, 4096, 768),
])
def test_block_identities(n, T, peek, P, E):
    rng = np.random.default_rng(n + T)
    ref = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    s = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    w = (rng.standard_normal(T) + 1j * rng.standard_normal(T)) / T
    rho = np.roll(ref, -peek)                       # clutter_removal.py:139
    B = P - E
    assert E >= T - 1 and B > 0
    X = [np.fft.fft(_block(rho, n0, E, P)) for n0, _ in _pieces(n, B)]

    # overlap-save FIR: out = s - (rho * w)[0:n] (linear convolution, :153-155), outputs taken from slots >= E
    H = np.fft.fft(np.concatenate([w, np.zeros(P - T)]))
    out = np.empty(n, complex)
    for (n0, cnt), Xp in zip(_pieces(n, B), X):
        y = np.fft.ifft(Xp * H)
        out[n0:n0 + cnt] = s[n0:n0 + cnt] - y[E:E + cnt]
    want = s - np.convolve(rho, w)[:n]
    assert np.abs(out - want).max() < 1e-10 * np.abs(want).max()

    # correlations with the roles swapped: the piece in slots [E, E + cnt), zeros elsewhere; lags 0 .. T-1
    def corr(sig, order):
        acc = np.zeros(P, complex)
        for p in order:
            n0, cnt = _pieces(n, B)[p]
            u = np.zeros(P, complex)
            u[E:E + cnt] = sig[n0:n0 + cnt]
            acc += np.fft.fft(u) * np.conj(X[p])
        return np.fft.ifft(acc)[:T]
    npc = len(X)
    direct = np.array([np.sum(s[k:] * np.conj(rho[:n - k])) for k in range(T)])          # xcorr, :145-147
    strided = corr(s, [p for t in range(3) for p in range(t, npc, 3)])                    # pieces team, team + 3, ...
    per = -(-npc // 3)
    runs = corr(s, [p for t in range(3) for p in range(t * per, min((t + 1) * per, npc))])  # a contiguous run per team
    scale = np.abs(direct).max()
    assert np.abs(strided - direct).max() < 1e-10 * scale and np.abs(runs - direct).max() < 1e-10 * scale
    auto = corr(rho, range(npc))
    direct_auto = np.array([np.sum(rho[k:] * np.conj(rho[:n - k])) for k in range(T)])   # :142-144
    assert np.abs(auto - direct_auto).max() < 1e-10 * np.abs(direct_auto).max()


def test_piece_size_of_the_4096_point_chain():
    """ltc_piece (ls_team_cached.h): B = 4096 - E with E = T - 1 rounded up to 16 samples -- every piece of a 128-byte
    aligned stream then starts on a 128-byte line, and E still covers the T - 1 samples of history the FIR needs"""
    for T in (2, 17, 18, 250, 266, 273, 769):
        E = (T - 1 + 15) & ~15
        B = 4096 - E
        assert E >= T - 1 and E - (T - 1) < 16 and (B * 8) % 128 == 0 and B > 0


# ---- the shared-inverse solve on coloured references ----------------------------------------------------------------
# ls.hip's cached chain solves every Doppler bin from ONE Levinson-Durbin run on c_0 (the unrotated reference):
#     c_f[k] = e^{j theta k} ( c_0[k] + (gamma - 1) S_e[k] ),   x = D T_0^{-1} D^H b  + nref refinement steps
# against the exact Toeplitz(c_f).  The host picks nref from |gamma - 1| 10 peek / N (white-noise reasoning); the solve
# kernels then measure their last two corrections and fall back to a Levinson solve of Toeplitz(c_f) when the error
# they leave, ~ |dx_k|^2 / |dx_{k-1}|, exceeds 1e-8 |x| (CHAIN_TOL2).  Restated here in float64, so that a change to
# either rule shows on the CPU first.

def _lagcorr(x, y, T):
    """sum_{n >= k} x[n] conj(y[n - k]), k < T, float64 (FFT)"""
    m = 1 << int(np.ceil(np.log2(2 * x.size)))
    return np.fft.ifft(np.fft.fft(x, m) * np.conj(np.fft.fft(y, m)))[:T]


def _nref(theta, n, peek):
    """ls.hip run_cached_chain: refinement steps from est = |gamma - 1| 10 peek / N (k steps leave ~ est^(k+1))"""
    est = abs(np.exp(-1j * theta * n) - 1.0) * 10.0 * peek / n if theta != 0.0 else 0.0
    k, left = 0, est
    while left > 1e-9 and k < 4:
        k, left = k + 1, left * est
    return k


def _chain_model(ref, srv, L, fs, bins, peek=10, guard=True):
    """(model output, exact output, fallbacks taken) of the chain on complex64 inputs, both in float64; the exact one
    solves every bin's Toeplitz(c_f) directly (what the oracle's per-bin Levinson does)"""
    from scipy.linalg import solve_toeplitz, toeplitz
    n, T = ref.size, L + peek
    rho = np.roll(ref.astype(np.complex128), -peek)
    c0 = _lagcorr(rho, rho, T)
    t0inv = np.linalg.inv(toeplitz(c0, np.conj(c0)))
    ym, ye = srv.astype(np.complex128), srv.astype(np.complex128)
    idx, fallbacks = np.arange(n), 0
    for f in bins:
        # effective slope of the reference's float32 ramp, fl32(2 pi f) fl32(1/Fs); the ramp restarts for the wrapped
        # samples (r_f = roll(ref e^{j phi}, -peek))
        theta = float(np.float32(2 * np.pi * f)) * float(np.float32(1.0) / np.float32(fs)) if f else 0.0
        rf = rho * np.exp(1j * theta * ((idx + peek) % n))
        cf = _lagcorr(rf, rf, T)
        tf = toeplitz(cf, np.conj(cf))
        D = np.exp(1j * theta * np.arange(T))
        b = _lagcorr(ym, rf, T)
        nref = _nref(theta, n, peek)
        dx = D * (t0inv @ (np.conj(D) * b))
        x, norms = dx, [np.vdot(dx, dx).real]
        for _ in range(nref):
            dx = D * (t0inv @ (np.conj(D) * (b - tf @ x)))
            x = x + dx
            norms.append(np.vdot(dx, dx).real)
        if guard and nref >= 1 and not norms[-1] ** 2 <= 1e-16 * np.vdot(x, x).real * norms[-2]:
            x = solve_toeplitz((cf, np.conj(cf)), b)
            fallbacks += 1
        ym = ym - np.convolve(rf, x)[:n]
        ye = ye - np.convolve(rf, solve_toeplitz((cf, np.conj(cf)), _lagcorr(ye, rf, T)))[:n]
    return ym, ye, fallbacks


def _excess(y, y_opt, L):
    core = slice(2 * L, y_opt.size - 2 * L)
    d = y[core] - y_opt[core]
    return float(np.vdot(d, d).real / np.vdot(y_opt[core], y_opt[core]).real)


@pytest.mark.parametrize("family", ["fm", "ofdm", "ar2", "white"])
@pytest.mark.parametrize("n,L,bins", [
    (40000, 64, (0.0, 1.0, -1.0, 2.0, -2.0)),      # the cached chain's shortest blocks (n >= 2000 peek)
    (40000, 64, (0.0, 0.5, -37.3)),
    (40000, 256, (0.0, 1.0, -1.0, 2.0, -2.0)),
    (262144, 64, (0.0, 1.0, -1.0, 2.0, -2.0)),
])
def test_shared_inverse_chain_on_coloured_references(family, n, L, bins):
    """E <= 1e-8 against the exact per-bin solve; without the guard the refinement alone leaves E up to 1e-4 on FM
    and diverges on OFDM (spectral radius of the iteration > 1) at 40000 samples"""
    from passiveradar_amd import scene
    make = {"fm": scene.make_fm_scene, "ofdm": scene.make_ofdm_scene, "ar2": scene.make_ar2_scene,
            "white": scene.make_scene}[family]
    ref, srv = make(n, 262184.87, L, 6200 + L, targets=(), noise_amp=1e-3)
    ym, ye, fallbacks = _chain_model(ref, srv, L, 262184.87, bins)
    e = _excess(ym, ye, L)
    assert e <= 1e-8, (e, fallbacks)
    if family == "white":
        assert fallbacks == 0                       # the guard costs nothing on a white reference
    if family in ("fm", "ofdm") and n == 40000:
        ym0, _, _ = _chain_model(ref, srv, L, 262184.87, bins, guard=False)
        assert _excess(ym0, ye, L) > 1e-6           # the white-noise rule alone is not enough here


def _corr_fft32(x, y, T, P):
    """sum_{n >= k} x[n] conj(y[n - k]), k < T, as the FFT correlation kernels form it (ls_fft.hip, ls_fft_team.hip):
    pieces of B = P - (T - 1) samples of x in slots [T - 1, P), the matching P-sample block of y, complex64 P-point
    transforms, conj(U) V-style products accumulated in complex64 in the frequency domain over the pieces a wave (or
    team) owns -- here all of them, the longest run the kernels can have -- and one complex64 inverse transform"""
    from scipy import fft as sfft
    n, E = x.size, T - 1
    B = P - E
    acc = np.zeros(P, np.complex64)
    for n0 in range(0, n, B):
        cnt = min(B, n - n0)
        u = np.zeros(P, np.complex64)
        u[E:E + cnt] = x[n0:n0 + cnt]
        idx = n0 - E + np.arange(P)
        ok = (idx >= 0) & (idx < n)
        v = np.zeros(P, np.complex64)
        v[ok] = y[idx[ok]]
        acc += sfft.fft(u) * np.conj(sfft.fft(v))
    return sfft.ifft(acc)[:T].astype(np.complex128)


def _ls_emulated(ref, srv, L, fs, bins, corr, peek=10):
    """LS_Filter_Multiple (one bin: LS_Filter_Toeplitz) with the correlations formed by `corr`, the solve and the FIR in
    float64: the error the float32 correlation sums alone leave"""
    from oracle import np_oracle as O
    n, T, out = ref.size, L + peek, srv.astype(np.complex128)
    for f in bins:
        r = np.roll(ref if f == 0 else O.frequency_shift(ref, f, fs), -peek).astype(np.complex64)
        cur = out.astype(np.complex64)                  # the device streams complex64 between bins
        w = O.levinson_hermitian(corr(r, r, T), corr(cur, r, T))
        out = cur.astype(np.complex128) - np.convolve(r.astype(np.complex128), w)[:n]
    return out


# (family, filterLen, bins, transform size, lo, hi): the cases test_gpu_conditioning.py holds to FLOOR_BAR on the FFT
# kernels (1024-point up to 769 taps, 4096-point team kernels beyond), each with the floor this emulation puts it at;
# with float64 correlations E is ~1e-12 on all of them
FFT_FLOOR_CASES = [
    ("ar2", 64, (0.0,), 1024, 3e-6, 1e-4),
    ("ar2", 256, (0.0,), 1024, 3e-6, 2e-4),
    ("ar2", 1024, (0.0,), 4096, 3e-6, 1e-4),
    ("ofdm", 1024, (0.0,), 4096, 3e-6, 1e-4),
    ("fm", 256, (0.0,), 1024, 1e-6, 1e-4),
    ("fm", 640, (0.0,), 1024, 1e-7, 1e-4),
    ("ofdm", 640, (0.0,), 1024, 1e-7, 1e-4),
    ("ofdm", 1024, (0.0, 1.0, -1.0), 4096, 3e-5, 3e-4),     # three chained 1034-tap solves
]


@pytest.mark.parametrize("family,L,bins,P,lo,hi", FFT_FLOOR_CASES)
def test_fft_correlation_floor(family, L, bins, P, lo, hi):
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    n, fs = 40000, 262184.87
    make = {"fm": scene.make_fm_scene, "ofdm": scene.make_ofdm_scene, "ar2": scene.make_ar2_scene}[family]
    ref, srv = make(n, fs, L, {"fm": 6200, "ofdm": 6300, "ar2": 6400}[family] + L, targets=(), noise_amp=1e-3)
    y_opt = O.LS_Filter_Multiple(ref, srv, L, fs, list(bins))
    e = _excess(_ls_emulated(ref, srv, L, fs, bins, lambda x, y, T: _corr_fft32(x, y, T, P)), y_opt, L)
    print(f"{family} T={L + 10} {len(bins)} bin(s), {P}-point float32 correlation: E = {e:.2e}")
    assert lo <= e < hi, e


def _corr_runs32(x, y, T, run=32):
    """sum_{n >= k} x[n] conj(y[n - k]), k < T, as the time-domain kernel forms it (ls.hip corr_partial_kernel): one lane
    per lag, complex64 products accumulated in float32 over runs of 32 samples, the runs added in double (and the waves
    and blocks in double, through the split float partials)"""
    n, out = x.size, np.empty(T, np.complex128)
    for k in range(T):
        p = (x[k:] * np.conj(y[:n - k])).astype(np.complex64)
        m = -(-p.size // run) * run
        pp = np.zeros(m, np.complex64)
        pp[:p.size] = p
        out[k] = np.cumsum(pp.reshape(-1, run), axis=1, dtype=np.complex64)[:, -1].astype(np.complex128).sum()
    return out


# (family, n, filterLen, sample rate, bins, lo, hi): the cases test_gpu_conditioning.py holds to a floor on the
# time-domain kernel (DIRECT_FLOOR there); the device measures 1.2e-5 .. 6.2e-5 on them
DIRECT_FLOOR_CASES = [
    ("ar2", 40000, 256, 262184.87, (0.0,), 3e-6, 1e-4),
    ("ofdm", 40000, 1024, 262184.87, (0.0,), 3e-6, 1e-4),
    ("ofdm", 40000, 1024, 262184.87, (0.0, 1.0, -1.0), 1e-5, 1e-4),
    ("ar2", 40960, 64, 262144.0, (0.0, 6.4, -6.4, 12.8), 3e-6, 1e-4),
]


@pytest.mark.parametrize("family,n,L,fs,bins,lo,hi", DIRECT_FLOOR_CASES)
def test_time_domain_correlation_floor(family, n, L, fs, bins, lo, hi):
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    make = {"fm": scene.make_fm_scene, "ofdm": scene.make_ofdm_scene, "ar2": scene.make_ar2_scene}[family]
    ref, srv = make(n, fs, L, {"fm": 6200, "ofdm": 6300, "ar2": 6400}[family] + L, targets=(), noise_amp=1e-3)
    y_opt = O.LS_Filter_Multiple(ref, srv, L, fs, list(bins))
    e = _excess(_ls_emulated(ref, srv, L, fs, bins, _corr_runs32), y_opt, L)
    print(f"{family} T={L + 10} {len(bins)} bin(s), float32 runs of 32: E = {e:.2e}")
    assert lo <= e < hi, e
