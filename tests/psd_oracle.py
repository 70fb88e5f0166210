"""A float64 NumPy restatement of the Welch contract of include/prcore.h (prc_welch) and passiveradar_amd/spectral.py:
matplotlib.mlab's psd / csd / specgram for complex input, sides='twosided', pad_to == NFFT, plus the rows (``navg``),
``step`` and short-input rules.  tests/test_psd_host.py holds it to matplotlib; the GPU tests use it (matplotlib is not
assumed where they run).  ``cases()`` is the table of seeded inputs both share."""
import numpy as np


def window64(window, nfft):
    return np.hanning(nfft) if window is None else np.asarray(window, dtype=np.float64)


def scale(w, Fs, scale_by_freq=True):
    return 1.0 / (Fs * (np.abs(w) ** 2).sum()) if scale_by_freq else 1.0 / np.abs(w).sum() ** 2


def segments(x, nfft, noverlap, detrend, w, step=1):
    """[nseg, nfft] complex128 spectra of the detrended, windowed segments of x[::step], natural bin order"""
    x = np.asarray(x)[::step].astype(np.complex128)
    if x.shape[0] < nfft:
        x = np.concatenate([x, np.zeros(nfft - x.shape[0], np.complex128)])
    hop = nfft - noverlap
    nseg = (x.shape[0] - nfft) // hop + 1
    seg = np.stack([x[s * hop:s * hop + nfft] for s in range(nseg)])
    if detrend == "mean":
        seg = seg - seg.mean(axis=1, keepdims=True)
    return np.fft.fft(seg * w[None, :], axis=1)


def rows_of(p, navg):
    """[nseg, nfft] per-segment values -> [rows, nfft] means (navg 0: all segments in one row), centred"""
    nseg = p.shape[0]
    k = nseg if navg == 0 else navg
    if k > nseg:
        raise ValueError("navg exceeds the number of segments")
    r = p[:(nseg // k) * k].reshape(nseg // k, k, -1).mean(axis=1)
    return np.roll(r, -(p.shape[1] // 2), axis=1)


def freqs(nfft, Fs, Fc=0):
    return np.roll(np.fft.fftfreq(nfft, 1 / Fs), -(nfft // 2)) + Fc


def welch(x, y=None, NFFT=256, Fs=2, detrend=None, window=None, noverlap=0, scale_by_freq=True, navg=0, step=1):
    """[rows, NFFT]: float64 mean |X|^2 * scale, or complex128 mean conj(X) Y * scale"""
    w = window64(window, NFFT)
    X = segments(x, NFFT, noverlap, detrend, w, step)
    if y is None:
        p = np.abs(X) ** 2
    else:
        p = np.conj(X) * segments(y, NFFT, noverlap, detrend, w, step)
    return rows_of(p, navg) * scale(w, Fs, scale_by_freq)


def psd(x, **kw):
    return welch(x, None, navg=0, **kw)[0]


def csd(x, y, **kw):
    return welch(x, y, navg=0, **kw)[0]


def specgram(x, navg=1, **kw):
    kw.setdefault("noverlap", 128)
    return welch(x, None, navg=navg, **kw).T


def times(n, NFFT, Fs, noverlap, navg=1):
    nseg = 1 if n < NFFT else (n - NFFT) // (NFFT - noverlap) + 1
    t = (NFFT / 2 + np.arange(nseg) * (NFFT - noverlap)) / Fs
    if navg == 1:
        return t
    k = nseg if navg == 0 else navg
    return t[:(nseg // k) * k].reshape(-1, k).mean(axis=1)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
def white(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


def tone60(n, seed):
    """a tone about 100 dB (in power per bin at the sizes tested) above a white floor"""
    return (np.exp(2j * np.pi * 0.1234 * np.arange(n)) + 1e-3 * white(n, seed)).astype(np.complex64)


def dc(n, seed):
    return (0.5 + 0.25j + 0.05 * white(n, seed)).astype(np.complex64)


def int8_raw(n, seed):
    """interleaved int8 I,Q scalars [2 n] and the complex64 they stand for"""
    z = white(n, seed)
    raw = np.empty(2 * n, np.int8)
    raw[0::2] = np.clip(np.round(40 * z.real), -128, 127)
    raw[1::2] = np.clip(np.round(40 * z.imag), -128, 127)
    return raw, (raw[0::2].astype(np.float32) + 1j * raw[1::2].astype(np.float32)).astype(np.complex64)


def bin_tone(nfft, k0, n):
    return np.exp(2j * np.pi * k0 * np.arange(n) / nfft).astype(np.complex64)


# nfft -> n of the parity cases: a tail that is dropped
PARITY_N = {64: 5 * 64 + 7, 256: 9 * 256 + 3, 2048: 6 * 2048 + 100, 8192: 5 * 8192 + 11}


def overlaps(nfft):
    return (0, nfft // 2, 37) + ((nfft - 1,) if nfft == 64 else ())


def parity_n(nfft, noverlap):
    return 200 if noverlap == nfft - 1 else PARITY_N[nfft]


_CASES = {}


def cases(nfft, noverlap):
    """name -> complex64 input for one (nfft, noverlap) of the parity table (built once per shape)"""
    key = (nfft, noverlap)
    if key not in _CASES:
        n = parity_n(nfft, noverlap)
        _CASES[key] = {"white": white(n, 11), "tone60": tone60(n, 12), "dc": dc(n, 13), "int8": int8_raw(n, 14)[1]}
    return _CASES[key]


_REF = {}


def psd_ref(nfft, noverlap, name, detrend):
    """the oracle's psd of a parity case, computed once"""
    key = (nfft, noverlap, name, detrend)
    if key not in _REF:
        _REF[key] = psd(cases(nfft, noverlap)[name], NFFT=nfft, Fs=2.4e6, detrend=detrend, noverlap=noverlap)
    return _REF[key]
