"""NumPy statement of the polyphase filter bank passiveradar_amd/csrc/channelize.hip computes (signal_utils.channelize,
prc_channelize):

    y[i][j] = sum_{t < L} h[t] x[j D + c - t] w^((k_i (start + j D + c - t)) mod M),   w = exp(-2 pi i / M),  c = (L - 1) / 2,

x zero outside [0, n), j < ceil(n / D).  ``channelize`` is that definition in float64: float32 taps as given, float64
twiddles, the phase index an integer.  tests/test_channelize_host.py holds it to an independent statement (rotate the
stream, then preproc_oracle.fir_decimate).

``emulate_tile`` / ``emulate_direct`` restate the two kernels' own float32 summation ORDER with the float32 twiddle table
(products and sums rounded separately: NumPy has no fused multiply-add); their error against the definition sets the GPU
accuracy bar."""
import numpy as np
from scipy.signal import firwin

import preproc_oracle as P

MAX_SEL = 64               # PRC_CHANNELIZE_MAX_SEL: rows per launch, the wrapper splits above
TILE_OUTPUTS = 256         # output times per workgroup of the tile form
TILE_MAX_BYTES = 163840    # PRC_CHANNELIZE_TILE_MAX_BYTES
# the GPU tests' accuracy bar: 4 x the worst error of the emulations below against the definition (4.4e-7), rounded up to one
# digit; tests/test_channelize_host.py recomputes it
GPU_BAR = 2e-6
DTYPES = ["int8", "uint8", "int16", "float32", "complex64"]


def taps32(D):
    return P.taps32(D)


def out_len(n, D):
    return -(-n // D)


def tile_bytes(D, L):
    """LDS bytes of the tile form: D rows of (256 + ceil(c / D) + floor(c / D) + 1) float2, the length made odd"""
    c = (L - 1) // 2
    return ((TILE_OUTPUTS + -(-c // D) + c // D + 1) | 1) * D * 8


def is_tile(D, L):
    return tile_bytes(D, L) <= TILE_MAX_BYTES


def to_complex(sig):
    """the complex samples of a raw array (interleaved I,Q scalars, a trailing odd scalar ignored) or a complex stream"""
    sig = np.asarray(sig)
    return sig.astype(np.complex64) if np.iscomplexobj(sig) else P.deinterleave(sig)


def fold(channels, M):
    return np.mod(np.asarray(channels, np.int64), M)


def twiddles64(M):
    """w^e, e < M"""
    return np.exp(-2j * np.pi * np.arange(M) / M)


def twiddles32(M):
    """the device table: (cos, sin)(2 pi r / M) in float64, rounded to float32"""
    ang = 2.0 * np.pi * np.arange(M, dtype=np.float64) / M
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _taps(D, taps):
    h = taps32(D) if taps is None else np.asarray(taps, np.float32)
    assert h.ndim == 1 and h.shape[0] % 2 == 1
    return h


def _gather(x, s):
    """x[s], zero where s is outside [0, n)"""
    inside = (s >= 0) & (s < x.shape[0])
    return np.where(inside, x[np.clip(s, 0, x.shape[0] - 1)], 0)


def channelize(sig, M, D, channels=None, taps=None, start=0):
    """the definition, tap by tap, in float64 / complex128: (K, ceil(n / D))"""
    x = to_complex(sig).astype(np.complex128)
    h = _taps(D, taps).astype(np.float64)
    k = fold(np.arange(M) if channels is None else channels, M)
    L, n = h.shape[0], x.shape[0]
    c = (L - 1) // 2
    j = np.arange(out_len(n, D), dtype=np.int64)
    W = twiddles64(M)
    y = np.zeros((k.shape[0], j.shape[0]), np.complex128)
    if n == 0:
        return y
    for t in range(L):
        s = j * D + c - t
        e = (k[:, None] * ((start + s) % M)[None, :]) % M        # Python ints / int64: exact at any start
        y += h[t] * _gather(x, s)[None, :] * W[e]
    return y


def rotated(sig, M, k, start=0):
    """x[m] exp(-2 pi i ((k (start + m)) mod M) / M) in complex128: the stream tuned to channel k, its phase exact"""
    x = to_complex(sig).astype(np.complex128)
    m = np.arange(x.shape[0], dtype=np.int64)
    e = (int(k) % M * ((start + m) % M)) % M
    return x * np.exp(-2j * np.pi * e / M)


# ---- the kernels' own summation order in float32 ------------------------------------------------------------------------
def emulate_tile(sig, M, D, channels=None, taps=None, start=0):
    """the tile form: tap phases p = 0 .. min(M, L) - 1 in turn; inside one, taps t = p, p + M, ... into u_p (re and im on
    their own); after each p every channel adds tw[(k p) mod M] u_p into its own accumulator (re: + w.re u.re, then
    - w.im u.im; im: + w.re u.im, then + w.im u.re); at the end acc conj(tw[(k (start + j D + c)) mod M])"""
    x = to_complex(sig)
    h = _taps(D, taps)
    k = fold(np.arange(M) if channels is None else channels, M)
    L, n = h.shape[0], x.shape[0]
    c = (L - 1) // 2
    j = np.arange(out_len(n, D), dtype=np.int64)
    cs, sn = twiddles32(M)
    ax = np.zeros((k.shape[0], j.shape[0]), np.float32)
    ay = np.zeros_like(ax)
    for p in range(min(M, L)):
        ux, uy = np.zeros(j.shape[0], np.float32), np.zeros(j.shape[0], np.float32)
        for t in range(p, L, M):
            v = _gather(x, j * D + c - t)
            ux = ux + h[t] * v.real.astype(np.float32)
            uy = uy + h[t] * v.imag.astype(np.float32)
        e = (k * p) % M
        wx, wy = cs[e][:, None], sn[e][:, None]
        ax = ax + wx * ux
        ax = ax + (-wy) * uy
        ay = ay + wx * uy
        ay = ay + wy * ux
    e = (k[:, None] * ((start + j * D + c) % M)[None, :]) % M
    tx, ty = cs[e], sn[e]
    re = ax * tx + ay * ty
    im = ay * tx - ax * ty
    assert re.dtype == np.float32 and im.dtype == np.float32
    return re + 1j * im


def emulate_direct(sig, M, D, channels=None, taps=None, start=0):
    """the direct form: lane l sums taps l, l + 64, ... in order, each term h[t] (x conj(tw[e])) with the exact table
    index e of its own sample; then the xor tree 32, 16, 8, 4, 2, 1"""
    x = to_complex(sig)
    h = _taps(D, taps)
    k = fold(np.arange(M) if channels is None else channels, M)
    L, n = h.shape[0], x.shape[0]
    c = (L - 1) // 2
    j = np.arange(out_len(n, D), dtype=np.int64)
    cs, sn = twiddles32(M)
    lx = np.zeros((64, k.shape[0], j.shape[0]), np.float32)
    ly = np.zeros_like(lx)
    for t in range(L):
        s = j * D + c - t
        v = _gather(x, s)
        vx, vy = v.real.astype(np.float32)[None, :], v.imag.astype(np.float32)[None, :]
        e = (k[:, None] * ((start + s) % M)[None, :]) % M
        tx, ty = cs[e], sn[e]
        zx = vx * tx + vy * ty
        zy = vy * tx - vx * ty
        l = t % 64
        lx[l] = lx[l] + h[t] * zx
        ly[l] = ly[l] + h[t] * zy
    off = 32
    while off:
        idx = np.arange(64) ^ off
        lx, ly = lx + lx[idx], ly + ly[idx]
        off >>= 1
    assert lx.dtype == np.float32
    return lx[0] + 1j * ly[0]


# ---- cases: (n samples, M, D, channels), the smallest shapes at which each thing can go wrong ---------------------------
ALL8 = list(range(8))
CASES = [
    (2000, 12, 12, [0, 1, -1, 5, 6]),        # M = D, with the Nyquist channel and a negative index
    (2001, 24, 12, [0, 3, -7, 23]),          # M = 2 D
    (1025, 8, 4, ALL8),                      # D | M, and n = 4 * 256 + 1: one output into a second tile
    (777, 5, 7, [0, 1, 2, -2]),              # coprime pair, prime M
    (300, 64, 3, [0, 31, 32, -1]),           # L = 61 < M: some tap phases are empty
    (37, 12, 10, [1]),                       # filter longer than the signal
    (1, 4, 2, [0, 3]),                       # a single input sample
    (4100, 100, 50, [0, 17, -33]),           # large M
    # one less than, exactly and one more than one and two tiles of 256 outputs
    (765, 4, 3, [0, 1, -1]), (768, 4, 3, [0, 1, -1]), (769, 4, 3, [0, 1, -1]),
    (1533, 4, 3, [0, 1, -1]), (1536, 4, 3, [0, 1, -1]), (1537, 4, 3, [0, 1, -1]),
    # either side of the tile / direct switch with the default taps: D = 73 is the last tile that fits
    (600, 8, 73, [1, 3]), (600, 8, 74, [1, 3]),
]
assert is_tile(73, 20 * 73 + 1) and not is_tile(74, 20 * 74 + 1)
# custom odd tap vectors whose length is not 20 D + 1: name -> (n, M, D, channels, L, cut-off as a fraction of Nyquist)
CUSTOM = {"short": (500, 12, 5, [0, 5, -1], 33, 1 / 6), "one_tap": (130, 6, 1, [0, 2, 3], 1, None),
          "long": (900, 10, 4, [0, 3, -4], 301, 1 / 5)}
FAR_START = 2 ** 40 + 12345


def custom_taps(name):
    _, _, _, _, L, cut = CUSTOM[name]
    if cut is None:
        return np.array([0.75], np.float32)
    return firwin(L, cut, window="hamming").astype(np.float32)


def case_seed(n, M, D):
    return 1000003 * M + 1009 * D + n


def case_input(n, M, D, dtype="int8"):
    """the raw array of a case: 2 n interleaved scalars of the dtype, or n complex64 samples"""
    seed = case_seed(n, M, D) + DTYPES.index(dtype)
    if dtype == "complex64":
        return P.white(n, seed)
    return P.raw_input(dtype, 2 * n, seed)


def all_cases():
    """(label, n, M, D, channels, taps or None) of every case, custom taps included"""
    out = [(f"{n}_{M}_{D}", n, M, D, ch, None) for n, M, D, ch in CASES]
    out += [(name, v[0], v[1], v[2], v[3], custom_taps(name)) for name, v in CUSTOM.items()]
    return out


def rel_err(a, b):
    """max|a - b| / max|b|, the peak-normalised error"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ---- what the GPU test modules leave on the device ------------------------------------------------------------------------
def device_tables():
    """the keys of the small per-device tables (decimation taps, twiddles) cached so far"""
    from passiveradar_amd import signal_utils
    with signal_utils._taps_lock:
        return set(signal_utils._taps)


def release_device_leftovers(tables_before):
    """free what a module's channelize calls left resident -- the tables cached since ``tables_before`` and this thread's pooled
    ``cz_*`` staging buffers -- so that the tests after it meet the allocator as they would without it
    (tests/test_gpu_lifetime.py measures free device memory to the MiB)"""
    from passiveradar_amd import engine, signal_utils
    with signal_utils._taps_lock:
        for key in set(signal_utils._taps) - set(tables_before):
            signal_utils._taps.pop(key).free()
    bufs = engine.staging().bufs
    for name in [n for n in bufs if n.startswith("cz_")]:
        bufs.pop(name).free()
