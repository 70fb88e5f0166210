"""NumPy restatement of the five signal_utils functions that passiveradar_amd/csrc/preproc.hip computes (decimate,
channel_preprocessing, shift, offset_compensation, normalize): float32 taps and the reference's float32 rotation, float64
sums.  tests/test_preproc_host.py holds it to goldens written by the reference itself (tools/gen_golden_preproc.py); the GPU
tests hold the kernels to it where no golden exists.

``emulate_tile`` / ``emulate_direct`` restate the two kernels' own float32 summation ORDER (products and sums rounded
separately: NumPy has no fused multiply-add); their error against the goldens sets the GPU accuracy bar."""
import numpy as np
from scipy.signal import firwin

TILE_MAX_Q = 59          # PRC_FIRDEC_TILE_MAX_Q
TILE_OUTPUTS = 256       # outputs per workgroup of the tile form


def taps32(q):
    return firwin(20 * q + 1, 1.0 / q, window="hamming").astype(np.float32)


def out_len(n, q):
    return -(-n // q)


def _padded(x, q):
    """x (n, k) with the zeros every output's window can reach: index i of the result is sample i - 10 q"""
    n = x.shape[0]
    m = out_len(n, q)
    xp = np.zeros(((m - 1) * q + 20 * q + 1,) + x.shape[1:], x.dtype)
    xp[10 * q:10 * q + n] = x
    return xp, m


def fir_decimate(x, q, h=None, dtype=np.complex128):
    """y[j] = sum_k h[k] x[j q + 10 q - k], zeros outside, along axis 0; sums in ``dtype``"""
    x = np.asarray(x)
    h = (taps32(q) if h is None else h).astype(np.float64)
    flat = x.reshape(x.shape[0], -1).astype(dtype)
    xp, m = _padded(flat, q)
    y = np.zeros((m, flat.shape[1]), dtype)
    for k in range(20 * q + 1):
        # sample j q + 10 q - k sits at index j q + 20 q - k of the padded copy
        y += h[k] * xp[20 * q - k:20 * q - k + (m - 1) * q + 1:q]
    return y.reshape((m,) + x.shape[1:])


def result_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype in (np.complex64, np.complex128, np.float32, np.float64):
        return dtype
    return np.dtype(np.complex128 if dtype.kind == "c" else np.float64)


def decimate(x, q):
    x = np.asarray(x)
    y = fir_decimate(x, q, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    return y.astype(result_dtype(x.dtype))


def deinterleave(raw):
    raw = np.asarray(raw)
    n = raw.shape[0] // 2
    return (raw[0:2 * n:2].astype(np.float32) + 1j * raw[1:2 * n:2].astype(np.float32)).astype(np.complex64)


def rotation(n, fc, Fs, start=0):
    """exp(j ph) as frequency_shift with a scalar phase of 0 computes it: ph = fl32(fl32(fl32(2 pi fc) fl32(i)) fl32(1 / fl32(Fs))),
    float32 sin / cos, for samples start .. start + n - 1"""
    i = np.arange(start, start + n).astype(np.float32)
    ph = (np.float32(2 * np.pi * fc) * i) * (np.float32(1.0) / np.float32(Fs))
    assert ph.dtype == np.float32
    return (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64)


def tuned(raw, fc, Fs):
    """frequency_shift(deinterleave_IQ(raw), fc, Fs): complex64 product"""
    z = deinterleave(raw)
    return (z * rotation(z.shape[0], fc, Fs)).astype(np.complex64)


def channel_preprocessing(sig, dec, fc, Fs):
    return fir_decimate(tuned(sig, fc, Fs), dec).astype(np.complex64)


def shift(x, n):
    x = np.asarray(x)
    if n == 0:
        return x
    e = np.zeros_like(x)
    L = x.shape[0]
    if n > 0 and n < L:
        e[n:] = x[:L - n]
    elif n < 0 and -n < L:
        e[:L + n] = x[-n:]
    return e


def normalize(x):
    x = np.asarray(x)
    y = x / np.mean(np.abs(x).astype(np.float64))
    return y.astype(result_dtype(x.dtype))


def white(n, seed, k=None):
    rng = np.random.default_rng(seed)
    shape = (n,) if k is None else (n, k)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def raw_int8(nscalars, seed):
    return np.random.default_rng(seed).integers(-128, 128, nscalars, dtype=np.int8)


# ---- the kernels' own summation order in float32 ------------------------------------------------------------------------
def emulate_tile(x, q):
    """the tile form: per output, phases p = 0 .. q-1 in turn, taps i = 0 .. 19 of each (h[i q + p] meets
    x[(j + 10 - i) q - p]), and tap 20 of phase 0 at the end of phase 0; float32 products and sums"""
    x = np.asarray(x, np.complex64).reshape(-1)
    h = taps32(q)
    xp, m = _padded(x, q)
    j = np.arange(m)
    re, im = np.zeros(m, np.float32), np.zeros(m, np.float32)
    for p in range(q):
        for i in list(range(20)) + ([20] if p == 0 else []):
            v = xp[(j + 10 - i) * q - p + 10 * q]
            re = re + h[i * q + p] * v.real
            im = im + h[i * q + p] * v.imag
    assert re.dtype == np.float32
    return re + 1j * im


def emulate_direct(x, q):
    """the direct form: lane l sums taps l, l + 64, ... in order, then the xor tree 32, 16, 8, 4, 2, 1"""
    x = np.asarray(x, np.complex64).reshape(-1)
    h = taps32(q)
    xp, m = _padded(x, q)
    j = np.arange(m)
    lanes = np.zeros((64, m), np.complex64)
    for k in range(20 * q + 1):
        v = xp[j * q + 20 * q - k]
        l = k % 64
        lanes[l] = (lanes[l].real + h[k] * v.real) + 1j * (lanes[l].imag + h[k] * v.imag)
    off = 32
    while off:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off >>= 1
    return lanes[0]


# ---- the cases of tests/golden/preproc_*.npz (tools/gen_golden_preproc.py writes them, the tests regenerate the inputs) ----
# (n, q): the six of the pinned agreement; n one less than, equal to and one more than one and two tiles of 256 outputs (and
# of q); filters longer than the signal; both sides of the tile / direct switch, and q = 97
DECIMATE_CASES = [(1000, 4), (1003, 7), (257, 10), (50, 3), (5, 4), (4096, 16),
                  (1023, 4), (1024, 4), (1025, 4), (2047, 4), (2048, 4), (2049, 4), (767, 3), (768, 3), (769, 3),
                  (37, 10), (1, 2), (599, 59), (700, 59), (700, 60), (599, 60), (3000, 97)]
DECIMATE_DTYPES = ["complex128", "float32", "float64", "int16"]      # n = 500, q = 5
# name -> (raw dtype, scalars, dec, fc, Fs)
CHANNEL_CASES = {"i8_2001": ("int8", 2001, 10, 1e5, 2.4e6), "i8_2000": ("int8", 2000, 10, 1e5, 2.4e6),
                 "i16_odd": ("int16", 3001, 7, 5e4, 2.4e6), "f32_odd": ("float32", 3000, 7, 5e4, 2.4e6),
                 "u8": ("uint8", 2400, 10, 1e5, 2.4e6), "neg_fc": ("int8", 2400, 4, -2.5e5, 2.4e6)}
LONG_SAMPLES = 2 ** 24 + 70000       # fl32(i) rounds from 2^24 on
LONG_KEEP = 300
LONG_SEED = 660
SHIFT_LEN = 20
SHIFTS = [1, -1, SHIFT_LEN - 1, SHIFT_LEN, SHIFT_LEN + 3, -SHIFT_LEN, -(SHIFT_LEN + 3)]
OFFSETS = [0, 12, -12]               # x2 = shift(x1, d); white complex64 of 40 000, ns 20 000, ndec 4, nlag 200
NORMALIZE_SHAPES = [(1,), (7,), (3, 4), (100000,)]
NORMALIZE_STRIDE = 97                # the golden keeps every 97th value of the flattened result


def decimate_input(n, q, k=None):
    return white(n, 100000 * q + n, k)


def dtype_input(name):
    z = white(500, 5005) * 100
    if name == "complex128":
        return z.astype(np.complex128)
    if name == "int16":
        return np.round(z.real * 20).astype(np.int16)
    return z.real.astype(name)


def raw_input(dtype, nscalars, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return rng.standard_normal(nscalars).astype(np.float32)
    info = np.iinfo(dtype)
    lo, hi = (info.min, info.max) if dtype != "int16" else (-2048, 2047)
    return rng.integers(lo, hi + 1, nscalars).astype(dtype)


def channel_input(name):
    dtype, nscalars, _, _, _ = CHANNEL_CASES[name]
    return raw_input(dtype, nscalars, sum(map(ord, name)))


def long_input():
    return raw_int8(2 * LONG_SAMPLES, LONG_SEED)


def checksum(raw):
    """(sum, sum of squares, CRC32) of an integer or byte-viewed array"""
    import zlib
    b = np.ascontiguousarray(raw)
    a = b.view(np.int8).astype(np.int64)
    return np.array([int(a.sum()), int((a * a).sum()), int(zlib.crc32(b.tobytes()))], np.int64)


def shift_inputs():
    return {"c64": white(SHIFT_LEN, 31), "i8": raw_int8(3 * SHIFT_LEN, 32).reshape(SHIFT_LEN, 3)}


def offset_input():
    return white(40000, 41)


def normalize_input(shape, dtype):
    n = int(np.prod(shape))
    z = white(n, 50 + n)
    x = (z if dtype == "complex64" else z.real).astype(dtype)
    if n >= 7:
        x[n // 3:n // 3 + max(n // 10, 2)] = 0            # a run of zeros inside the data
    return x.reshape(shape)
