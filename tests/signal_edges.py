"""Inputs off unit amplitude and on dead air for the signal-processing entry points, and what to expect of them.

Shared by tests/test_signal_edges_host.py (the oracles: every expectation below is itself under test there) and
tests/test_gpu_signal_edges.py (the kernels).

Amplitude ladder.  ``ref`` is multiplied by 2^a and ``srv`` by 2^b, a != b (unequal exponents tell a swapped channel or a
wrong degree).  In the normal range every IEEE add, multiply, fma, divide and sqrt commutes with a power of two, and so does
the mantissa-only hardware rcp / rsq: an entry point of degree (da, db) in (ref, srv) without an absolute constant returns
its scale-0 result times 2^(da a + db b), bit for bit.

Exponent budget.  Inputs are of unit amplitude, the degree is at most 2 and a sum has at most 2^17 terms.  With |a|, |b| <= 24
a product of two scaled samples is within 2^+-48 of the unit-amplitude product and a sum of 2^17 of them within 2^(17+48) of
one; the entry points that carry an absolute constant get one rung further out (LS_Filter_SVD with ref at 2^-42: squares at
2^-84, summed in float64).  Every result stays inside 2^+-100 with float32's normal range at 2^+-126, so nothing overflows
and nothing that matters is subnormal.  ``budget`` asserts this on the float64 oracle output before anything is launched;
``scaled`` asserts that every scaling was exact (scaling back returns the same bits).

Dead air.  Finite inputs only: silent streams (all zeros), dropouts (a run of exact zeros) and constant streams.
"""
import functools

import numpy as np

# (a, b): two negative and two positive exponents for either channel, int16 full scale (+15) and +-24 among them; the
# sums a + b (8, 9, -14, 14) are all different from zero and from each other
LADDER = ((15, -7), (24, -15), (-24, 10), (-10, 24))
BUDGET = 100


def pow2(e):
    return float(np.ldexp(1.0, int(e)))


def _real_type(x):
    return np.finfo(np.asarray(x).dtype).dtype.type


def scaled(x, e):
    """x * 2^e in x's own dtype, exact: scaling back returns the same bits (nothing overflowed, nothing went subnormal)"""
    x = np.asarray(x)
    t = _real_type(x)
    with np.errstate(over="ignore", under="ignore"):
        y = x * t(pow2(e))
        assert y.dtype == x.dtype
        assert same_bits(y * t(pow2(-e)), x), f"scaling by 2^{e} was not exact"
    return y


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({4: np.uint32, 8: np.uint64}[_real_type(a)(0).itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def diff_report(got, want):
    """'' when the bits agree, else how many elements differ, where first and by how much (peak-normalised)"""
    got, want = np.asarray(got), np.asarray(want)
    if same_bits(got, want):
        return ""
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"dtype/shape {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(got.size, -1).any(axis=1))
    with np.errstate(all="ignore"):
        peak = np.abs(want[np.isfinite(want)]).max() if np.isfinite(want).any() else np.nan
        err = np.nanmax(np.abs(got.reshape(-1)[bad] - want.reshape(-1)[bad])) / peak
    return f"{bad.size} of {got.size} elements differ in bits, first at {int(bad[0])}, worst {err:.3g} of the peak"


def budget(oracle_out, da, db, ladder=LADDER, extra=()):
    """assert that the float64 oracle's result of degree (da, db), scaled for every rung, stays inside 2^+-BUDGET"""
    peak = float(np.abs(np.asarray(oracle_out)).max())
    assert np.isfinite(peak) and peak > 0.0
    for a, b in tuple(ladder) + tuple(extra):
        e = np.log2(peak) + da * a + db * b
        assert -BUDGET < e < BUDGET, f"peak 2^{e:.1f} at exponents ({a}, {b}) leaves the exponent budget"


def expected(out0, da, db, a, b):
    """the scale-0 result carried to exponents (a, b) of (ref, srv): out0 * 2^(da a + db b), exactly"""
    return scaled(out0, da * a + db * b)


def first_nonfinite(x):
    """index of the first sample that is not finite, None when all are"""
    bad = np.flatnonzero(~np.isfinite(np.asarray(x).reshape(-1)))
    return int(bad[0]) if bad.size else None


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def pair(n, seed, rangeBins=20, fs=1.0e4):
    """(ref, srv): the white-reference scene the parity tests use, complex64, read-only, made once per shape"""
    from passiveradar_amd import scene
    return _frozen(*scene.make_scene(n, fs, rangeBins, seed))


@functools.lru_cache(maxsize=None)
def white(n, seed):
    rng = np.random.default_rng(seed)
    return _frozen((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))


@functools.lru_cache(maxsize=None)
def raw_float32(nscalars, seed):
    """interleaved I,Q scalars as a float32 recording holds them"""
    return _frozen(np.random.default_rng(seed).standard_normal(nscalars).astype(np.float32))


def silent(n, dtype=np.complex64):
    return np.zeros(n, dtype)


def hole(x, start, length):
    """x with x[start:start + length] = 0 (an SDR dropout)"""
    y = np.array(x)
    y[start:start + length] = 0
    return y


def constant_raw(dtype, nscalars, i, q):
    """a recording stuck at one (I, Q) pair -- full scale included"""
    raw = np.empty(nscalars, dtype)
    raw[0::2] = i
    raw[1::2] = q
    return raw


def full_scale(dtype):
    """(I, Q) at the two ends of an integer type's range, (1, -1) for float32"""
    if np.dtype(dtype).kind == "f":
        return 1.0, -1.0
    info = np.iinfo(dtype)
    return info.max, info.min


# ---- shapes: the smallest rows of the existing parametrisations that still reach each kernel form --------------------------
CAF_N, CAF_R, CAF_F = 8192, 70, 256            # 1024-point and time-domain segment kernels; 256 bins: both Doppler methods
CAF_TEAM = (131072, 2048, 32)                  # 4096-point team kernel, two pieces of 2048 + the direct tail sample
CAF_MULTI = (65536, 300, 16)                   # 4096-point multi call: one full piece + a remainder piece
LS_N, LS_L = 16384, 32                         # every LS method; 16384 >= 8192: method 4 runs the 4096-point chain
LS_FS, LS_BINS = 1.0e4, (0.0, 1.0, -1.0)       # the three-bin chain
LS_TEAM_L = 790                                # T = 800 > 769: the team kernels
LS_TEAM_N = 3 * (LS_TEAM_L + 10) + 5000
NLMS_L, NLMS_N, NLMS_MU = 24, 1500, 0.05       # one wavefront
NLMS_LONG_L = 2039                             # T = 2049: a workgroup of two wavefronts
NLMS_LONG_N = NLMS_LONG_L + 10 + 700
NLMS_STREAMS, NLMS_STREAM_N, NLMS_STRIDE = 5, 500, 512
GAL_N, GAL_L, GAL_D, GAL_MU1, GAL_MU2 = 700, 8, 64, 2e-3, 2e-2
CFAR_H, CFAR_W, CFAR_FW, CFAR_GW = 33, 64, 7, 2
SVD_N, SVD_L, SVD_PEEK = 1021, 17, 10

# the exponent at which each absolute constant meets the quantity it guards
GAL_EDGE = -17        # b^H b + 1e-10: 64 taps of |ref|^2 ~ 2^-34 give ~ 1e-9 .. 1e-10
CFAR_EDGE = -33       # box + 1e-10: a box mean of ~ 2^-33 = 1.2e-10
LS_REG_EDGE = -7      # Gram diagonal n |ref|^2 + reg: 16384 * 2^-14 = 1 against reg = 1
SVD_ABOVE = -36       # sigma ~ sqrt(n) |ref| = 2^5 * 2^-36 = 4.7e-10: every direction just above the 1e-10 cut
SVD_BELOW = -42       # ... 7.3e-12: every direction below it, nothing is cancelled


def nlms_first_nonfinite(filterLen, start):
    """a dropout ref[start:start + m] = 0 with m > T = filterLen + peek: the tap window u_k = ref[k+1 .. k+T] is all zero
    first at k = start - 1; that step's error still uses finite taps (out[filterLen + start - 1] is finite), its update
    divides 0 by 0, and the next output, out[filterLen + start], is the first that is not finite"""
    return filterLen + start
