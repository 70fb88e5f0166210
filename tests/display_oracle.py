"""NumPy restatement of the display contract: the limits of range_doppler_plot.py:75-76 and the
RGBA8 pixels matplotlib's Normalize + Colormap.__call__(bytes=True) give for them.  All arithmetic in float64, every
operation rounded on its own.  tests/test_display_host.py holds it to matplotlib; tests/test_gpu_display.py holds the
device to it."""
import numpy as np


def gnuplot2_lut():
    x = np.linspace(0, 1, 256)
    r = x / 0.32 - 0.78125
    g = 2 * x - 0.84
    b = np.zeros(256)
    m = x < 0.25
    b[m] = 4 * x[m]
    m = (x >= 0.25) & (x < 0.92)
    b[m] = -2 * x[m] + 1.84
    m = x >= 0.92
    b[m] = x[m] / 0.08 - 11.5
    lut = np.clip(np.stack([r, g, b, np.ones(256)], axis=1), 0, 1)
    return (lut * 255).astype(np.uint8)


def percentile(data, p):
    """NumPy's default (linear) percentile of the flattened data, restated: q = p/100, vi = (n-1) q, k = floor(vi),
    t = vi - k (both order statistics the last one when vi >= n-1), _lerp without FMA; NaN when a NaN is present"""
    x = np.sort(np.asarray(data, dtype=np.float64).ravel())          # NaN sorts last
    n = x.size
    if np.isnan(x[-1]):
        return np.float64(np.nan)
    vi = np.float64(n - 1) * (np.float64(p) / np.float64(100))
    if vi >= n - 1:
        a = b = x[-1]
        t = np.float64(0.0)
    else:
        k = int(np.floor(vi))
        t = vi - np.floor(vi)
        a, b = x[k], x[k + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return a + d * t if t < 0.5 else b - d * (np.float64(1.0) - t)


def limits(data, p_lo=35, p_hi=99, hi_scale=1.5):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([percentile(data, p_lo), np.float64(hi_scale) * percentile(data, p_hi)], dtype=np.float64)


def colour(data, vmin, vmax, lut):
    """RGBA8 of every cell of ``data`` (any shape) -> shape + (4,)"""
    v = np.asarray(data, dtype=np.float64)
    lut = np.asarray(lut, dtype=np.uint8)
    out = np.zeros(v.shape + (4,), np.uint8)
    vmin, vmax = np.float64(vmin), np.float64(vmax)
    if vmin > vmax:                      # matplotlib raises; the device paints the frame "bad"
        return out
    if vmin == vmax:
        out[...] = lut[0]
        return out
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xa = ((v - vmin) / (vmax - vmin)) * np.float64(256.0)
    bad = np.isnan(xa)
    idx = np.zeros(v.shape, np.int64)
    inside = ~bad & (xa >= 0) & (xa < 256)
    idx[inside] = np.trunc(xa[inside]).astype(np.int64)
    idx[~bad & (xa >= 256)] = 255
    out[...] = lut[idx]
    out[bad] = 0
    return out


def oriented(frame, orient="plot"):
    frame = np.asarray(frame)
    return np.fliplr(frame.T) if orient == "plot" else frame


def render(frame, lut=None, lim=None, p_lo=35, p_hi=99, hi_scale=1.5, orient="plot"):
    """one frame (H, W) -> (W, H, 4) for "plot", (H, W, 4) for "stored" """
    lut = gnuplot2_lut() if lut is None else lut
    lim = limits(frame, p_lo, p_hi, hi_scale) if lim is None else lim
    return np.ascontiguousarray(colour(oriented(frame, orient), lim[0], lim[1], lut))


def frame_cases(seed=7):
    """name -> float64 frame (H, W): the shapes and value patterns the display tests share"""
    rng = np.random.default_rng(seed)
    c = {}
    for H, W in ((1, 1), (2, 1), (3, 5), (37, 23), (64, 48), (1, 70), (70, 1)):
        c[f"dense_{H}x{W}"] = rng.exponential(1.0, (H, W))
    f = rng.exponential(1.0, (37, 23))
    f[rng.random((37, 23)) < 0.5] = 0.0
    c["half_zero"] = f
    c["two_values"] = np.where(rng.random((37, 23)) < 0.3, 2.5, -1.25)
    c["negative"] = rng.standard_normal((64, 48)) * 3.0 - 1.0
    f = rng.exponential(1.0, (37, 23))
    f[5, 7] = np.inf
    c["one_inf"] = f
    f = rng.exponential(1.0, (37, 23))
    f[30, 2] = np.nan
    c["one_nan"] = f
    c["all_zero"] = np.zeros((37, 23))
    c["constant"] = np.full((3, 5), 4.25)
    f = np.zeros((37, 23))
    f[::2] = -0.0
    f[3, 3] = 1.0
    c["signed_zeros"] = f
    return c
