"""NumPy oracle of the order-statistic CFAR (CFAR_2D_OS, prc_cfar_os): test infrastructure, like tests/gal_oracle.py.

The training set of cell (i, j) is X[(i + c - a) mod H, (j + c - b) mod W] for the taps (a, b) in [0, fw)^2 outside the guard
block [e1, e2)^2, c = (fw-1)//2 -- the taps of oracle/np_oracle.py::CFAR_2D's box.  The Nt rolled copies of the frame are
stacked, np.partition takes the k-th smallest per cell (in the frame's own dtype: a selection rounds nothing), and both
scales are formed in float64."""
import math

import numpy as np


def window(fw, gw):
    """(c, e1, e2) of CFAR_2D's (fw, gw) window"""
    e1 = max((fw - gw) // 2, 0)
    e2 = min(fw - e1 + 1, fw)
    return (fw - 1) // 2, e1, e2


def taps(fw, gw):
    """the (a, b) of the training cells"""
    _, e1, e2 = window(fw, gw)
    return [(a, b) for a in range(fw) for b in range(fw) if not (e1 <= a < e2 and e1 <= b < e2)]


def training_cells(fw, gw):
    _, e1, e2 = window(fw, gw)
    return fw * fw - (e2 - e1) ** 2


def default_rank(fw, gw):
    return math.ceil(0.75 * training_cells(fw, gw))


def training_stack(X, fw, gw):
    """[Nt, H, W]: plane t holds, at (i, j), training cell t of cell (i, j)"""
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("one 2-D frame")
    c = window(fw, gw)[0]
    tp = taps(fw, gw)
    if not tp:
        raise ValueError("the window has no training cell")
    return np.stack([np.roll(X, (-(c - a), -(c - b)), axis=(0, 1)) for a, b in tp])


def noise(X, fw, gw, rank=None):
    """z: the rank-th smallest (1-based) training cell per cell, + 0.0 (no -0), in X's dtype"""
    S = training_stack(X, fw, gw)
    k = default_rank(fw, gw) if rank is None else int(rank)
    if not 1 <= k <= S.shape[0]:
        raise ValueError(f"rank = {k} outside 1 .. {S.shape[0]}")
    return np.partition(S, k - 1, axis=0)[k - 1] + S.dtype.type(0)


def noise_at_ranks(X, fw, gw, ranks):
    """{rank: z} for several ranks of one frame from one sort of the stack (the same selection as ``noise``)"""
    S = np.sort(training_stack(X, fw, gw), axis=0)
    return {int(k): S[int(k) - 1] + S.dtype.type(0) for k in ranks}


def ratios(X, z, scale):
    """both scales in float64 from a frame and its z map"""
    x64, z64 = np.asarray(X).astype(np.float64), np.asarray(z).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x64 / np.mean(np.abs(x64))) / (z64 + 1e-10) if scale == "reference" else x64 / z64


def CFAR_2D_OS(X, fw, gw, thresh=None, rank=None, scale="reference", return_noise=False):
    """one real 2-D frame -> the ratio in float64 (bool with a threshold; NaN compares false)"""
    X = np.asarray(X)
    z = noise(X, fw, gw, rank)
    x64, z64 = X.astype(np.float64), z.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if scale == "reference":
            cr = (x64 / np.mean(np.abs(x64))) / (z64 + 1e-10)
        elif scale == "plain":
            cr = x64 / z64
        else:
            raise ValueError("scale is 'reference' or 'plain'")
        out = cr > thresh if thresh is not None else cr
    return (out, z) if return_noise else out


def pfa(T, ncells, rank):
    """Rohling's false-alarm probability of square-law cells in exponential noise at multiplier T"""
    m = ncells - np.arange(rank, dtype=np.float64)
    return float(np.prod(m / (m + T)))
