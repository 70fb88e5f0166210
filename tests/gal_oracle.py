"""NumPy restatement of the reference's GAL_JPE (passiveRadar/clutter_removal.py:251-365) in the prefix-sum form the
kernel (passiveradar_amd/csrc/gal.hip) uses.  Per sample n (x = ref[n + peek], bo = the previous step's b):

    f[m] = x - sum_{j=1..m} conj(k[j]) bo[j-1]                         m < L   (an inclusive prefix sum)
    b[0] = x;  b[m] = bo[m-1] - k[m] f[m-1] (1 <= m < L);  b[m] = bo[m-1] (L <= m < D)
    P[m-1] = 0.9 P[m-1] + 0.19 (|f[m-1]|^2 + |bo[m-1]|^2);   k[m] += mu1 grad / (P[m-1] + 1e-10)
    e = srv[n] - h^H b;  h += mu2 conj(e) b / (b^H b + 1e-10);  mu1 = min(0.999 mu1 + 1e-8 e^2, 5e-3)

``dtype`` is the dtype of the lattice state (b, k, P, h); the reference keeps it complex64.  The inputs keep their own
dtype, so e, h and mu1 promote exactly as in the reference (complex128 inputs carry h and e in complex128 there).
mu1 is complex (e^2, not |e|^2) and the cap compares in NumPy's lexicographic complex order."""
import numpy as np


def gal_jpe(ref, srv, L, D, mu1, mu2, peek=10, dtype=np.complex64, return_filter=False, stats=None):
    ref = np.asarray(ref)
    srv = np.asarray(srv)
    if ref.shape != srv.shape:
        raise ValueError("Input vectors must have the same length")
    if L > D or L < 1:
        raise ValueError("lattice length must be in [1, delay-line length]")
    ct = np.dtype(dtype)
    rt = np.finfo(ct).dtype
    N = ref.shape[0]
    b = np.zeros(D, ct)
    k = np.zeros(D, ct)
    P = np.full(D, 1e-8, rt)
    h = np.zeros(D, ct)
    out = np.zeros(srv.shape, np.result_type(ct, np.complex64))
    caps = 0
    for n in range(max(N - peek - 1, 0)):
        x = ct.type(ref[n + peek])
        bo = b
        c = np.conj(k[1:L]) * bo[:L - 1]
        f = np.empty(L, ct)
        f[0] = x
        f[1:] = x - np.cumsum(c)
        b = np.empty(D, ct)
        b[0] = x
        b[1:L] = bo[:L - 1] - k[1:L] * f[:L - 1]
        b[L:] = bo[L - 1:D - 1]
        E = np.abs(f[:L - 1]) ** 2 + np.abs(bo[:L - 1]) ** 2
        P[:L - 1] = rt.type(0.9) * P[:L - 1] + rt.type(1.0 - 0.9 ** 2) * E
        grad = np.conj(f[:L - 1]) * b[1:L] + bo[:L - 1] * np.conj(f[1:L])
        k[1:L] = k[1:L] + mu1 * grad / (P[:L - 1] + 1e-10)      # rounded into k's dtype on assignment
        e = srv[n] - np.vdot(h, b)
        h = h + mu2 * np.conj(e) * b / (np.vdot(b, b) + 1e-10)
        out[n] = e
        mu1 = 0.999 * mu1 + 1e-8 * e ** 2
        if mu1.real > 5e-3 or (mu1.real == 5e-3 and mu1.imag > 0):
            mu1 = 5e-3
            caps += 1
    if stats is not None:
        stats["caps"] = caps
    if return_filter:
        return out, k, h
    return out
