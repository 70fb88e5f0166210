"""NumPy restatement of the reference's LS_Filter_SVD (passiveRadar/clutter_removal.py:58-107) in float64, with the cut rule
of the drop-in (passiveradar_amd/csrc/ls_svd.hip, include/prcore.h):

    A[:, k] = roll(ref, k - peek)           k = 0 .. T-1, T = filterLen + peek         (complex128, N x T)
    U, S, VH = svd(A)
    keep_i  = not (S_i < max(1e-10, rcond * S_0))
    h = V diag(keep / S) U^H srv;   out = srv - A h

``rcond=None`` is the drop-in's default 4 sqrt(T) 2^-26; ``rcond=0`` is the reference's absolute rule alone (it drops what
lies below 1e-10 and nothing else).  The inputs are taken as they are (complex64 data promoted to complex128, so the
problem solved is the one the complex64 data poses); nothing is rounded on the way out."""
import numpy as np


def default_rcond(T):
    return 4.0 * np.sqrt(float(T)) * 2.0 ** -26


def data_matrix(ref, filterLen, peek):
    r = np.asarray(ref).astype(np.complex128)
    return np.stack([np.roll(r, k) for k in range(-int(peek), int(filterLen))], axis=1)


def ls_filter_svd(ref, srv, filterLen, peek=10, rcond=None, info=None):
    """returns (out, taps) in complex128; ``info``: a dict that receives the singular values ("sv", descending), the number
    of directions kept ("kept") and the cut ("cut")"""
    ref = np.asarray(ref)
    srv = np.asarray(srv)
    if ref.shape != srv.shape:
        raise ValueError("Input vectors must have the same length")
    T = int(filterLen) + int(peek)
    rc = default_rcond(T) if rcond is None else float(rcond)
    A = data_matrix(ref, filterLen, peek)
    s = srv.astype(np.complex128)
    U, S, VH = np.linalg.svd(A, full_matrices=False)
    cut = max(1e-10, rc * (S[0] if S.size else 0.0))
    keep = ~(S < cut)
    inv = np.zeros_like(S)
    inv[keep] = 1.0 / S[keep]
    h = VH.conj().T @ (inv * (U.conj().T @ s))
    if info is not None:
        info["sv"], info["kept"], info["cut"] = S, int(keep.sum()), cut
    return s - A @ h, h
