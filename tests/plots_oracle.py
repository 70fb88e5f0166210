"""NumPy / plain-Python statement of plot extraction (prc_plots of include/prcore.h), for tests only.

Detection: storage cell i = h W + w of a frame [H][W] (H Doppler rows, W range columns) detects iff stat[i] > thresh in
float32 (NaN never, +Inf does) and it lies outside get_measurements' excluded zones with their widths as parameters:
w < range_guard or w >= W - range_guard; Doppler column c = H-1-h inside [H/2 - doppler_guard, H/2 + doppler_guard).
A plot is a connected component of detecting cells (4- or 8-connectivity, no wrap), found here by flood fill.
Per plot, members in ascending storage index and g = the cell's float32 weight as float64: mass = sum g, hbar = (sum g h) /
mass, wbar = (sum g w) / mass -- explicit loops, one rounding per add and per divide (np.sum would sum pairwise); a mass
that is not finite or not > 0 puts the centroid on the peak cell.  The peak is the member of largest stat, ties to the
smallest storage index; strength = that stat, index = w_p H + (H-1-h_p).  range = wbar ((0 - R) / (W-1)) + R, doppler =
((H-1) - hbar) (2 D / (H-1)) + (-D).  A frame's plots come in descending strength, ties by descending index.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("range", "doppler", "strength", "index", "mass", "hbar", "wbar", "ncells", "h0", "h1", "w0", "w1", "peak")


def detections(stat, thresh, range_guard=8, doppler_guard=4):
    """bool [H][W]"""
    s = np.asarray(stat, dtype=np.float32)
    H, W = s.shape
    with np.errstate(invalid="ignore"):
        det = s > np.float32(thresh)
    w = np.arange(W)
    c = H - 1 - np.arange(H)
    det[:, (w < range_guard) | (w >= W - range_guard)] = False
    det[(c >= H // 2 - doppler_guard) & (c < H // 2 + doppler_guard), :] = False
    return det


def label(mask, connectivity=8):
    """int32 [H][W]: 0 outside the mask, else 1 + the rank of the component among the components ordered by their smallest
    storage index (flood fill with an explicit stack)"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8")
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    lab = np.zeros((H, W), np.int32)
    nxt = 0
    for h0 in range(H):
        for w0 in range(W):
            if not mask[h0, w0] or lab[h0, w0]:
                continue
            nxt += 1
            lab[h0, w0] = nxt
            stack = [(h0, w0)]
            while stack:
                h, w = stack.pop()
                for dh, dw in steps:
                    y, x = h + dh, w + dw
                    if 0 <= y < H and 0 <= x < W and mask[y, x] and not lab[y, x]:
                        lab[y, x] = nxt
                        stack.append((y, x))
    return lab


def weights_f32(stat, weight):
    """the float32 weight of every cell: stat itself, a float32 map, or |complex64| = hypotf, taken as the header states it:
    through float64 -- exact squares, a rounded sum, a rounded root -- then rounded to float32.  (np.abs of complex64 is
    not used: its vectorised loop is float32 arithmetic and lands one or two ulps away on a third of Gaussian values.)"""
    if weight is None:
        return np.asarray(stat, dtype=np.float32)
    w = np.asarray(weight)
    if np.iscomplexobj(w):
        w = w.astype(np.complex64)
        re, im = w.real.astype(np.float64), w.imag.astype(np.float64)
        with np.errstate(all="ignore"):
            return np.sqrt(re * re + im * im).astype(np.float32)
    return w.astype(np.float32)


def key_of(v):
    """the order-preserving integer key of a float32 (-0 taken as +0)"""
    b = int(np.float32(v).view(np.uint32))
    if b == 0x80000000:
        b = 0
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


def plots(stat, thresh, frame_extent, weight=None, connectivity=8, range_guard=8, doppler_guard=4):
    """one frame -> dict: ``ncells_total`` (detecting cells), ``count`` (plots) and one array per name of FIELDS, in output order"""
    s = np.asarray(stat, dtype=np.float32)
    H, W = s.shape
    g32 = weights_f32(s, weight)
    det = detections(s, thresh, range_guard, doppler_guard)
    lab = label(det, connectivity)
    D, R = np.float64(frame_extent[0]), np.float64(frame_extent[1])
    rstep = (np.float64(0.0) - R) / np.float64(W - 1)
    dstep = (np.float64(2.0) * D) / np.float64(H - 1)
    flat_lab, flat_s, flat_g = lab.ravel(), s.ravel(), g32.ravel()
    members = {}
    for i in np.nonzero(flat_lab)[0]:                      # ascending storage index
        members.setdefault(int(flat_lab[i]), []).append(int(i))
    rows = []
    with np.errstate(all="ignore"):
        for cells in members.values():
            M = sh = sw = np.float64(0.0)
            peak = cells[0]
            for i in cells:
                h, w = divmod(i, W)
                g = np.float64(flat_g[i])
                M = M + g
                sh = sh + g * np.float64(h)
                sw = sw + g * np.float64(w)
                if key_of(flat_s[i]) > key_of(flat_s[peak]):
                    peak = i
            hp, wp = divmod(peak, W)
            if np.isfinite(M) and M > 0:
                hbar, wbar = sh / M, sw / M
            else:
                hbar, wbar = np.float64(hp), np.float64(wp)
            hs = [i // W for i in cells]
            ws = [i % W for i in cells]
            rows.append(dict(range=wbar * rstep + R, doppler=(np.float64(H - 1) - hbar) * dstep + (-D),
                             strength=np.float64(flat_s[peak]), index=wp * H + (H - 1 - hp), mass=M, hbar=hbar, wbar=wbar,
                             ncells=len(cells), h0=min(hs), h1=max(hs), w0=min(ws), w1=max(ws), peak=peak,
                             key=(key_of(flat_s[peak]) << 32) | (wp * H + (H - 1 - hp))))
    rows.sort(key=lambda r: r["key"], reverse=True)
    out = {k: np.array([r[k] for r in rows], dtype=np.float64 if k in ("range", "doppler", "strength", "mass", "hbar", "wbar")
                       else np.int64) for k in FIELDS}
    out["count"] = len(rows)
    out["ncells_total"] = int(det.sum())
    out["labels"] = lab
    return out
