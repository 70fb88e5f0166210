"""The definition of prc_tbd / prc_tbd_trace (include/prcore.h) in NumPy: every product and every sum an explicit float32
operation, the predecessors visited in ascending code order with a strict float32 '>' (NaN and -Inf are never chosen, ties
go to the smallest code)."""
import numpy as np

NONE = 255


def excluded(H, W, range_guard=8, doppler_guard=4):
    """prc_plots' two masks as bool [H, W]"""
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    c = H - 1 - h
    return (w < range_guard) | (w >= W - range_guard) | ((c >= H // 2 - doppler_guard) & (c < H // 2 + doppler_guard))


def inputs(stat, clip=np.inf, range_guard=8, doppler_guard=4):
    """z' of a frame or a stack [..., H, W]"""
    z = np.asarray(stat, dtype=np.float32)
    H, W = z.shape[-2:]
    c = np.float32(clip)
    with np.errstate(invalid="ignore"):
        zp = np.where(z > c, c, z)                       # a NaN stays
    return np.where(excluded(H, W, range_guard, doppler_guard), np.float32(0.0), zp).astype(np.float32)


def predecessors(H, W, qd, qr, row_shift=None):
    """per code, (h', w', valid) as [H, W] arrays: Python integers of any size underneath, so nothing overflows"""
    s = np.zeros(H, dtype=np.int64) if row_shift is None else np.asarray(row_shift, dtype=np.int64)
    h, w = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    out = []
    for dh in range(-qd, qd + 1):
        hp = h + dh
        ok_h = (hp >= 0) & (hp < H)
        hc = np.clip(hp, 0, H - 1)
        for dw in range(-qr, qr + 1):
            wp = w - s[hc] + dw                          # |.| < 2^31 + W + qr: exact in int64
            ok = ok_h & (wp >= 0) & (wp < W)
            out.append((np.broadcast_to(hc, (H, W)), np.clip(wp, 0, W - 1), ok))
    return out


def tbd(stat, qd=1, qr=1, alpha=0.9, clip=np.inf, range_guard=8, doppler_guard=4, row_shift=None, prev=None):
    """(score float32 [N, H, W], back uint8 [N, H, W]) of a stack [N, H, W]"""
    z = inputs(stat, clip, range_guard, doppler_guard)
    N, H, W = z.shape
    a = np.float32(alpha)
    pred = predecessors(H, W, qd, qr, row_shift)
    assert len(pred) <= 255
    score, back = np.empty((N, H, W), np.float32), np.empty((N, H, W), np.uint8)
    last = None if prev is None else np.asarray(prev, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(N):
            code = np.full((H, W), NONE, np.uint8)
            best = np.full((H, W), -np.inf, np.float32)
            if last is not None:
                for c, (hp, wp, ok) in enumerate(pred):
                    v = last[hp, wp]
                    take = ok & (v > best)
                    best = np.where(take, v, best)
                    code = np.where(take, np.uint8(c), code)
            m = np.where(code == NONE, np.float32(0.0), best).astype(np.float32)
            prod = (a * m).astype(np.float32)            # rounded once ...
            last = (z[k] + prod).astype(np.float32)      # ... and once more: never a fused multiply-add
            score[k], back[k] = last, code
    return score, back


def trace(back, ends, depth, qd=1, qr=1, row_shift=None):
    """paths int32 [nends, depth] (prc_tbd_trace)"""
    back = np.asarray(back)
    N, H, W = back.shape
    s = np.zeros(H, dtype=np.int64) if row_shift is None else np.asarray(row_shift, dtype=np.int64)
    nr, ncodes = 2 * qr + 1, (2 * qd + 1) * (2 * qr + 1)
    ends = np.asarray(ends).reshape(-1, 2)
    paths = np.full((ends.shape[0], depth), -1, np.int32)
    for e, (f, cell) in enumerate(ends.tolist()):
        if not (0 <= f < N and 0 <= cell < H * W):
            continue
        paths[e, 0] = cell
        for j in range(1, depth):
            if f - j < 0:
                break
            code = int(back[f - j + 1].ravel()[cell])
            if code >= ncodes:
                break
            h, w = divmod(cell, W)
            hp = h + code // nr - qd
            if not 0 <= hp < H:
                break
            wp = w - int(s[hp]) + code % nr - qr
            if not 0 <= wp < W:
                break
            cell = hp * W + wp
            paths[e, j] = cell
    return paths


def same_bits(got, want):
    """bit identity of two float32 arrays; where BOTH are NaN only that is compared (IEEE 754 leaves the sign and payload of
    a NaN an operation produces open, and processors differ in it)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    both = np.isnan(got) & np.isnan(want)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | both))


def planted_scene(seed, with_target=True, nframes=20, H=64, W=96, amp=2.5, row=20, col0=10, step=2):
    """|unit complex Gaussian| [nframes, H, W] with one target of amplitude ``amp`` added to the complex cell
    (row, col0 + step k) of frame k; the same seed without the target is the same noise"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((nframes, H, W)) + 1j * rng.standard_normal((nframes, H, W))) * np.sqrt(0.5)
    if with_target:
        for k in range(nframes):
            x[k, row, col0 + step * k] += amp
    return np.abs(x).astype(np.float32)
