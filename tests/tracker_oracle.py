"""NumPy restatement of the reference's measurement extraction and multi-target Kalman tracker
(passiveRadar/target_detection.py:164-537), for tests only.

It states the rules the device kernels of passiveradar_amd/csrc/track.hip follow, in plain NumPy:

* get_measurements (:164-229): mean |v| of the whole frame, the ``fliplr(frame.T)`` orientation, the range-row and
  Doppler-column masks, numpy's ``linear`` percentile (k / t / ``_lerp`` as numpy 2.x computes them), candidates
  ``v/mean >= thr`` sorted by descending strength with ties broken by descending flat index in the ``fliplr(T)``
  row-major order (``np.flip(np.argsort(s, kind="stable"))``), and coordinates from numpy 2.x's linspace formula.
* the tracker (:231-537) with every quirk of the reference kept (see ``associate`` and ``update``); candidates are
  masked, never compacted, so "the first remaining candidate" keeps the reference's meaning.

A frame whose mean is not finite and positive (a NaN or Inf in it, or all zeros) yields no candidates.
"""
from __future__ import annotations

import math

import numpy as np

PERCENTILE = 99.8
F1 = np.array([[1, 0, -0.003, 0], [0, 0, -0.003, -0.003], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
F2 = np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
Q = np.diag([4.0, 0.03, 0.2, 0.08])
HM = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
R = np.diag([5.0, 2.0])
P0 = np.diag([5.0, 0.0225, 0.04, 0.1])
S0 = np.diag([1.0, 1.0])
HIST0 = np.array([1, 0, 0, 0, 0, 1, 1, 1, 1, 1] + [0] * 10, dtype=np.float64)


# ---- host helpers ---------------------------------------------------------------------------------------------------
def percentile_kt(n, p=PERCENTILE):
    """(k, t) of numpy's ``linear`` percentile of n values: q = p/100, vi = q (n-1), k = floor(vi), t = vi - k; above
    the last index numpy takes both order statistics at n-1 (t = 0)."""
    q = np.true_divide(np.float64(p), 100)
    vi = np.float64(n - 1) * q
    k = int(math.floor(vi))
    t = float(vi - np.float64(k))
    if vi >= n - 1:
        k, t = n - 1, 0.0
    return k, t


def lerp(a, b, t):
    """numpy's _lerp, including its t >= 0.5 branch"""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    d = b - a
    if t >= 0.5:
        return float(b - d * (np.float64(1.0) - t))
    return float(a + d * t)


def percentile(x, p=PERCENTILE):
    """np.percentile(x, p) (linear) from the exact order statistics x(k), x(k+1)"""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = x.size
    k, t = percentile_kt(n, p)
    k1 = min(k + 1, n - 1)
    part = np.partition(x, [k, k1])
    return lerp(part[k], part[k1], t)


def linspace(start, stop, num):
    """numpy 2.x linspace: i*step + start (two roundings), the last point set to stop"""
    start, stop = np.float64(start), np.float64(stop)
    step = (stop - start) / np.float64(num - 1)
    y = np.arange(num, dtype=np.float64) * step + start
    y[-1] = stop
    return y


# ---- get_measurements -----------------------------------------------------------------------------------------------
def measure(frame, frame_extent, p=PERCENTILE):
    """Candidates of one frame [H][W] (H = Doppler rows, W = range columns): dict with range, doppler, strength (f64,
    sorted) and idx (flat index in the fliplr(T) orientation, int64), plus count and thr."""
    f = np.asarray(frame)
    Hh, Ww = f.shape
    mean = np.float64(np.abs(f.astype(np.float64)).sum(dtype=np.float64)) / np.float64(f.size)
    empty = dict(range=np.zeros(0), doppler=np.zeros(0), strength=np.zeros(0), idx=np.zeros(0, np.int64), count=0,
                 thr=np.nan, mean=mean)
    if not (np.isfinite(mean) and mean > 0):
        return empty
    s = np.fliplr(f.astype(np.float64).T) / mean               # [W][H]: rows range, columns reversed Doppler
    s[:8, :] = 0
    s[-8:, :] = 0
    c = Hh // 2
    s[:, c - 4:c + 4] = 0
    thr = percentile(s, p)
    flat = s.ravel()
    sel = np.nonzero(flat >= thr)[0]
    order = np.flip(np.argsort(flat[sel], kind="stable"))
    idx = sel[order].astype(np.int64)
    rpts = linspace(frame_extent[1], 0, Ww)
    dpts = linspace(-1 * frame_extent[0], frame_extent[0], Hh)
    return dict(range=rpts[idx // Hh], doppler=dpts[idx % Hh], strength=flat[idx], idx=idx, count=int(idx.size),
                thr=thr, mean=mean)


def get_measurements(frame, p, frame_extent):
    """(3, M) like the reference: range, Doppler, strength.  ``p`` is ignored as in the tracker (always 99.8) -- but this
    restatement honours it for the edge tests of the C ABI."""
    m = measure(frame, frame_extent, p)
    return np.stack((m["range"], m["doppler"], m["strength"]))


# ---- tracker --------------------------------------------------------------------------------------------------------
def new_track(meas=None):
    """initialize_track (:333-387); the reference's swapped estimate / measurement tuple order is harmless: both [r, f]"""
    r, f = (0.0, 0.0) if meas is None else (float(meas[0]), float(meas[1]))
    x = np.array([r, 0.0, f, -1.0])
    return dict(status=0 if meas is None else 1, lifetime=1, measurement=np.array([r, f]), estimate=np.array([r, f]),
                hist=HIST0.copy(), x=x, P=P0.copy(), S=S0.copy())


def inv2(S):
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    return np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]]) / det


def associate(tr, rng, dop, alive):
    """associate_measurements (:231-331) on masked candidates; returns the measurement or None and updates `alive`.
    Quirks kept on purpose: the free track takes the overall strongest candidate and removes |dr| < 10, |dd| < 12 around
    it; the preliminary track takes argmin sqrt(r^2 + d^2) (absolute norm, first occurrence); the confirmed track gates
    early on the last ESTIMATE (4 km, 20 Hz), validates with the last MEASUREMENT and the stored S (< 6), takes the
    strongest validated candidate, removes ~earlyGate, and leaves the list unchanged if nothing validates."""
    st = tr["status"]
    if st == 0:
        gate = alive.copy()
    elif st == 1:
        gate = alive & (np.abs(rng - tr["measurement"][0]) < 5) & (np.abs(dop - tr["measurement"][1]) < 24)
    else:
        gate = alive & (np.abs(rng - tr["estimate"][0]) < 4) & (np.abs(dop - tr["estimate"][1]) < 20)
    cand = np.nonzero(gate)[0]
    if st == 2:
        Si = inv2(tr["S"])
        ok = []
        for j in cand:
            z = np.array([tr["measurement"][0] - rng[j], tr["measurement"][1] - dop[j]])
            ok.append(z @ Si @ z < 6)
        cand = cand[np.array(ok, dtype=bool)] if cand.size else cand
    if cand.size == 0:
        return None
    if st == 0:
        j = cand[0]
        if cand.size > 1:
            gate = alive & (np.abs(rng - rng[j]) < 10) & (np.abs(dop - dop[j]) < 12)
    elif st == 1:
        j = cand[int(np.argmin(np.sqrt(rng[cand] ** 2 + dop[cand] ** 2)))]
    else:
        j = cand[0]
    alive &= ~gate
    return np.array([rng[j], dop[j]])


def update(tr, meas):
    """update_track (:389-453): kill / promote read the history from BEFORE its shift (intentional, as the reference);
    the adaptive update scales R by |z - z_prev|^2; without a measurement the track extrapolates and keeps its last one."""
    x, P = tr["x"], tr["P"]
    x = F1 @ x
    P = F2 @ P @ F2.T + Q
    hist = tr["hist"]
    if meas is None:
        S = HM @ P @ HM.T + R
        new_meas = tr["measurement"]
        new_hist = np.concatenate(([0.0], hist[:-1]))
    else:
        dm = meas - tr["measurement"]
        S = HM @ P @ HM.T + R * (dm[0] ** 2 + dm[1] ** 2)
        K = P @ HM.T @ inv2(S)
        x = x + K @ (meas - HM @ x)
        P = (np.eye(4) - K @ HM) @ P
        new_meas = meas
        new_hist = np.concatenate(([1.0], hist[:-1]))
    st, life = tr["status"], tr["lifetime"]
    if st == 1:
        if life > 4 and hist[0:10].sum() < 6:
            st = 0
        if life > 4 and hist[0:10].sum() > 8:
            st = 2
    elif st == 2:
        if life > 4 and hist.sum() < 4:
            st = 0
    return dict(status=st, lifetime=life + 1, measurement=np.array(new_meas, dtype=np.float64), estimate=HM @ x,
                hist=new_hist, x=x, P=P, S=S)


def track(cands, ntracks):
    """multitarget_tracker (:455-537) over per-frame candidate lists [(range, doppler), ...] in strength order; returns
    a list (frames) of lists (tracks) of state dicts.  When the candidates run out the loop over free tracks breaks: the
    free tracks left are not touched and do not age."""
    tracks = [new_track() for _ in range(ntracks)]
    out = []
    for rng, dop in cands:
        rng = np.asarray(rng, np.float64)
        dop = np.asarray(dop, np.float64)
        alive = np.ones(rng.size, dtype=bool)
        st = [t["status"] for t in tracks]
        order = ([i for i in range(ntracks) if st[i] == 2] + [i for i in range(ntracks) if st[i] == 1])
        for i in order:
            tracks[i] = update(tracks[i], associate(tracks[i], rng, dop, alive))
        for i in (i for i in range(ntracks) if st[i] == 0):
            if not alive.any():
                break
            tracks[i] = new_track(associate(tracks[i], rng, dop, alive))
        out.append([dict(t) for t in tracks])
    return out


def multitarget_tracker(data, frame_extent, ntracks):
    """the restated tracker on numpy (H, W, Nframes) frames, as the reference is called"""
    cands = []
    for i in range(data.shape[2]):
        m = measure(data[:, :, i], frame_extent)
        cands.append((m["range"], m["doppler"]))
    return track(cands, ntracks)


def history_arrays(hist):
    """state dicts -> dict of stacked arrays [frames][tracks](...)"""
    keys = ("status", "lifetime", "measurement", "estimate", "hist", "x", "P", "S")
    return {k: np.array([[t[k] for t in row] for row in hist]) for k in keys}
