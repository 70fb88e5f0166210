"""Writes tests/golden/tracker_*.npz from the reference's own get_measurements and multitarget_tracker
(passiveRadar/target_detection.py:164-537).  Run where the reference checkout exists:

    python tools/gen_golden_tracker.py [--reference PATH]

* tracker_measure.npz: a dozen frames of several shapes (odd H and W, the minimum 8 x 17) and the reference's (3, M)
  candidate lists; `idx<i>` is each candidate's flat index in the reference's fliplr(frame.T) orientation, recovered
  from its coordinates.
* tracker_scene.npz: 128 frames of 96 x 48 with three moving targets (one fades out, one appears late) and the
  reference's full (Nframes, 10) history.

Frames are uint16 counts / 256 (exact in f32 and f64).  Every frame is checked to be free of ties among its candidates
and at the k / k+1 order statistics, because the reference's default argsort leaves the order of ties undefined -- except
the 8 x 17 frames, where the reference's masks zero every cell; their candidates are compared as a set (`tied<i>`).
The scene is checked to go through every status transition (0->1, 1->0, 1->2, 2->0).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")


def quantise(x):
    return np.clip(np.round(x * 256.0), 0, 65535).astype(np.uint16)


def noise_frame(rng, H, W):
    return rng.exponential(1.0, (H, W))


def blob(frame, h, w, amp):
    H, W = frame.shape
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    frame += amp * np.exp(-((hh - h) ** 2 / 1.5 + (ww - w) ** 2 / 1.0))


def tie_free(frame):
    """no ties among the candidates or at x(k) / x(k+1) of the masked, normalised frame"""
    s = np.fliplr(frame.T) / np.mean(np.abs(frame).flatten())
    s[:8, :] = 0
    s[-8:, :] = 0
    c = s.shape[1] // 2
    s[:, c - 4:c + 4] = 0
    flat = np.sort(s.ravel())
    n = flat.size
    k = int(np.floor(0.998 * (n - 1)))
    thr = np.percentile(s, 99.8)
    cand = np.sort(s.ravel()[s.ravel() >= thr])
    return bool(np.all(np.diff(cand) > 0) and (k + 1 >= n or flat[k] < flat[k + 1]))


def cand_index(cm, H, W, extent):
    rpts = np.linspace(extent[1], 0, W)
    dpts = np.linspace(-1 * extent[0], extent[0], H)
    r = np.array([int(np.nonzero(rpts == v)[0][0]) for v in cm[0]], dtype=np.int64)
    c = np.array([int(np.nonzero(dpts == v)[0][0]) for v in cm[1]], dtype=np.int64)
    return r * H + c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PASSIVERADAR_REFERENCE"), required="PASSIVERADAR_REFERENCE" not in os.environ,
                    help="checkout of the reference (Max-Manning/passiveRadar)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    np.float = float          # target_detection.py:10-17 uses aliases removed in NumPy >= 1.24
    np.int = int
    import scipy
    from passiveRadar import target_detection as ref_td

    versions = dict(numpy=np.__version__, scipy=scipy.__version__)
    rng = np.random.default_rng(20261016)

    # ---- measurement golden -------------------------------------------------------------------------------------
    shapes = [(96, 48), (97, 49), (64, 33), (65, 17), (9, 17), (8, 17), (8, 17), (128, 61), (33, 96), (101, 37),
              (256, 40), (48, 177)]
    extents = [[150.0, 120.0], [251.5, 77.25], [99.0, 300.0], [10.0, 20.0]]
    meas = {}
    for i, (H, W) in enumerate(shapes):
        extent = extents[i % len(extents)]
        while True:
            f = noise_frame(rng, H, W)
            for _ in range(2):
                blob(f, rng.uniform(0, H), rng.uniform(8, W - 8), rng.uniform(5, 30))
            f = quantise(f).astype(np.float64) / 256.0
            if H == 8 or tie_free(f):
                break
        cm = ref_td.get_measurements(f, 99.8, extent)
        meas[f"f{i}"] = quantise(f)
        meas[f"ext{i}"] = np.array(extent)
        meas[f"cand{i}"] = cm
        meas[f"idx{i}"] = cand_index(cm, H, W, extent)
        meas[f"tied{i}"] = np.array(H == 8)
    meas["nframes"] = np.array(len(shapes))
    meas["versions"] = np.array(str(versions))
    np.savez_compressed(os.path.join(OUT, "tracker_measure.npz"), **meas)

    # ---- tracker scene ------------------------------------------------------------------------------------------
    H, W, N, NT = 96, 48, 128, 10
    extent = [150.0, 150.0]            # [max Doppler (Hz), max range (km)]: about 3.1 per cell either way
    # targets: (first frame, last frame, h0, w0, dh/frame, dw/frame, amplitude)
    targets = [(0, 128, 30.0, 12.0, 0.05, 0.12, 40.0), (10, 95, 70.0, 38.0, -0.04, -0.10, 35.0),
               (50, 128, 55.0, 30.0, 0.06, 0.05, 30.0)]
    while True:
        frames = np.empty((H, W, N))
        for t in range(N):
            f = noise_frame(rng, H, W)
            for (a, b, h0, w0, dh, dw, amp) in targets:
                if a <= t < b:
                    blob(f, h0 + dh * (t - a), w0 + dw * (t - a), amp)
            frames[:, :, t] = quantise(f).astype(np.float64) / 256.0
        if all(tie_free(frames[:, :, t]) for t in range(N)):
            break
    hist = ref_td.multitarget_tracker(frames, extent, NT)
    st = hist["status"]
    trans = set()
    for t in range(1, N):
        for j in range(NT):
            trans.add((int(st[t - 1, j]), int(st[t, j])))
    for need in ((0, 1), (1, 0), (1, 2), (2, 0)):
        assert need in trans, (need, sorted(trans))
    ks = hist["kalman_state"]
    np.savez_compressed(os.path.join(OUT, "tracker_scene.npz"), frames=quantise(frames), extent=np.array(extent),
                        ntracks=np.array(NT), status=st, lifetime=hist["lifetime"], measurement=hist["measurement"],
                        estimate=hist["estimate"], history=hist["measurement_history"], x=ks["x"], P=ks["P"],
                        S=ks["S"], versions=np.array(str(versions)))
    for fn in ("tracker_measure.npz", "tracker_scene.npz"):
        print(fn, os.path.getsize(os.path.join(OUT, fn)), "bytes")
    print("transitions", sorted(trans), versions)


if __name__ == "__main__":
    main()
