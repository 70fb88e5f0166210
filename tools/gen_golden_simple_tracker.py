"""Writes tests/golden/strack_*.npz and tests/golden/persistence*.npz from the reference's own simple_target_tracker
(passiveRadar/target_detection.py:530-681) and persistence (passiveRadar/plotting_tools.py).  Run where the reference
checkout exists:

    python tools/gen_golden_simple_tracker.py [--reference PATH]

strack_<name>.npz: frames (H, W, N), the extents and the reference's history (lock_mode, measurement, measurement_idx,
estimate, x, P, S).  Frames are uint16 counts / 256 (exact in float32 and float64) in `q`, or float64 in `f64` for the
edge scenes (NaN, +-Inf, zeros, negative values).  Every frame's badness is kept at least 1e-6 away from the lock
threshold 12, so a last-bit difference cannot flip a lock decision; argmax ties are well defined and allowed.
Together the scenes cover every lock state and transition, gates that wrap to empty, wrap to a non-empty tail and clip
at the far edges, H < 250, 250 < H < 260, H > 260, W <= 16 and the edge frames.

persistence.npz: float64 and float32 stacks with an Inf, and the reference's output for a grid of (k, hold, decay).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import simple_tracker_oracle as O  # noqa: E402


def quantise(x):
    return np.clip(np.round(x * 256.0), 0, 65535).astype(np.uint16)


def noise(rng, H, W, N):
    return rng.exponential(1.0, (H, W, N))


def put(frames, i, r, c, amp=80.0):
    """a target at s-cell (range row r, Doppler column c) of frame i: storage (H-1-c, r)"""
    H = frames.shape[0]
    frames[H - 1 - c, r, i] += amp


def scene_walk(rng):
    """96 x 48: a target that appears, is tracked, jumps 25 Doppler columns for one frame (locked -> losing -> locked),
    vanishes, comes back and vanishes for good"""
    H, W, N = 96, 48, 90
    ext = (120.0, 150.0)
    f = noise(rng, H, W, N)
    r, c = 30.0, 60.0
    for i in range(N):
        visible = (5 <= i < 30) or (34 <= i < 36) or (40 <= i < 60) or (62 <= i < 63) or (70 <= i < 80)
        r += rng.normal(0, 0.3)
        c += rng.normal(0, 0.5)
        r = min(max(r, 12), W - 12)
        c = min(max(c, 10), H - 10)
        if visible:
            put(f, i, int(round(r)), int(round(c)) + (25 if i == 50 else 0))
    return "walk", f, ext


def scene_wrap_empty(rng):
    """W = 48: a target locked at range row 20, the gate's rows s[-4:44] wrap to s[44:44]: empty, (0, 0)"""
    H, W, N = 80, 48, 30
    ext = (100.0, 100.0)
    f = noise(rng, H, W, N)
    for i in range(N):
        put(f, i, 20 if i < 12 else 10, 40)
    return "wrap_empty", f, ext


def scene_wrap_tail(rng):
    """H = 80: a target locked at Doppler column 10, the gate's columns s[:, -38:58] wrap to s[:, 42:58], a non-empty
    tail far from the target, where a second target is"""
    H, W, N = 80, 40, 30
    ext = (100.0, 100.0)
    f = noise(rng, H, W, N)
    for i in range(N):
        put(f, i, 20, 10)
        put(f, i, 22, 50, 40.0)
    return "wrap_tail", f, ext


def scene_far_edge(rng):
    """a target near the far range and Doppler edges: the gate clips at W and H"""
    H, W, N = 64, 40, 30
    ext = (100.0, 100.0)
    f = noise(rng, H, W, N)
    for i in range(N):
        put(f, i, W - 10, H - 3)
    return "far_edge", f, ext


def scene_h(rng, H, name):
    H, W, N = H, 24, 24
    ext = (60.0, 300.0)
    f = noise(rng, H, W, N)
    for i in range(N):
        put(f, i, 12, 255 if i % 3 else min(H - 5, 262))
        put(f, i, 11, 240, 30.0)
    return name, f, ext


def scene_narrow(rng):
    """W = 16: every row masked"""
    H, W, N = 40, 16, 8
    f = noise(rng, H, W, N)
    put(f, 2, 8, 20)
    return "w16", f, (50.0, 50.0)


def scene_edges(rng):
    """float64 edge frames between ordinary ones: NaN, +Inf, -Inf, all zeros, all negative, mixed signs"""
    H, W, N = 48, 40, 24
    ext = (100.0, 100.0)
    f = np.round(noise(rng, H, W, N) * 256) / 256
    for i in range(N):
        put(f, i, 20, 30)
    f[5, 22, 3] = np.nan
    f[30, 3, 5] = np.inf                 # masked cell: the mean is Inf, no NaN survives, (0, 0)
    f[10, 25, 7] = np.inf
    f[12, 24, 7] = -np.inf
    f[7, 12, 9] = -np.inf
    f[:, :, 11] = 0.0
    f[:, :, 13] = -f[:, :, 13]
    f[:, :, 15] = f[:, :, 15] - 1.5
    f[40, 1, 17] = np.nan                # NaN in a masked cell still makes the mean NaN
    return "edges", f, ext


def run_reference(ref_td, frames, ext):
    h = ref_td.simple_target_tracker(frames, ext[0], ext[1])
    ks = h["kalman_state"]
    return dict(lock_mode=h["lock_mode"], measurement=h["measurement"], measurement_idx=h["measurement_idx"],
                estimate=h["estimate"], x=ks["x"], P=ks["P"].reshape(-1, 16), S=ks["S"].reshape(-1, 4))


def transitions(lock):
    st = np.argmax(lock, axis=1)
    prev = np.concatenate(([0], st[:-1]))
    return {(int(a), int(b)) for a, b in zip(prev, st)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PASSIVERADAR_REFERENCE"),
                    required="PASSIVERADAR_REFERENCE" not in os.environ,
                    help="checkout of the reference (Max-Manning/passiveRadar)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    np.float = float          # target_detection.py:530-537 uses aliases removed in NumPy >= 1.24
    np.int = int
    from passiveRadar import target_detection as ref_td
    from passiveRadar import plotting_tools as ref_pt

    rng = np.random.default_rng(20261016)
    scenes = [scene_walk(rng), scene_wrap_empty(rng), scene_wrap_tail(rng), scene_far_edge(rng),
              scene_h(rng, 200, "h200"), scene_h(rng, 255, "h255"), scene_h(rng, 300, "h300"), scene_narrow(rng),
              scene_edges(rng)]
    seen = set()
    for name, frames, ext in scenes:
        edge = name == "edges"
        if not edge:
            q = quantise(frames)
            frames = q.astype(np.float64) / 256.0
        with np.errstate(all="ignore"):
            g = run_reference(ref_td, frames.copy(), ext)
            o = O.simple_target_tracker(frames, ext[0], ext[1])
        bad = np.abs(o["badness"] - 12.0)
        assert bad.min() > 1e-6, (name, bad.min())
        for k in ("lock_mode", "measurement", "measurement_idx"):
            assert np.array_equal(o[k], g[k]), (name, k)
        seen |= transitions(g["lock_mode"])
        payload = dict(ext=np.array(ext), **g)
        payload["f64" if edge else "q"] = frames if edge else q
        fn = os.path.join(OUT, f"strack_{name}.npz")
        np.savez_compressed(fn, **payload)
        print(name, frames.shape, sorted(transitions(g["lock_mode"])), os.path.getsize(fn))
    want = {(0, 0), (0, 1), (1, 0), (1, 2), (2, 2), (2, 3), (3, 0), (3, 2)}
    assert want <= seen, want - seen

    # ---- persistence ------------------------------------------------------------------------------------------------
    H, W, L = 9, 7, 12
    x64 = quantise(rng.exponential(1.0, (H, W, L))).astype(np.float64) / 256.0
    x64[3, 4, 5] = np.inf
    x32 = x64.astype(np.float32)
    x32[2, 2, 7] = -np.inf
    cases, outs = [], []
    for hold in (0, 1, 20, 3, 12, 50):
        for decay in (0.9, 0.0, 1.0, -0.5, 1e-200):
            for k in (-1, 0, 6, L - 1):
                for which, X in ((0, x64), (1, x32)):
                    with np.errstate(all="ignore"):
                        out = ref_pt.persistence(X, k, hold, decay)
                    cases.append((which, k, hold, decay))
                    outs.append(out)
    fn = os.path.join(OUT, "persistence.npz")
    np.savez_compressed(fn, x64=x64, x32=x32, cases=np.array(cases, dtype=np.float64), out=np.array(outs))
    print("persistence", len(cases), os.path.getsize(fn))


if __name__ == "__main__":
    main()
