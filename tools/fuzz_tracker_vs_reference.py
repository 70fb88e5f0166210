"""Compares the NumPy restatement of the tracker (tests/tracker_oracle.py) with the reference's own get_measurements
and multitarget_tracker on random tie-free scenes.  Run where the reference checkout exists:

    python tools/fuzz_tracker_vs_reference.py [--scenes 20] [--reference PATH]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--reference", default=os.environ.get("PASSIVERADAR_REFERENCE"), required="PASSIVERADAR_REFERENCE" not in os.environ,
                    help="checkout of the reference (Max-Manning/passiveRadar)")
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    np.float = float          # target_detection.py:10-17 uses aliases removed in NumPy >= 1.24
    np.int = int
    from passiveRadar import target_detection as ref_td
    import tracker_oracle as T
    from gen_golden_tracker import blob, noise_frame, quantise, tie_free

    rng = np.random.default_rng(77)
    worst, done = 0.0, 0
    for s in range(args.scenes):
        H, W, N = int(rng.integers(24, 97)), int(rng.integers(17, 61)), int(rng.integers(20, 60))
        ext = [float(rng.uniform(5, 300)), float(rng.uniform(5, 300))]
        tg = [(rng.uniform(0, H), rng.uniform(8, W - 8), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2),
               rng.uniform(10, 40)) for _ in range(int(rng.integers(1, 4)))]
        frames = np.empty((H, W, N))
        for t in range(N):
            f = noise_frame(rng, H, W)
            for h0, w0, dh, dw, a in tg:
                blob(f, h0 + dh * t, w0 + dw * t, a)
            frames[:, :, t] = quantise(f).astype(np.float64) / 256.0
        if not all(tie_free(frames[:, :, t]) for t in range(N)):
            continue
        for t in range(N):
            a = ref_td.get_measurements(frames[:, :, t], 99.8, ext)
            b = T.get_measurements(frames[:, :, t], 99.8, ext)
            assert np.array_equal(a[:2], b[:2]), (s, t)
            assert np.allclose(a[2], b[2], rtol=1e-12, atol=0), (s, t)
        ref = ref_td.multitarget_tracker(frames, ext, 10)
        h = T.history_arrays(T.multitarget_tracker(frames, ext, 10))
        assert np.array_equal(ref["status"], h["status"]), s
        assert np.array_equal(ref["lifetime"], h["lifetime"]), s
        assert np.array_equal(ref["measurement_history"], h["hist"]), s
        err = max(float(np.abs(ref["kalman_state"]["x"] - h["x"]).max()),
                  float(np.abs(ref["kalman_state"]["P"] - h["P"]).max()),
                  float(np.abs(ref["estimate"] - h["estimate"]).max()))
        worst = max(worst, err)
        done += 1
        print(f"scene {s}: {H} x {W} x {N} frames, {len(tg)} targets: candidates exact, states max abs diff {err:.2e}")
    print(f"{done} scenes agree; worst state difference {worst:.2e}")


if __name__ == "__main__":
    main()
