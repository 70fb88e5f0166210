"""Times track-before-detect (target_detection.track_before_detect, prc_tbd) on one MI355X.

The published stack's shape: 1199 frames of 1024 Doppler rows x 177 range columns, reach (1, 1), alpha 0.9, the row shifts
tbd_row_shifts gives for the config-2 geometry (FM illuminator, wavelength 3 m, 0.5 s between frames, 125 m range columns,
+-256 Hz).  The statistic is prc_cfar_os at CFAR_2D's (18, 4) window, plain scale, of unit-power complex Gaussian noise
(seeded, generated on the device) with one echo per Doppler band walking its row's shift.
Recorded, in one run on one box: prc_tbd in the one-frame-per-launch form and in the time-blocked form at several frames per
launch K and band heights B, each eager (device events around the call on preallocated buffers) and as a captured graph
(events around the replay); prc_tbd_trace; and the wall clock of the tbd_maps chain next to track_maps(cfar="os",
measure="plots") on the same maps.  Median of --reps after a warm-up.  No time here is a threshold.

The DERIVED floor: one read of the statistic and one write each of score and back, 9 bytes per cell and frame, at the
6.29 TB/s copy ceiling DESIGN.md uses.  Prints one JSON line.

    python tools/tbd_bench.py [--reps 5] [--frames 1199] [--chain-frames 1199] [--commit ID] [--out profiles/tbd_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_CEILING_TBS = 6.29


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--chain-frames", type=int, default=1199)
    ap.add_argument("--commit", default=None, help="commit id to record (default: git rev-parse HEAD of this tree)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.target_detection import CFAR_2D_OS, os_cfar_threshold, tbd_maps, tbd_row_shifts, track_maps
    _lib.require_gpu()
    N, H, W, fw, gw, rank = args.frames, 1024, 177, 18, 4, 225
    ext, dt, lam = [256.0, 0.125 * (W - 1)], 0.5, 3.0
    shifts = tbd_row_shifts(H, W, ext, dt, lam)
    gen = torch.Generator(device="cuda").manual_seed(21)
    xc = torch.complex(torch.randn((N, H, W), generator=gen, device="cuda"), torch.randn((N, H, W), generator=gen, device="cuda"))
    xc = (xc * (0.5 ** 0.5)).contiguous()
    rows = [60, 200, 350, 460, 560, 700, 850, 980]                 # one echo per band of shifts, amplitude 2.5, walking its row's shift
    for k in range(N):
        for r in rows:
            xc[k, r, (20 + int(shifts[r]) * k) % (W - 40) + 20] += 2.5
    stat = CFAR_2D_OS(xc, fw, gw, rank=rank, scale="plain").contiguous()
    out = dict(tool="tbd_bench", commit=args.commit or commit_id(), reps=args.reps, frames=N, H=H, W=W, reach=[1, 1], alpha=0.9,
               row_shift_min=int(shifts.min()), row_shift_max=int(shifts.max()), shipped_frames_per_launch=_lib.TBD_FRAMES,
               data="unit-power complex Gaussian noise, seed 21, plus eight echoes of amplitude 2.5 walking their rows' shifts; "
                    "statistic: prc_cfar_os (18, 4), rank 225, plain scale")
    floor = N * H * W * 9 / (COPY_CEILING_TBS * 1e12) * 1e3
    out["floor"] = dict(derived_from=f"one read of stat, one write each of score and back ({N * H * W * 9} bytes) at {COPY_CEILING_TBS} TB/s",
                        floor_ms=round(floor, 4))

    def stats(ts):
        return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(float(np.min(ts)), 3), ms_max=round(float(np.max(ts)), 3))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return stats(ts)

    d = engine.tbd_desc(H, W, 0.9, 1, 1)
    sh = torch.from_numpy(shifts).cuda()
    score = torch.zeros((N, H, W), dtype=torch.float32, device="cuda")
    back = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    ref = None
    forms = [(1, None)] + [(K, B) for K in (2, 4, 6, 8, 12, 16, 32) for B in (None, 2, 4, 8, 16)]
    runs = []
    for K, B in forms:
        def call(stream):
            engine.tbd_execute(d, stat, sh, None, N, score, back, stream, K, B)
        r = dict(frames_per_launch=K, band_rows=B if B else "auto", launches=-(-N // K))
        r["eager"] = timed(lambda: call(_lib.torch_stream_ptr()))
        if ref is None:
            ref = (score.view(torch.int32).clone(), back.clone())
        r["same_bytes_as_first_form"] = bool(torch.equal(score.view(torch.int32), ref[0]) and torch.equal(back, ref[1]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                call(_lib.torch_stream_ptr())
        side.synchronize()
        r["graph"] = timed(g.replay)
        r["floor_share_graph"] = round(floor / r["graph"]["ms_median"], 4)
        runs.append(r)
        del g
    out["prc_tbd"] = runs
    best = min(runs, key=lambda r: r["graph"]["ms_median"])
    out["fastest_graph"] = dict(frames_per_launch=best["frames_per_launch"], band_rows=best["band_rows"], ms=best["graph"]["ms_median"])
    best = min(runs, key=lambda r: r["eager"]["ms_median"])
    out["fastest_eager"] = dict(frames_per_launch=best["frames_per_launch"], band_rows=best["band_rows"], ms=best["eager"]["ms_median"])

    # the shipped default, and 4096 ends traced 16 frames back
    out["prc_tbd_default"] = timed(lambda: engine.tbd_execute(d, stat, sh, None, N, score, back, _lib.torch_stream_ptr()))
    rng = np.random.default_rng(21)
    ends = torch.from_numpy(np.stack((rng.integers(16, N, 4096), rng.integers(0, H * W, 4096)), axis=1).astype(np.int32)).cuda()
    paths = torch.zeros((4096, 16), dtype=torch.int32, device="cuda")
    out["prc_tbd_trace_4096x16"] = timed(lambda: engine.tbd_trace(d, back, sh, N, ends, 4096, 16, paths, _lib.torch_stream_ptr()))

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 2)

    xs = xc[:args.chain_frames]
    reps = max(2, args.reps // 2)
    nt = engine.cfar_training_cells(fw, gw)
    thr = os_cfar_threshold(1e-4, nt, rank)
    # the integrated score has no closed-form threshold: calibrate on the score of this stack (its 99.99th percentile)
    sthr = float(torch.quantile(score[-1].flatten(), 0.9999))
    res = tbd_maps(xs, ext, dt, lam, thresh=sthr, depth=16, fw=fw, gw=gw, cfar="os", cfar_rank=rank)
    out["chain"] = dict(frames=int(xs.shape[0]), cfar="os", tbd_thresh=round(sthr, 4), plot_thresh=round(thr, 4),
                        tbd_plots_per_frame_mean=round(float(res[0].float().mean()), 2),
                        wall_ms_tbd_maps=wall(lambda: tbd_maps(xs, ext, dt, lam, thresh=sthr, depth=16, fw=fw, gw=gw, cfar="os",
                                                               cfar_rank=rank), reps),
                        wall_ms_track_maps_plots=wall(lambda: track_maps(xs, ext, cfar="os", cfar_rank=rank, measure="plots",
                                                                         plot_thresh=thr), reps))
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
