"""Times plot extraction (target_detection.extract_plots, prc_plots) on one MI355X.

The published stack's shape: 1199 frames of 1024 Doppler rows x 177 range columns.  Unit-power complex Gaussian noise
(Rayleigh magnitudes; seeded, generated on the device) plus ten 3 x 3 targets 12 exp(-0.35 d^2) per frame at seeded
places outside the excluded zones.  The statistic is prc_cfar_os at CFAR_2D's (18, 4) window, rank 225 of 299, plain scale;
the thresholds are os_cfar_threshold's multipliers for Pfa 1e-3 and 1e-4; the weights are the complex maps themselves.
Recorded, in one run on one box: prc_plots at both thresholds with and without the info records (device events around the
call on preallocated buffers: the kernel alone; also with max_cells = 1024, a quarter of the LDS), the detections and
plots it found, prc_track_measure on the same statistic, and the track_maps chain (wall clock, device tensor in, records
out) under both values of ``measure``.  No time here is a threshold.

The DERIVED floor: the kernel has to read the statistic once -- frames x H x W x 4 bytes at the 6.29 TB/s copy ceiling
DESIGN.md uses; the lists it sorts and the records it writes are three orders of magnitude smaller.  Prints one JSON line.

    python tools/plots_bench.py [--reps 5] [--frames 1199] [--chain-frames 1199] [--out profiles/plots_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_CEILING_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--chain-frames", type=int, default=1199)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.target_detection import CFAR_2D_OS, TrackPlan, os_cfar_threshold, track_maps
    _lib.require_gpu()
    N, H, W, fw, gw, rank, ntargets = args.frames, 1024, 177, 18, 4, 225, 10
    ext = [256.0, 177.0]
    gen = torch.Generator(device="cuda").manual_seed(20)
    xc = torch.complex(torch.randn((N, H, W), generator=gen, device="cuda"), torch.randn((N, H, W), generator=gen, device="cuda"))
    xc = (xc * (0.5 ** 0.5)).contiguous()
    rng = np.random.default_rng(20)
    rows = np.concatenate((np.arange(2, H // 2 - 6), np.arange(H // 2 + 6, H - 2)))      # clear of the Doppler zone
    th = torch.from_numpy(rng.choice(rows, (N, ntargets))).cuda()
    tw = torch.from_numpy(rng.integers(10, W - 10, (N, ntargets))).cuda()
    fidx = torch.arange(N, device="cuda")[:, None].expand(N, ntargets)
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            amp = float(12.0 * np.exp(-0.35 * (dh * dh + dw * dw)))
            xc.index_put_((fidx, th + dh, tw + dw), torch.full((N, ntargets), amp, dtype=torch.complex64, device="cuda"), accumulate=True)
    stat = CFAR_2D_OS(xc, fw, gw, rank=rank, scale="plain").contiguous()
    nt = engine.cfar_training_cells(fw, gw)
    out = dict(tool="plots_bench", reps=args.reps, frames=N, H=H, W=W, fw=fw, gw=gw, rank=rank, training_cells=nt,
               data="unit-power complex Gaussian noise plus ten 3 x 3 targets 12 exp(-0.35 d^2) per frame, seed 20; "
                    "statistic: prc_cfar_os, plain scale; weights: the complex maps")

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
        return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(float(np.min(ts)), 3), ms_max=round(float(np.max(ts)), 3))

    stream = _lib.torch_stream_ptr()
    cap = 1024
    counts = torch.zeros(N, dtype=torch.int32, device="cuda")
    ncells = torch.zeros(N, dtype=torch.int32, device="cuda")
    cands = torch.zeros(N * cap * 32, dtype=torch.uint8, device="cuda")
    info = torch.zeros(N * cap * 48, dtype=torch.uint8, device="cuda")
    floor = N * H * W * 4 / (COPY_CEILING_TBS * 1e12) * 1e3
    out["floor"] = dict(derived_from=f"one read of the float32 statistic ({N * H * W * 4} bytes) at {COPY_CEILING_TBS} TB/s",
                        floor_ms=round(floor, 4))
    for pfa in (1e-3, 1e-4):
        thr = os_cfar_threshold(pfa, nt, rank)
        d = engine.plots_desc(H, W, thr, ext, capacity=cap, complex_weight=True)
        for with_info in (False, True):
            r = timed(lambda: engine.plots_execute(d, stat, xc, N, counts, ncells, cands, info if with_info else None, None, stream))
            r["floor_share"] = round(floor / r["ms_median"], 4)
            out[f"prc_plots_pfa{pfa:g}" + ("_info" if with_info else "")] = r
        # max_cells is also the LDS a workgroup asks for (20 bytes per cell, rounded up to a power of two): 1024 cells = 20 KiB
        # lets several workgroups share a CU where the default 4096 = 80 KiB allows one
        d1k = engine.plots_desc(H, W, thr, ext, max_cells=1024, capacity=cap, complex_weight=True)
        r = timed(lambda: engine.plots_execute(d1k, stat, xc, N, counts, ncells, cands, None, None, stream))
        r["floor_share"] = round(floor / r["ms_median"], 4)
        out[f"prc_plots_pfa{pfa:g}_max_cells_1024"] = r
        c, nc = counts.cpu().numpy(), ncells.cpu().numpy()
        out[f"found_pfa{pfa:g}"] = dict(thresh=round(thr, 6), detections_per_frame_mean=round(float(nc.mean()), 2),
                                       detections_per_frame_max=int(nc.max()), plots_per_frame_mean=round(float(c.mean()), 2),
                                       plots_per_frame_max=int(c.max()), frames_over_max_cells=int((nc > _lib.PLOTS_LDS_CELLS).sum()),
                                       frames_over_capacity=int((c > cap).sum()))

    # get_measurements' rule on the same statistic: every cell at or above the frame's 99.8th percentile
    mcap = 512
    plan = TrackPlan(H, W, 10, mcap, ext)
    mcands = torch.zeros(N * mcap * 32, dtype=torch.uint8, device="cuda")
    out["prc_track_measure"] = timed(lambda: plan.measure(stat.data_ptr(), N, counts.data_ptr(), mcands.data_ptr(), stream))
    out["prc_track_measure"]["candidates_per_frame_mean"] = round(float(counts.cpu().numpy().mean()), 2)
    plan.close()

    # the chain: CFAR -> measurements -> multitarget_tracker, wall clock, device tensor in, records out
    xs = xc[:args.chain_frames]

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

    reps = max(2, args.reps // 2)
    thr = os_cfar_threshold(1e-4, nt, rank)
    out["track_maps"] = dict(frames=int(xs.shape[0]), cfar="os",
                             wall_ms_percentile=wall(lambda: track_maps(xs, ext, cfar="os"), reps),
                             wall_ms_plots=wall(lambda: track_maps(xs, ext, cfar="os", measure="plots", plot_thresh=thr), reps))
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
