"""Times the exact ambiguity patches (range_doppler_processing.xambg_patch, prc_xambg_patch) on one MI355X.

(a) a config-2 frame (n = 2 400 000, Kaiser window): ten patches of 16 lags x 16 Dopplers in one call, as a detector
    would ask for around its CFAR hits, and one patch of 64 lags x 512 Dopplers; plus refine_peaks on the ten.
(b) a direct_xambg-shaped surface at n = 262 144, R = 63, F = 64 (one patch of 64 x 64, wrap off), next to the
    ``direct_xambg`` drop-in on the same shape.  direct_xambg is what it was before this tool existed -- a host loop of
    2 F launches on host-staged arrays -- so its time here is the earlier commit's; it has no device-tensor form, so both
    are timed wall-clock from NumPy arrays in to a NumPy array out, and the patch call also with HIP events on device
    tensors.

Each device time is given next to two DERIVED floors (recorded, not thresholds): the arithmetic, 8 n nlags (ndoppler + 1)
flop per patch -- one complex multiply-add per (sample, lag, Doppler) and one lag product per (sample, lag) -- at the
~100 TFLOP/s packed fp32 multiply-adds sustain; and the memory traffic, 8 n (ref) + 4 n (window) +
8 (n + nlags) (srv) bytes per (patch, group of 64 lags, group of 16 Dopplers) pass at the 6.29 TB/s copy ceiling.  The
passes of one frame re-read the same 38 MB; whether those re-reads are served from the Infinity Cache has NOT been
measured, so the memory floor is an upper bound on what HBM must deliver, not a statement of where the bytes came from.
Prints one JSON line.

    python tools/xambg_patch_bench.py [--reps 10] [--out profiles/xambg_patch_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TB_S = 6.29        # MI355X copy ceiling (TB/s)
FP32_TFLOPS = 100.0    # packed fp32 multiply-adds, sustained


def floors(n, npatches, nlags, ndoppler, windowed):
    flop = 8.0 * n * nlags * (ndoppler + 1) * npatches
    passes = npatches * -(-nlags // 64) * -(-ndoppler // 16)
    byts = passes * (8.0 * n + (4.0 * n if windowed else 0.0) + 8.0 * (n + min(nlags, 64)))
    return dict(flop=flop, arithmetic_ms=round(flop / (FP32_TFLOPS * 1e12) * 1e3, 5), passes=passes, bytes=byts,
                memory_ms=round(byts / (HBM_TB_S * 1e12) * 1e3, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib, scene
    from passiveradar_amd.range_doppler_processing import direct_xambg, xambg_patch
    from passiveradar_amd.target_detection import refine_peaks
    _lib.require_gpu()
    out = dict(tool="xambg_patch_bench", reps=args.reps, hbm_tb_s=HBM_TB_S, fp32_tflops=FP32_TFLOPS,
               infinity_cache="unmeasured: the passes of one frame re-read the same data; where those re-reads are served from "
                              "was not measured")

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
        return round(float(np.median(ts)), 4), round(float(np.min(ts)), 4)

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 3)

    def entry(n, npatches, nlags, ndoppler, t):
        f = floors(n, npatches, nlags, ndoppler, True)
        return dict(n=n, npatches=npatches, nlags=nlags, ndoppler=ndoppler, ms_median=t[0], ms_min=t[1], floors=f,
                    tflops=round(f["flop"] / (t[0] * 1e-3) / 1e12, 2),
                    arithmetic_floor_share=round(f["arithmetic_ms"] / t[0], 4), memory_floor_share=round(f["memory_ms"] / t[0], 4))

    # (a) config 2: n = 2.4 M samples at 2.4 MS/s
    n, fs = 2400000, 2.4e6
    ref, srv = scene.make_scene(n, fs, 256, scene.scene_seed(2))
    tr, ts_, tw = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda(), torch.from_numpy(np.kaiser(n, 5.0).astype(np.float32)).cuda()
    rng = np.random.default_rng(2)
    lags = rng.integers(0, 240, 10)
    dops = rng.uniform(-150.0, 150.0, 10)
    step = 0.25 * fs / n
    t10 = timed(lambda: xambg_patch(tr, ts_, fs, lags, dops, 16, 16, step, tw))
    X10 = xambg_patch(tr, ts_, fs, lags, dops, 16, 16, step, tw)
    tpk = timed(lambda: refine_peaks(X10, lags, dops, step))
    t1 = timed(lambda: xambg_patch(tr, ts_, fs, [0], [-64.0], 64, 512, step, tw))
    out["config2_ten_16x16"] = entry(n, 10, 16, 16, t10)
    out["config2_ten_16x16"]["refine_peaks_ms_median"] = tpk[0]
    out["config2_one_64x512"] = entry(n, 1, 64, 512, t1)
    del tr, ts_, tw

    # (b) a direct_xambg-shaped surface
    n, R, F = 262144, 63, 64
    fs = float(n)
    ref, srv = scene.make_scene(n, fs, R, scene.scene_seed(2, 1))
    tr, ts_ = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()
    args_ = ([0], [-0.5 * F], R + 1, F, 1.0, None, False)
    td = timed(lambda: xambg_patch(tr, ts_, fs, *args_))
    w_patch = wall(lambda: xambg_patch(ref, srv, fs, *args_), args.reps)
    w_direct = wall(lambda: direct_xambg(ref, srv, R, F, fs), max(2, args.reps // 3))
    a = xambg_patch(ref, srv, fs, *args_)[0][:, ::-1]
    b = direct_xambg(ref, srv, R, F, fs)[:, :, 0]
    f = floors(n, 1, R + 1, F, False)
    out["direct_surface"] = dict(n=n, rangeBins=R, freqBins=F, patch_device_ms_median=td[0], patch_device_ms_min=td[1],
                                 patch_numpy_in_numpy_out_ms=w_patch, direct_xambg_numpy_in_numpy_out_ms=w_direct,
                                 direct_xambg_over_patch=round(w_direct / w_patch, 2), floors=f,
                                 tflops=round(f["flop"] / (td[0] * 1e-3) / 1e12, 2),
                                 surfaces_differ_by_peak_relative=float(np.abs(a - b).max() / np.abs(b).max()),
                                 note="direct_xambg's float32 phase ramp is what separates the two surfaces")
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
