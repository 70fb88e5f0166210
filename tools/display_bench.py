"""Times the display path at the published size on one MI355X: 1199 persistence frames of 1024 Doppler x 177 range bins.
HIP events around prc_display_limits and prc_display_rgba alone (float64 and float32 stacks, "plot" and "stored"
orientation), render_frames from a device stack, and the whole render_maps chain from complex maps (CFAR ->
persistence -> limits -> RGBA, in slabs).  The HBM floors are DERIVED (bytes each kernel must move once, at the
6.29 TB/s copy ceiling), not measured.  The reference's side -- np.percentile x 2 plus a NumPy colour mapping per
float64 frame -- is timed on one core of the host the tool runs on (--reference-only: nothing else, no GPU needed).
Prints one JSON line.

    python tools/display_bench.py [--frames 1199] [--reps 10] [--out profiles/display_bench.json]
    python tools/display_bench.py --reference-only
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TB_S = 6.29        # MI355X peak HBM bandwidth (TB/s)
H, W = 1024, 177


def reference_ms_per_frame(nframes=12):
    """range_doppler_plot.py:73-76 + the colour mapping of imshow, in NumPy, per 1024 x 177 float64 frame"""
    from passiveradar_amd.plotting_tools import gnuplot2_lut
    lut = gnuplot2_lut()
    rng = np.random.default_rng(0)
    frames = rng.exponential(1.0, (nframes, H, W))
    t_pct, t_map = [], []
    for f in frames:
        t0 = time.perf_counter()
        data = np.fliplr(f.T)
        vmn = np.percentile(data.flatten(), 35)
        vmx = 1.5 * np.percentile(data.flatten(), 99)
        t1 = time.perf_counter()
        xa = (data - vmn) / (vmx - vmn) * 256.0
        idx = np.clip(xa, 0, 255).astype(np.intp)
        px = lut[idx]
        t2 = time.perf_counter()
        assert px.shape == (W, H, 4)
        t_pct.append((t1 - t0) * 1e3)
        t_map.append((t2 - t1) * 1e3)
    return dict(frames=nframes, percentiles_ms_per_frame=round(float(np.median(t_pct)), 3),
                colour_map_ms_per_frame=round(float(np.median(t_map)), 3),
                total_ms_per_frame=round(float(np.median(t_pct) + np.median(t_map)), 3), numpy=np.__version__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    out = dict(tool="display_bench", frames=args.frames, H=H, W=W, reps=args.reps)
    out["reference_one_cpu_core"] = reference_ms_per_frame()
    if not args.reference_only:
        import torch
        from passiveradar_amd import _lib
        from passiveradar_amd.plotting_tools import persistence_stack, render_frames, render_maps
        _lib.require_gpu()
        lib = _lib.lib()
        N, n = args.frames, H * W
        gen = torch.Generator(device="cuda").manual_seed(1234)
        cf = -torch.log1p(-torch.rand((N, H, W), generator=gen, device="cuda", dtype=torch.float32) * 0.999999)
        x64 = persistence_stack(cf, 20, 0.9)
        x32 = x64.to(torch.float32)
        lim = torch.empty((N, 2), dtype=torch.float64, device="cuda")
        px = torch.empty((N, W, H, 4), dtype=torch.uint8, device="cuda")
        stream = _lib.torch_stream_ptr()

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
            return float(np.median(ts))

        def limits(x, code):
            _lib.check(lib.prc_display_limits(x.data_ptr(), code, n, N, 35.0, 99.0, 1.5, lim.data_ptr(), stream))

        def rgba(x, code, orient):
            _lib.check(lib.prc_display_rgba(x.data_ptr(), code, H, W, N, lim.data_ptr(), None, orient, px.data_ptr(), stream))

        for tag, x, code, size in (("f64", x64, _lib.REAL_F64, 8), ("f32", x32, _lib.REAL_F32, 4)):
            t_lim = timed(lambda: limits(x, code))
            t_plot = timed(lambda: rgba(x, code, _lib.DISPLAY_PLOT))
            t_stored = timed(lambda: rgba(x, code, _lib.DISPLAY_STORED))
            fl_lim = N * n * size / (HBM_TB_S * 1e12) * 1e3
            fl_px = N * n * (size + 4) / (HBM_TB_S * 1e12) * 1e3
            out[tag] = dict(limits_ms=round(t_lim, 4), rgba_plot_ms=round(t_plot, 4), rgba_stored_ms=round(t_stored, 4),
                            limits_hbm_floor_ms_derived=round(fl_lim, 4), rgba_hbm_floor_ms_derived=round(fl_px, 4),
                            limits_share_of_floor=round(fl_lim / t_lim, 3), rgba_plot_share_of_floor=round(fl_px / t_plot, 3),
                            rgba_stored_share_of_floor=round(fl_px / t_stored, 3),
                            render_frames_ms=round(timed(lambda: render_frames(x)), 4))
        del x64, x32
        xc = torch.complex(cf, torch.zeros_like(cf))
        del cf
        out["render_maps_ms"] = round(timed(lambda: render_maps(xc)), 4)
        out["render_maps_us_per_frame"] = round(out["render_maps_ms"] * 1e3 / N, 3)
        out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
