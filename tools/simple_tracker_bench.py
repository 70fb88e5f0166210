"""Times simple_target_tracker and persistence at the published size on one MI355X: 1199 frames of 1024 Doppler x 177
range bins (float32, a wandering target that fades in and out).  HIP events around prc_strack_run (scan + walk), the
simple_target_tracker drop-in from a device tensor (including its workspace, record download and history build), the
simple_track_maps chain from complex maps, and persistence_stack with float64 and float32 output.  The scan / walk split
comes from a rocprofv3 kernel-stats CSV of an earlier run of this tool (--kernel-stats).  Prints one JSON line.

    rocprofv3 --kernel-trace --stats -d OUT -o strack -- python tools/simple_tracker_bench.py --reps 3
    python tools/simple_tracker_bench.py [--frames 1199] [--reps 10] [--kernel-stats OUT/.../strack_kernel_stats.csv]
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TB_S = 6.29        # MI355X peak HBM bandwidth (TB/s)


def published_batch(torch, N, H, W):
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = -torch.log1p(-torch.rand((N, H, W), generator=gen, device="cuda", dtype=torch.float32) * 0.999999)
    rng = np.random.default_rng(1)
    r = np.clip(90 + np.cumsum(rng.normal(0, 0.4, N)), 12, W - 12).round().astype(int)
    c = np.clip(600 + np.cumsum(rng.normal(0, 1.0, N)), 40, H - 40).round().astype(int)
    on = (np.arange(N) // 150) % 4 != 3
    idx = torch.tensor(np.nonzero(on)[0], device="cuda")
    x[idx, torch.tensor(H - 1 - c[on], device="cuda"), torch.tensor(r[on], device="cuda")] += 60.0
    return x.contiguous()


def kernel_stats(path):
    """{kernel family: mean ns} from a rocprofv3 *_kernel_stats.csv"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for fam in ("strack_scan_kernel", "strack_walk_kernel", "persistence_kernel"):
                if fam in name:
                    out.setdefault(fam, []).append(float(row["AverageNs"]))
    return {k: v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.plotting_tools import persistence_stack
    from passiveradar_amd.target_detection import _strack_desc, simple_target_tracker, simple_track_maps

    _lib.require_gpu()
    N, H, W = args.frames, 1024, 177
    ext = (375.0, 256 / 1.092)
    x = published_batch(torch, N, H, W)
    d = _strack_desc(H, W, _lib.REAL_F32, *ext)
    nb = C.c_size_t(0)
    _lib.check(_lib.lib().prc_strack_workspace_bytes(C.byref(d), N, C.byref(nb)))
    ws = torch.empty(max(nb.value, 8), dtype=torch.uint8, device="cuda")
    rec = torch.empty(N * 272, dtype=torch.uint8, device="cuda")
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

    t_run = timed(lambda: _lib.check(_lib.lib().prc_strack_run(C.byref(d), x.data_ptr(), N, None, rec.data_ptr(),
                                                               ws.data_ptr(), stream)))
    h = simple_target_tracker(x, *ext)
    gated = int(np.count_nonzero(np.concatenate(([0.0], h["lock_mode"][:-1, 0])) == 0))
    t_drop = timed(lambda: simple_target_tracker(x, *ext))
    t_p64 = timed(lambda: persistence_stack(x, 20, 0.9))
    t_p32 = timed(lambda: persistence_stack(x, 20, 0.9, out_dtype=np.float32))
    xc = torch.complex(x, torch.zeros_like(x))
    t_chain = timed(lambda: simple_track_maps(xc, *ext))
    floor64 = (N * H * W * 4 + N * H * W * 8) / (HBM_TB_S * 1e12) * 1e3
    floor32 = (N * H * W * 4 + N * H * W * 4) / (HBM_TB_S * 1e12) * 1e3
    out = dict(tool="simple_tracker_bench", frames=N, H=H, W=W, reps=args.reps, gated_frames=gated,
               strack_run_ms=round(t_run, 4), drop_in_ms=round(t_drop, 4), simple_track_maps_ms=round(t_chain, 4),
               persistence_stack_f64_ms=round(t_p64, 4), persistence_stack_f32_ms=round(t_p32, 4),
               persistence_hbm_floor_f64_ms=round(floor64, 4), persistence_hbm_floor_f32_ms=round(floor32, 4),
               persistence_f64_share_of_floor=round(floor64 / t_p64, 3),
               persistence_f32_share_of_floor=round(floor32 / t_p32, 3),
               device=torch.cuda.get_device_name(0))
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        if "strack_scan_kernel" in ks:
            out["scan_ms"] = round(min(ks["strack_scan_kernel"]) / 1e6, 4)
            out["scan_tb_per_s"] = round(N * H * W * 4 / (out["scan_ms"] * 1e-3) / 1e12, 3)
        if "strack_walk_kernel" in ks:
            out["walk_ms"] = round(min(ks["strack_walk_kernel"]) / 1e6, 4)
            out["walk_us_per_frame"] = round(out["walk_ms"] * 1e3 / N, 3)
            out["walk_us_per_gated_frame_upper"] = round(out["walk_ms"] * 1e3 / max(gated, 1), 3)
        if "persistence_kernel" in ks:
            out["persistence_kernel_ms"] = [round(v / 1e6, 4) for v in ks["persistence_kernel"]]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
