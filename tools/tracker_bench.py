"""Times the tracker feature at the published size on one MI355X: 1199 frames of 1024 Doppler x 177 range bins with three
moving targets.  HIP events around prc_track_measure, prc_track_run and the whole track_maps chain (CFAR_2D_abs of the
complex maps -> measure -> run, including its count read-back and the record download).  Prints one JSON line.

    python tools/tracker_bench.py [--frames 1199] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def published_batch(torch, N, H, W):
    """the benchmark's input, built on the device: exponential clutter and three targets moving as the tracker's model
    says (range rate -0.003 km per Hz per frame); extents [250 Hz, 300 km]"""
    ext = [250.0, 300.0]
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = -torch.log1p(-torch.rand((N, H, W), generator=gen, device="cuda", dtype=torch.float32) * 0.999999)
    dpts = np.linspace(-ext[0], ext[0], H)
    rpts = np.linspace(ext[1], 0, W)
    hh = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    ww = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    t = np.arange(N)
    for f0, r0 in ((-20.0, 80.0), (30.0, 250.0), (-5.0, 150.0)):
        w = np.interp(r0 - 0.003 * f0 * t, rpts[::-1], np.arange(W)[::-1])
        h = H - 1 - np.interp(np.full(N, f0), dpts, np.arange(H))
        th = torch.tensor(h, device="cuda", dtype=torch.float32)[:, None, None]
        tw = torch.tensor(w, device="cuda", dtype=torch.float32)[:, None, None]
        x += 60.0 * torch.exp(-((hh - th) ** 2 / 2.0 + (ww - tw) ** 2 / 1.0))
    return x.contiguous(), ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import TrackPlan, expected_capacity, track_maps

    _lib.require_gpu()
    N, H, W = args.frames, 1024, 177
    x, ext = published_batch(torch, N, H, W)
    cap = expected_capacity(H, W)
    plan = TrackPlan(H, W, 10, cap, ext)
    counts = torch.empty(N, dtype=torch.int32, device="cuda")
    cands = torch.empty(N * cap * 32, dtype=torch.uint8, device="cuda")
    recs = torch.empty(N * 10 * 256, dtype=torch.uint8, device="cuda")
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

    t_meas = timed(lambda: plan.measure(x.data_ptr(), N, counts.data_ptr(), cands.data_ptr(), stream))
    assert int(counts.max()) <= cap
    t_run = timed(lambda: plan.run(counts.data_ptr(), cands.data_ptr(), N, recs.data_ptr(), stream))
    # the chain from the complex maps: |x| of the clutter-plus-target magnitudes as the real part
    xc = torch.complex(x, torch.zeros_like(x))
    del x
    t_chain = timed(lambda: track_maps(xc, ext, 10))
    out = dict(tool="tracker_bench", frames=N, H=H, W=W, capacity=cap, reps=args.reps,
               measure_ms=round(t_meas, 4), run_ms=round(t_run, 4), track_maps_ms=round(t_chain, 4),
               frames_per_s=round(N / (t_chain * 1e-3), 1),
               measure_tb_per_s=round(N * H * W * 4 / (t_meas * 1e-3) / 1e12, 4),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
