"""Times the batches-algorithm surfaces (range_doppler_processing.batch_xambg, prc_batch_xambg) on one MI355X.

Shapes: (L 4096, hop 4608, F 512, R 256) and (L 1024, hop 1152, F 2048, R 256), one frame and 64 frames, reciprocal and matched
filter: HIP events around the call on device tensors, median and minimum of ``--reps``.  Next to each figure stand
  * fast_xambg's plan (prc_caf_execute; this change does not touch it) at the same n, R and F on the same box,
  * the Doppler stage alone -- the same column kernel on the same shape through prc_caf_execute_doppler -- and the batch stage
    as the difference (the two kernels run back to back on one stream),
  * the DERIVED floor: one read of the F L samples of both channels, one write and one read of the slow-time buffer and one
    write of the surface, at the 6.29 TB/s copy ceiling,
and the device's rel_err against the float64 definition (tests/batch_xambg_oracle.py) per batch length and filter, on frame 0.
Prints one JSON line.

    python tools/batch_xambg_bench.py [--reps 20] [--out profiles/batch_xambg_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_TB_S = 6.29        # MI355X copy ceiling (TB/s)
SHAPES = [(4096, 4608, 512, 256, 549), (1024, 1152, 2048, 256, 165)]     # L, hop, F, R, start
FRAMES = [1, 64]


def floor_ms(L, F, R, nframes):
    cols = R + 1
    nbytes = nframes * (2 * 8 * F * L + 3 * 8 * F * cols)
    return nbytes / (HBM_TB_S * 1e12) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    import batch_xambg_oracle as O
    from passiveradar_amd import _lib, engine
    _lib.require_gpu()
    st = _lib.torch_stream_ptr()

    def timed(fn):
        for _ in range(3):
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

    out = dict(tool="batch_xambg_bench", reps=args.reps, hbm_tb_s=HBM_TB_S, gpu_bar=O.GPU_BAR, runs=[], accuracy=[])
    gen = torch.Generator(device="cuda").manual_seed(1234)
    for L, hop, F, R, start in SHAPES:
        n = start + (F - 1) * hop + L
        nf_max = max(FRAMES)
        ref = torch.view_as_complex(torch.randn((nf_max, n, 2), generator=gen, device="cuda") * (0.5 ** 0.5))
        srv = 0.7 * torch.roll(ref, 17, dims=1) + 0.1 * torch.view_as_complex(torch.randn((nf_max, n, 2), generator=gen, device="cuda"))
        surf = torch.empty((nf_max, F, R + 1), dtype=torch.complex64, device="cuda")
        plan = engine.CafPlan(n, R, F, max_frames=nf_max)
        for filt in ("reciprocal", "matched"):
            d = engine.batch_xambg_desc(n, L, R, F, hop, start, _lib.BATCH_FILTERS[filt], 0.1)
            ws = torch.empty(engine.batch_xambg_workspace_bytes(d, nf_max), dtype=torch.uint8, device="cuda")
            engine.batch_xambg_execute(d, ref, srv, n, None, surf, 1, ws, st)
            torch.cuda.synchronize()
            want = O.surface(ref[0].cpu().numpy(), srv[0].cpu().numpy(), L, F, R, hop, start, filt, 0.1)
            out["accuracy"].append(dict(batch_len=L, freq_bins=F, range_bins=R, filter=filt,
                                        rel_err=float("%.3g" % O.rel_err(surf[0].cpu().numpy(), want))))
            for nf in FRAMES:
                ms, best = timed(lambda: engine.batch_xambg_execute(d, ref, srv, n, None, surf, nf, ws, st))
                caf, caf_best = timed(lambda: plan.execute(ref, srv, surf, nf, n, n, None, stream=st))
                plan.execute_segments(ref, srv, nf, n, n, None, stream=st)
                dop, dop_best = timed(lambda: plan.execute_doppler(surf, nf, stream=st))
                fl = floor_ms(L, F, R, nf)
                out["runs"].append(dict(batch_len=L, hop=hop, freq_bins=F, range_bins=R, n=n, nframes=nf, filter=filt, ms=ms, best_ms=best,
                                        doppler_stage_ms=dop, batch_stage_ms=round(ms - dop, 4), fast_xambg_ms=caf,
                                        fast_xambg_best_ms=caf_best, fast_xambg_method=plan.method, floor_ms=round(fl, 4),
                                        share_of_floor=round(fl / ms, 4), input_gb_s=round(nf * 16.0 * F * L / ms / 1e6, 1)))
        plan.close()
        del ref, srv, surf
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
