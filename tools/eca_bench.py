"""Times ECA_Filter (passiveradar_amd/csrc/eca.hip) stage by stage on one MI355X at the LS block shape of config 2 (hop chunks of
1 200 000 samples, 256 + 10 taps, bins 0, +-1, +-2 Hz at Fs = 2.4 MHz): one block, and one call of --blocks blocks (256), on a
white reference with a decaying clutter filter whose echoes fluctuate slowly.

Stages, from the library's own events (prc_eca_set_profiling): correlate (float64 correlations of every pair of regressors and
their reduction), solve (block Levinson) and apply (the FIR of every bin).  Each is given beside its DERIVED floor at the
78.6 TFLOP/s (39.3e12 FMA/s) of vector float64 and the 8 TB/s of HBM the MI355X is specified with:

    correlate  n T B (B + 1) complex multiply-adds of 4 float64 FMAs;  16 n bytes read (nothing of size n is written)
    solve      sum over steps m of 4 (m + 1) B^3 + 2 (m + 1) B^2 complex multiply-adds = T^2 (8 B^3 + 4 B^2) FMAs, on ONE
               compute unit per block (1/256 of the device), so the floor does not shrink until 256 blocks share a call
    apply      n T B complex multiply-adds of 4 float64 FMAs;  24 n bytes (ref, srv read, out written)

prc_ls_execute (LS_Filter_Multiple's chain over the same bins) runs on the same input beside it, for scale only: it solves
another problem (one bin after another) with float32 FFT kernels.  Prints one JSON line.

    python tools/eca_bench.py [--reps 3] [--blocks 256] [--out profiles/eca_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

FP64_FMA_PER_S = 39.3e12
HBM_BYTES_PER_S = 8.0e12
CUS = 256
N, L, PEEK, FS = 1200000, 256, 10, 2.4e6
BINS = (0.0, 1.0, -1.0, 2.0, -2.0)


def floors_ms(n, T, B, nblocks):
    corr = max(nblocks * n * T * B * (B + 1) * 4 / FP64_FMA_PER_S, nblocks * 16 * n / HBM_BYTES_PER_S)
    solve = -(-nblocks // CUS) * T * T * (8 * B ** 3 + 4 * B ** 2) / (FP64_FMA_PER_S / CUS)
    apply = max(nblocks * n * T * B * 4 / FP64_FMA_PER_S, nblocks * 24 * n / HBM_BYTES_PER_S)
    return {"correlate": corr * 1e3, "solve": solve * 1e3, "apply": apply * 1e3}


def make_input(torch, dev, nblocks):
    """[nblocks, N] ref and srv: a decaying clutter filter whose taps drift by a fraction of a hertz, plus noise"""
    T = L + PEEK
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    ref = torch.view_as_complex(torch.randn((nblocks, N, 2), generator=g, device=dev))
    srv = 0.05 * torch.view_as_complex(torch.randn((nblocks, N, 2), generator=g, device=dev))
    t = torch.arange(N, device=dev, dtype=torch.float64) / FS
    for d, (f, amp) in enumerate(((0.0, 1.0), (0.6, 0.3), (-1.4, 0.2), (1.0, 0.1))):
        rot = torch.exp(2j * np.pi * f * t).to(torch.complex64)
        srv += amp * torch.roll(ref, 2 + 3 * d, dims=1) * rot
    assert T < N
    return ref.contiguous(), srv.contiguous()


def time_eca(torch, engine, ref, srv, nblocks, reps):
    B, T = len(BINS), L + PEEK
    out = torch.empty_like(srv)
    info = torch.empty(nblocks, dtype=torch.int32, device=ref.device)
    ws = torch.empty(engine.eca_workspace_bytes(N, L, PEEK, B, nblocks), dtype=torch.uint8, device=ref.device)
    runs = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        engine.eca_execute(ref, srv, out, N, L, PEEK, FS, BINS, 0.0, nblocks, N, N, None, info, ws)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            runs.append(list(engine.eca_get_profile()) + [wall])
    med = np.median(np.array(runs), axis=0)
    fl = floors_ms(N, T, B, nblocks)
    ms = {"correlate": float(med[0]), "solve": float(med[1]), "apply": float(med[2])}
    res = {"blocks": nblocks, "ms": {k: round(v, 4) for k, v in ms.items()}, "wall_ms": round(float(med[3]), 3),
           "floor_ms": {k: round(v, 4) for k, v in fl.items()},
           "fraction_of_floor": {k: round(fl[k] / ms[k], 4) for k in ms},
           "flagged_blocks": int(info.sum().item()),
           "residual_power": float((out[0].abs() ** 2).mean() / (srv[0].abs() ** 2).mean()),
           "workspace_mb": round(ws.numel() / 1e6, 1)}
    return res, out


def time_chain(torch, engine, ref, srv, nblocks, reps):
    plan = engine.LsPlan(N, L, PEEK, False, nblocks, 0)
    out = torch.empty_like(srv)
    runs = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.execute(ref, srv, out, nblocks, N, N, FS, BINS, 0.0, None, None)
        torch.cuda.synchronize()
        if rep:
            runs.append((time.perf_counter() - t0) * 1e3)
    res = {"blocks": nblocks, "wall_ms": round(float(np.median(runs)), 3),
           "residual_power": float((out[0].abs() ** 2).mean() / (srv[0].abs() ** 2).mean())}
    plan.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=256, help="blocks of the batched call (0: skip it)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import engine
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "fp64_fma_per_s": FP64_FMA_PER_S, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "reps": args.reps, "n": N, "filter_len": L, "peek": PEEK, "taps": L + PEEK, "bins_hz": list(BINS), "sample_rate": FS,
           "eca": [], "ls_chain_for_scale": []}
    engine.eca_set_profiling(True)
    for nblocks in (1, args.blocks):
        if nblocks < 1:
            continue
        ref, srv = make_input(torch, dev, nblocks)
        r, _ = time_eca(torch, engine, ref, srv, nblocks, args.reps)
        res["eca"].append(r)
        print("eca", json.dumps(r), file=sys.stderr, flush=True)
        c = time_chain(torch, engine, ref, srv, nblocks, args.reps)
        res["ls_chain_for_scale"].append(c)
        print("chain", json.dumps(c), file=sys.stderr, flush=True)
        del ref, srv
        torch.cuda.empty_cache()
    engine.eca_set_profiling(False)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
