"""Times LS_Filter_SVD (passiveradar_amd/csrc/ls_svd.hip) stage by stage on one MI355X, one block per shape, at the LS block
shapes of config 2 and config 3 as tools/ls_chain_bench.py has them (hop chunks of 1 200 000 samples; 256 + 10 and
1034 + 10 taps), on a white reference with a decaying clutter filter.

Stages, from the library's own events (prc_ls_svd_set_profiling): correlate (float64 circular correlations and their
reduction), jacobi (Gram set-up, the sweeps, one counter read-back per sweep), taps (eigenvalues, cut, taps) and apply (the
circular FIR).  The correlation is also given as a fraction of its DERIVED floor: n * T * 2 correlations * 4 float64
multiply-adds at the 78.6 TFLOP/s (39.3e12 FMA/s) of vector float64 the MI355X is specified with.

The same arithmetic as the reference's LS_Filter_SVD (complex64 N x T matrix of circular shifts, LAPACK SVD, taps,
matrix-vector product) is timed in NumPy on one core of the host at a reduced n: at the full size that matrix alone is
2.5 GB (config 2) and 10 GB (config 3).  Prints one JSON line.

    python tools/ls_svd_bench.py [--reps 3] [--cpu-n 32768] [--out profiles/ls_svd_bench.json]
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
SHAPES = {"cfg2": (1200000, 256, 10), "cfg3": (1200000, 1034, 10)}


def numpy_same_arithmetic_s(n, L, peek, rng):
    ref = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    srv = (np.roll(ref, 2) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    from threadpoolctl import threadpool_limits
    with threadpool_limits(limits=1):                       # one core, whatever the environment sets for BLAS
        t0 = time.perf_counter()
        A = np.empty((n, L + peek), np.complex64)
        for k in range(L + peek):
            A[:, k] = np.roll(ref, k - peek)
        U, S, VH = np.linalg.svd(A, full_matrices=False)
        inv = np.where(S < 1e-10, 0.0, 1.0 / np.where(S > 0, S, 1.0)).astype(np.float32)
        h = VH.conj().T @ (inv * (U.conj().T @ srv))
        out = srv - A @ h
        dt = time.perf_counter() - t0
    assert np.isfinite(out).all()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-n", type=int, default=32768)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import engine
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "fp64_fma_per_s": FP64_FMA_PER_S, "reps": args.reps, "shapes": {}}
    engine.ls_svd_set_profiling(True)
    for name, (n, L, peek) in SHAPES.items():
        if args.only and name not in args.only.split(","):
            continue
        T = L + peek
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        ref = torch.view_as_complex(torch.randn((n, 2), generator=g, device=dev))
        h0 = torch.view_as_complex(torch.randn((T, 2), generator=g, device=dev)) * torch.exp(-torch.arange(T, device=dev) / 6.0)
        hp = torch.zeros(n, dtype=torch.complex64, device=dev)
        hp[:T] = h0
        srv = torch.fft.ifft(torch.fft.fft(torch.roll(ref, -peek)) * torch.fft.fft(hp)) \
            + 0.05 * torch.view_as_complex(torch.randn((n, 2), generator=g, device=dev))
        srv = srv.contiguous()
        out = torch.empty_like(srv)
        info = torch.empty(3, dtype=torch.int32, device=dev)
        ws = torch.empty(engine.ls_svd_workspace_bytes(n, L, peek, 1), dtype=torch.uint8, device=dev)
        runs = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            engine.ls_svd_execute(ref, srv, out, n, L, peek, None, 1, n, n, None, None, info, ws)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms, sweeps = engine.ls_svd_get_profile()
            if rep:
                runs.append(list(ms) + [wall])
        med = np.median(np.array(runs), axis=0)
        kept, sw, conv = (int(v) for v in info.cpu().numpy())
        floor = n * T * 2 * 4 / FP64_FMA_PER_S * 1e3
        res["shapes"][name] = {
            "n": n, "filter_len": L, "peek": peek, "taps": T, "kept": kept, "sweeps": sw, "converged": conv,
            "residual_power": float((out.abs() ** 2).mean() / (srv.abs() ** 2).mean()),
            "ms": {"correlate": round(float(med[0]), 4), "jacobi": round(float(med[1]), 4), "taps": round(float(med[2]), 4),
                   "apply": round(float(med[3]), 4)},
            "wall_ms": round(float(med[4]), 3),
            "correlate_fp64_fma_floor_ms": round(floor, 4),
            "correlate_fraction_of_fp64_fma_floor": round(floor / float(med[0]), 4),
            "workspace_mb": round(ws.numel() / 1e6, 1),
        }
        print(name, json.dumps(res["shapes"][name]), file=sys.stderr, flush=True)
    engine.ls_svd_set_profiling(False)
    _, L, peek = SHAPES["cfg2"]
    secs = numpy_same_arithmetic_s(args.cpu_n, L, peek, np.random.default_rng(1))
    res["reference_cpu"] = {"what": "NumPy, the reference's arithmetic (complex64 N x T matrix, LAPACK SVD), one core of the host",
                            "n": args.cpu_n, "filter_len": L, "peek": peek, "seconds": round(secs, 3),
                            "matrix_gb_at_full_n": {k: round(v[0] * (v[1] + v[2]) * 8 / 1e9, 2) for k, v in SHAPES.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
