"""Times the joint echo canceller (clutter_removal.cancel_echoes, prc_echo_cancel) on one MI355X.

Shapes: one config-2 frame (n = 2 400 000 samples at 2.4 MHz) with 4 atoms and with 32 atoms, and a stack of 256 frames of
65 536 samples with 4 atoms each; Doppler-slope columns on, white complex64 reference, echoes at the atoms' lags with Dopplers
0.2 cell off the listed ones.  Device events around the call on preallocated buffers, median of --reps after two warm-ups.

Stages.  The entry point has no profiling switch (it stays capturable), so the stage times are DIFFERENCES of whole calls:
    pass  = (t(refine = 2) - t(refine = 0)) / 2          one Gram + reduce + solve pass
    apply = t(refine = 0) - pass                          the atom list's working copy and the streaming subtraction
    solve = the same `pass` difference at n = 1024        reduce + solve with next to no Gram work (launch gaps included)
    gram  = pass - solve
Every difference carries the noise of both of its calls.

DERIVED floors, printed beside the times and never used as a threshold:
    gram:  8 n (C + 1)(C + 2) / 2 float64 flop per pass at the float64 vector rate, 78.6 TFLOP/s -- half of the 157.3 TFLOP/s
           float32 vector peak the microarchitecture notes give (AMD's MI355X data sheet states the float64 vector figure);
    apply: 16 n bytes (one read of srv, one write of out) at the 6.29 TB/s copy ceiling DESIGN.md uses.

    python tools/echo_bench.py [--reps 10] [--commit ID] [--out profiles/echo_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_CEILING_TBS = 6.29
FP64_VECTOR_TFLOPS = 78.6


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def atoms_of(k):
    """k atoms at lags 5 j + 2, Dopplers spread over +-60 cells"""
    return [5 * j + 2 for j in range(k)], [float((23 * j) % 121 - 60) + 0.4 for j in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default=None, help="commit id to record (default: git rev-parse HEAD of this tree)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib, engine
    _lib.require_gpu()
    st = _lib.torch_stream_ptr()

    def scene(nframes, n, fs, lags, dops):
        gen = torch.Generator(device="cuda").manual_seed(7)
        ref = torch.complex(torch.randn((nframes, n), generator=gen, device="cuda"), torch.randn((nframes, n), generator=gen, device="cuda"))
        ref = (ref * (0.5 ** 0.5)).contiguous()
        srv = 1e-3 * torch.complex(torch.randn((nframes, n), generator=gen, device="cuda"),
                                   torch.randn((nframes, n), generator=gen, device="cuda"))
        i = torch.arange(n, device="cuda", dtype=torch.float64)
        for j, (lag, f) in enumerate(zip(lags, dops)):
            turns = torch.remainder((f + 0.2 * fs / n) / fs * i, 1.0)
            ph = torch.polar(torch.ones_like(turns), 2 * np.pi * turns).to(torch.complex64)
            srv += torch.roll(ref, lag, dims=1) * ph / (1 + 0.2 * j)
        return ref, srv.contiguous()

    def timed(nframes, n, fs, lags, dops, ref, srv, refine):
        M = len(lags)
        d = engine.echo_desc(n, fs, M, nframes, True, True, refine)
        rec = np.zeros((nframes, M), _lib.ECHO_ATOM_DTYPE)
        rec["lag"], rec["doppler"] = lags, dops
        atoms = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
        counts = torch.full((nframes,), M, dtype=torch.int32, device="cuda")
        out = torch.empty_like(srv)
        fit = torch.empty(nframes * M * _lib.ECHO_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        info = torch.empty(nframes, dtype=torch.int32, device="cuda")
        ws = torch.empty(engine.echo_workspace_bytes(d), dtype=torch.uint8, device="cuda")
        ms = []
        for k in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            engine.echo_execute(d, ref, srv, atoms, counts, out, fit, info, ws, st)
            b.record()
            b.synchronize()
            if k >= 2:
                ms.append(a.elapsed_time(b))
        assert not info.cpu().numpy().any()
        p = lambda x: float((x.abs().to(torch.float64) ** 2).sum())
        return float(np.median(ms)), 10 * np.log10(p(out) / p(srv)), int(ws.numel())

    rows = []
    for name, nframes, n, k in (("config-2 frame, 4 atoms", 1, 2_400_000, 4), ("config-2 frame, 32 atoms", 1, 2_400_000, 32),
                                ("256 frames of 65536, 4 atoms", 256, 65_536, 4)):
        fs = 2.4e6
        lags, dops = atoms_of(k)
        ref, srv = scene(nframes, n, fs, lags, dops)
        t0, _, _ = timed(nframes, n, fs, lags, dops, ref, srv, 0)
        t2, db, wsb = timed(nframes, n, fs, lags, dops, ref, srv, 2)
        small = scene(nframes, 1024, fs, lags, dops)
        s0, _, _ = timed(nframes, 1024, fs, lags, dops, small[0], small[1], 0)
        s2, _, _ = timed(nframes, 1024, fs, lags, dops, small[0], small[1], 2)
        C = 2 * k
        pass_ms, solve_ms = (t2 - t0) / 2, (s2 - s0) / 2
        rows.append({
            "shape": name, "nframes": nframes, "n": n, "atoms": k, "columns": C, "workspace_bytes": wsb,
            "ms_call_refine0": t0, "ms_call_refine2": t2, "residual_db_refine2": db,
            "ms_pass": pass_ms, "ms_solve_and_reduce": solve_ms, "ms_gram": pass_ms - solve_ms, "ms_apply": t0 - pass_ms,
            "floor_ms_gram": 8.0 * n * nframes * (C + 1) * (C + 2) / 2 / (FP64_VECTOR_TFLOPS * 1e12) * 1e3,
            "floor_ms_apply": 16.0 * n * nframes / (COPY_CEILING_TBS * 1e12) * 1e3,
        })
        del ref, srv
        torch.cuda.empty_cache()
    res = {"bench": "echo_cancel", "commit": args.commit or commit_id(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "method": "device events around whole calls; stage times are differences of calls (see tools/echo_bench.py)",
           "floors": {"fp64_vector_tflops": FP64_VECTOR_TFLOPS, "copy_ceiling_tbs": COPY_CEILING_TBS,
                      "note": "derived, never used as a threshold"},
           "rows": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
