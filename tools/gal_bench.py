"""ns per step per stream of prc_gal_execute, and of prc_nlms_execute at the same tap count, on the GPU:

    python tools/gal_bench.py [--out profiles/gal_bench.json] [--steps 2048]
    python tools/gal_bench.py --reference PATH --cpu-only      # the reference's CPU seconds per sample (no GPU)

(L, D) in {(8, 64), (16, 256), (32, 1034), (1034, 1034)} at 1, 1024 and 3072 streams.  Times are device events around
`reps` launches after a warm-up launch.  The CPU figures (one core, the reference's own GAL_JPE on 256 samples) are kept in
the same JSON file under "reference_cpu_s_per_sample" when it already holds them."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SHAPES = [(8, 64), (16, 256), (32, 1034), (1034, 1034)]
STREAMS = [1, 1024, 3072]


def cpu(reference, out):
    sys.path.insert(0, reference)
    from passiveRadar.clutter_removal import GAL_JPE
    rng = np.random.default_rng(1)
    res = {}
    for L, D in SHAPES:
        n = 256 + 11
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        t0 = time.perf_counter()
        GAL_JPE(x, x, L, D, 1e-3, 1e-2)
        res[f"{L}x{D}"] = (time.perf_counter() - t0) / 256
        print(L, D, res[f"{L}x{D}"], flush=True)
    data = json.load(open(out)) if os.path.exists(out) else {}
    data["reference_cpu_s_per_sample"] = res
    json.dump(data, open(out, "w"), indent=1)


def gpu(out, steps, reps):
    import torch
    from passiveradar_amd import engine, _lib
    _lib.require_gpu()
    rows = []
    for L, D in SHAPES:
        for ns in STREAMS:
            n = steps + 11
            g = torch.Generator(device="cuda").manual_seed(ns + D)
            ref = torch.randn(ns, n, dtype=torch.complex64, device="cuda", generator=g)
            srv = torch.randn(ns, n, dtype=torch.complex64, device="cuda", generator=g)
            o = torch.empty_like(srv)
            st = _lib.torch_stream_ptr()
            timed = {}
            for name, fn in (("gal", lambda: engine.gal_execute(ref, srv, o, n, L, D, 1e-3, 1e-2, 10, None, None, ns,
                                                                 stream=st)),
                             ("nlms", lambda: engine.nlms_execute(ref, srv, o, n, D - 10, 1e-2, 10, None, None, ns,
                                                                  stream=st))):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
                nst = (n - 11) if name == "gal" else (n - D)
                timed[name] = ms * 1e6 / nst
            row = {"L": L, "D": D, "streams": ns, "steps": steps, "gal_ns_per_step": round(timed["gal"], 1),
                   "nlms_ns_per_step_same_D": round(timed["nlms"], 1),
                   "gal_ns_per_step_per_stream": round(timed["gal"] / ns, 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del ref, srv, o
    data = json.load(open(out)) if os.path.exists(out) else {}
    data.update({"device": torch.cuda.get_device_name(), "rows": rows})
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(data, open(out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gal_bench.json"))
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    if a.reference:
        cpu(a.reference, a.out)
    if not a.cpu_only:
        gpu(a.out, a.steps, a.reps)
