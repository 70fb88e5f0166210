"""Times the polyphase filter bank (signal_utils.channelize) on one MI355X against its yardstick, K calls of
``channel_preprocessing`` on the same box and the same recording.

The workload is the int8 recording of DESIGN.md section 15 (600 s at 2.4 MS/s, 1.44e9 samples, 2.88 GB, generated on the
device; or as much as fits) at M = 12, D = 10 and at M = 24, D = 12, for K = 1, 2, 4, 8, 12 channels: HIP events around the
call on device tensors, median of ``--reps``.  Next to each figure stand the two DERIVED floors: the bytes that must move once,
(2 + 8 K / D) per int8 sample at the 6.29 TB/s copy ceiling, and 4 L + 8 M K flop per output time at the ~100 TFLOP/s packed
fp32 sustains.  Prints one JSON line.

    python tools/channelize_bench.py [--seconds 600] [--reps 10] [--out profiles/channelize_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_TB_S = 6.29        # MI355X copy ceiling (TB/s)
FP32_TFLOPS = 100.0    # packed fp32, sustained
FS = 2.4e6
CONFIGS = [(12, 10), (24, 12)]
KS = [1, 2, 4, 8, 12]


def floors(n, M, D, K):
    L = 20 * D + 1
    hbm = n * (2.0 + 8.0 * K / D) / (HBM_TB_S * 1e12) * 1e3
    vec = -(-n // D) * (4.0 * L + 8.0 * M * K) / (FP32_TFLOPS * 1e12) * 1e3
    return dict(hbm_ms=round(hbm, 4), vector_ms=round(vec, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0, help="length of the recording")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.signal_utils import channel_preprocessing, channelize
    _lib.require_gpu()

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
        return float(np.median(ts)), float(np.min(ts))

    gen = torch.Generator(device="cuda").manual_seed(1234)
    free, _ = _lib.mem_info()
    n = min(int(args.seconds * FS), int(free * 0.4) // 12)       # 2 n bytes in, at most 8 n * 12 / 10 out
    rec = torch.empty((2 * n,), device="cuda", dtype=torch.int8)
    piece = 1 << 28
    for s in range(0, 2 * n, piece):                              # generated on the device, in pieces
        e = min(2 * n, s + piece)
        rec[s:e] = torch.randint(-40, 41, (e - s,), generator=gen, device="cuda", dtype=torch.int8)

    out = dict(tool="channelize_bench", reps=args.reps, hbm_tb_s=HBM_TB_S, fp32_tflops=FP32_TFLOPS, seconds=round(n / FS, 2),
               samples=n, dtype="int8", fs=FS, runs=[])
    for M, D in CONFIGS:
        for K in KS:
            chans = [(5 * i + 1) % M for i in range(K)]           # distinct, spread over the band
            ms, best = timed(lambda: channelize(rec, M, D, chans))
            yard, yard_best = timed(lambda: [channel_preprocessing(rec, D, -k * FS / M, FS) for k in chans])
            fl = floors(n, M, D, K)
            out["runs"].append(dict(nchan=M, dec=D, K=K, channels=chans, ms=round(ms, 3), best_ms=round(best, 3),
                                    k_calls_of_channel_preprocessing_ms=round(yard, 3),
                                    k_calls_of_channel_preprocessing_best_ms=round(yard_best, 3),
                                    speedup=round(yard / ms, 3), floor=fl, share_of_hbm_floor=round(fl["hbm_ms"] / ms, 4),
                                    share_of_vector_floor=round(fl["vector_ms"] / ms, 4),
                                    input_gb_s=round(2.0 * n / ms / 1e6, 1)))
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
