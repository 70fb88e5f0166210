"""Times the FIR decimating front end on one MI355X.

(a) ``channel_preprocessing`` of an int8 recording generated on the device (600 s at 2.4 MS/s, 2.88 GB, or as much as fits)
    at ``dec`` = 10: one launch, HIP events around the call on a device tensor.
(b) the same recording through ``prc_fir_decimate`` with the rotation off (what the rotation costs).
(c) ``decimate`` of the complex64 stream of the same length (8 bytes per sample in).

Each time is given in ms and as a share of the two DERIVED floors: the bytes that must move once ((2 + 8 / q) per input
sample for (a) and (b), (8 + 8 / q) for (c)) at the 6.29 TB/s copy ceiling, and 4 (20 q + 1) flops per output at the ~100 TFLOP/s
packed fp32 sustains.  The reference's own arithmetic (deinterleave, float32 rotation,
scipy.signal.decimate(x, q, 20 q, ftype='fir')) is timed on one core of the host the tool runs on, on ``--numpy-seconds`` of
signal, and scaled.  Prints one JSON line.

    python tools/preproc_bench.py [--seconds 600] [--q 10] [--reps 10] [--out profiles/preproc_bench.json]
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
FP32_TFLOPS = 100.0    # packed fp32, sustained
FS = 2.4e6
FC = 1e5


def floors(n, q, in_bytes):
    hbm = n * (in_bytes + 8.0 / q) / (HBM_TB_S * 1e12) * 1e3
    vec = -(-n // q) * 4.0 * (20 * q + 1) / (FP32_TFLOPS * 1e12) * 1e3
    return dict(hbm_ms=round(hbm, 4), vector_ms=round(vec, 4))


def reference_ms(raw, q):
    """the reference's channel_preprocessing arithmetic on one core"""
    from scipy.signal import decimate
    t0 = time.perf_counter()
    z = (raw[0:-1:2] + 1j * raw[1::2]).astype(np.complex64)
    nn = np.arange(z.shape[0], dtype=np.complex64)
    z = z * np.exp(1j * 2 * np.pi * FC * nn / FS)
    y = decimate(z, q, 20 * q, ftype="fir", axis=0)
    dt = (time.perf_counter() - t0) * 1e3
    assert y.shape[0] == -(-z.shape[0] // q)
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0, help="length of the recording")
    ap.add_argument("--q", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.signal_utils import channel_preprocessing, decimate
    _lib.require_gpu()
    q = args.q
    out = dict(tool="preproc_bench", q=q, reps=args.reps, hbm_tb_s=HBM_TB_S, fp32_tflops=FP32_TFLOPS)

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
    n = min(int(args.seconds * FS), int(free * 0.4) // 10)       # (b) holds 8 n bytes in and 8 n / q out
    rec = torch.empty((2 * n,), device="cuda", dtype=torch.int8)
    piece = 1 << 28
    for s in range(0, 2 * n, piece):                              # generated on the device, in pieces
        e = min(2 * n, s + piece)
        rec[s:e] = torch.randint(-40, 41, (e - s,), generator=gen, device="cuda", dtype=torch.int8)

    def entry(ms, best, fl, in_bytes):
        return dict(ms=round(ms, 3), best_ms=round(best, 3), floor=fl, share_of_hbm_floor=round(fl["hbm_ms"] / ms, 4),
                    share_of_vector_floor=round(fl["vector_ms"] / ms, 4), input_gb_s=round(n * in_bytes / ms / 1e6, 1),
                    tflops=round(-(-n // q) * 4.0 * (20 * q + 1) / ms / 1e9, 2))

    ms, best = timed(lambda: channel_preprocessing(rec, q, FC, FS))
    host = rec[:2 * int(args.numpy_seconds * FS)].cpu().numpy()
    t_np = reference_ms(host, q)
    out["channel_preprocessing"] = dict(seconds=round(n / FS, 2), samples=n, dtype="int8", fc=FC, fs=FS,
                                        **entry(ms, best, floors(n, q, 2), 2),
                                        reference_one_core_ms_scaled=round(t_np * n / (host.shape[0] // 2), 1),
                                        reference_seconds_timed=args.numpy_seconds)
    # the same recording through prc_fir_decimate with the rotation off: what the rotation costs
    import ctypes as C
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix, d.fs = q, 20 * q + 1, _lib.RAW_DTYPES["int8"], 0, FS
    from scipy.signal import firwin
    taps = torch.from_numpy(firwin(20 * q + 1, 1.0 / q, window="hamming").astype(np.float32)).cuda()
    y = torch.empty((-(-n // q),), dtype=torch.complex64, device="cuda")
    ms, best = timed(lambda: _lib.check(_lib.lib().prc_fir_decimate(C.byref(d), taps.data_ptr(), rec.data_ptr(), n, 1, 0, 1,
                                                                    y.data_ptr(), 1, 0, _lib.torch_stream_ptr())))
    out["int8_no_rotation"] = dict(samples=n, dtype="int8", **entry(ms, best, floors(n, q, 2), 2))
    del rec, y
    z = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
    ms, best = timed(lambda: decimate(z, q))
    out["decimate"] = dict(samples=n, dtype="complex64", **entry(ms, best, floors(n, q, 8), 8))
    out["device"] = torch.cuda.get_device_name(0)
    out["numpy"] = np.__version__
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
