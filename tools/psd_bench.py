"""Times the Welch spectra on one MI355X.

(a) the four spectra of ``spectral.preview`` at the shipped configuration's ``input_chunk_length`` (4 799 250 int8
    scalars per channel): two 8192-point spectra of the raw int8 channels and two 2048-point spectra of the tuned and
    resampled complex64 channels (13/119 of the samples), HIP events around the ``psd`` calls on device tensors.
(b) one waterfall: ``specgram(nfft 8192, navg 64, noverlap 0)`` of an int8 recording generated on the device, as much of
    600 s at 2.4 MS/s as fits in HBM (all of it: 2.88 GB).

Each time is given in ms and as a share of the DERIVED floor, the larger of: bytes that must move once (input read once
at noverlap 0, output written once) at the 6.29 TB/s copy ceiling, and 5 N log2 N flops per segment at the ~100 TFLOP/s
packed fp32 sustains.  The NumPy time of the same arithmetic (float32 window, complex64 FFT, float64
mean) on one core of the host the tool runs on goes in the same file; for (b) it is timed on ``--numpy-segments`` segments
and scaled.  Prints one JSON line.

    python tools/psd_bench.py [--seconds 600] [--reps 10] [--out profiles/psd_bench.json]
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
ICL = 4799250          # input_chunk_length of the shipped configuration (scalars per channel)
FS = 2.4e6


def floor_ms(nseg, nfft, in_bytes_per_sample, out_bytes):
    hbm = (nseg * nfft * in_bytes_per_sample + out_bytes) / (HBM_TB_S * 1e12) * 1e3
    flops = nseg * 5.0 * nfft * np.log2(nfft) / (FP32_TFLOPS * 1e12) * 1e3
    return dict(hbm_ms=round(hbm, 5), butterfly_ms=round(flops, 5), floor_ms=round(max(hbm, flops), 5))


def numpy_welch_ms(x, nfft, navg):
    """the same arithmetic in NumPy on one core: complex64 segments, float32 Hann, complex64 FFT, float64 mean of |X|^2"""
    w = np.hanning(nfft).astype(np.float32)
    nseg = x.shape[0] // nfft
    t0 = time.perf_counter()
    seg = x[:nseg * nfft].reshape(nseg, nfft) * w
    X = np.fft.fft(seg, axis=1)
    p = X.real.astype(np.float64) ** 2 + X.imag.astype(np.float64) ** 2
    k = nseg if navg == 0 else navg
    rows = np.roll(p[:(nseg // k) * k].reshape(nseg // k, k, nfft).mean(axis=1), -nfft // 2, axis=1)
    dt = (time.perf_counter() - t0) * 1e3
    assert rows.shape[1] == nfft
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0, help="length of the waterfall's recording")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy-segments", type=int, default=2048)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.spectral import psd, specgram
    _lib.require_gpu()
    out = dict(tool="psd_bench", reps=args.reps, hbm_tb_s=HBM_TB_S, fp32_tflops=FP32_TFLOPS)

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

    gen = torch.Generator(device="cuda").manual_seed(1234)
    # (a) the four spectra of preview
    n_in = ICL // 2
    n_ch = -(-n_in * 13 // 119)
    raw = [torch.randint(-40, 41, (ICL,), generator=gen, device="cuda", dtype=torch.int8) for _ in range(2)]
    ch = [torch.view_as_complex(torch.randn((n_ch, 2), generator=gen, device="cuda", dtype=torch.float32)) for _ in range(2)]

    def four():
        for r in raw:
            psd(r, NFFT=8192, Fs=FS, raw=True)
        for c in ch:
            psd(c, NFFT=2048, Fs=2e5)

    t_in = timed(lambda: psd(raw[0], NFFT=8192, Fs=FS, raw=True))
    t_ch = timed(lambda: psd(ch[0], NFFT=2048, Fs=2e5))
    t_four = timed(four)
    f_in = floor_ms(n_in // 8192, 8192, 2, 8 * 8192)
    f_ch = floor_ms(n_ch // 2048, 2048, 8, 8 * 2048)
    f_four = 2 * f_in["floor_ms"] + 2 * f_ch["floor_ms"]
    host_in = raw[0].cpu().numpy()
    host_in = (host_in[0::2].astype(np.float32) + 1j * host_in[1::2].astype(np.float32)).astype(np.complex64)
    host_ch = ch[0].cpu().numpy()
    out["preview_spectra"] = dict(
        input_chunk_length=ICL, input_segments=n_in // 8192, channel_samples=n_ch, channel_segments=n_ch // 2048,
        input_psd_ms=round(t_in, 4), input_psd_floor=f_in, input_psd_share_of_floor=round(f_in["floor_ms"] / t_in, 4),
        channel_psd_ms=round(t_ch, 4), channel_psd_floor=f_ch, channel_psd_share_of_floor=round(f_ch["floor_ms"] / t_ch, 4),
        four_spectra_ms=round(t_four, 4), four_spectra_floor_ms=round(f_four, 5),
        four_spectra_share_of_floor=round(f_four / t_four, 4),
        numpy_one_core_ms=round(2 * numpy_welch_ms(host_in, 8192, 0) + 2 * numpy_welch_ms(host_ch, 2048, 0), 2))
    del raw, ch

    # (b) the waterfall of a whole recording
    free, _ = _lib.mem_info()
    n = int(args.seconds * FS)
    n = min(n, int(free * 0.5) // 2)
    nseg = n // 8192
    rows = nseg // 64
    rec = torch.empty((2 * n,), device="cuda", dtype=torch.int8)
    piece = 1 << 28
    for s in range(0, 2 * n, piece):                          # generated on the device, in pieces
        e = min(2 * n, s + piece)
        rec[s:e] = torch.randint(-40, 41, (e - s,), generator=gen, device="cuda", dtype=torch.int8)
    t_wf = timed(lambda: specgram(rec, NFFT=8192, Fs=FS, noverlap=0, navg=64, raw=True))
    f_wf = floor_ms(rows * 64, 8192, 2, rows * 8 * 8192)
    m = min(args.numpy_segments, nseg)
    h = rec[:2 * m * 8192].cpu().numpy()
    h = (h[0::2].astype(np.float32) + 1j * h[1::2].astype(np.float32)).astype(np.complex64)
    t_np = numpy_welch_ms(h, 8192, 64) * (rows * 64) / m
    out["waterfall"] = dict(seconds=round(n / FS, 2), samples=n, segments=rows * 64, rows=rows, nfft=8192, navg=64,
                            ms=round(t_wf, 3), floor=f_wf, share_of_floor=round(f_wf["floor_ms"] / t_wf, 4),
                            input_gb_s=round(2 * rows * 64 * 8192 / t_wf / 1e6, 1),
                            numpy_one_core_ms_scaled=round(t_np, 1), numpy_segments_timed=m)
    out["device"] = torch.cuda.get_device_name(0)
    out["numpy"] = np.__version__
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
