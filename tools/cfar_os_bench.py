"""Times the order-statistic CFAR (target_detection.CFAR_2D_OS, prc_cfar_os) on one MI355X.

The published stack's shape: 1199 frames of 1024 Doppler rows x 177 range columns at CFAR_2D's (18, 4) window, rank 225 of
299, Rayleigh magnitudes of unit-power complex Gaussian noise (seeded, generated on the device).  Recorded, in one run on one
box: prc_cfar_os on float32 magnitudes and on the complex64 maps (both scales), prc_cfar2d / prc_cfar2d_c64 on the same
data, and track_maps(..., cfar="os") next to cfar="mean".  No time here is a threshold.

The DERIVED floor.  The kernel selects by narrowing a key interval (interpolated pivots, then midpoints): a counting sweep costs one compare and one
add-with-carry per (cell, training value), a closing sweep an xor, a subtract and a minimum.  A wavefront (4 rows x 64
columns) sweeps until its slowest cell is done.  ``emulate`` below runs the kernel's own loop in NumPy on a crop of the
first frame -- its selected values are checked against the device's noise map, so the count belongs to the code that was
timed -- and gives the mean number of sweeps per wavefront.  Floor = wavefronts x VALU instructions per wavefront x 2 cycles
(a wave64 VALU instruction on a CDNA4 SIMD-32 with another wave to overlap) / (1024 SIMDs x 2.4 GHz).
The LDS traffic of a sweep (18 rows x 6 ds_read_b128 per wavefront) is about a third of what the LDS array sustains in that
time, so the VALU count is the bound.  Prints one JSON line.

    python tools/cfar_os_bench.py [--reps 5] [--frames 1199] [--chain-frames 1199] [--out profiles/cfar_os_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SIMDS, GHZ, VALU_CYCLES = 1024, 2.4, 2.0     # 256 CUs x 4 SIMD-32; cycles per wave64 VALU instruction with waves to overlap
TILE_ROWS, TILE_COLS, WAVE_ROWS = 16, 64, 4  # CO_TY, CO_TX, rows of a wavefront (cfar_os.hip)
INTERP_STEPS = 12                            # CO_INTERP_STEPS
COUNT_OPS, CLOSE_OPS = 2, 3                  # VALU instructions per (cell, training value) of a counting / closing sweep


def float_keys(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)


def unkey(k):
    k = k.astype(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def emulate(X, fw, gw, rank):
    """cfar_os_kernel's selection loop on one float32 frame: (z, counting sweeps per wavefront, closing sweep per wavefront)"""
    import cfar_os_oracle as OS
    X = np.ascontiguousarray(X, dtype=np.float32)
    H, W = X.shape
    c = OS.window(fw, gw)[0]
    K = float_keys(X)
    S = np.stack([np.roll(K, (-(c - a), -(c - b)), axis=(0, 1)) for a, b in OS.taps(fw, gw)])
    nt, k = S.shape[0], int(rank)
    lo, hm = np.empty((H, W), np.int64), np.empty((H, W), np.int64)
    for i0 in range(0, H, TILE_ROWS):
        for j0 in range(0, W, TILE_COLS):
            rows = (i0 + c - (fw - 1) + np.arange(TILE_ROWS + fw - 1)) % H
            cols = (j0 + c - (fw - 1) + np.arange(TILE_COLS + fw - 1)) % W
            t = K[np.ix_(rows, cols)]
            lo[i0:i0 + TILE_ROWS, j0:j0 + TILE_COLS], hm[i0:i0 + TILE_ROWS, j0:j0 + TILE_COLS] = t.min(), t.max()
    clo, chi = np.zeros((H, W), np.int64), np.full((H, W), nt, np.int64)
    steps, live = np.zeros((H, W), np.int64), np.ones((H, W), bool)
    for step in range(INTERP_STEPS + 33):
        live &= (lo != hm) & (clo != k - 1) & (chi != k)
        if not live.any():
            break
        w = hm - lo
        off = w >> 1
        if step < INTERP_STEPS:                  # the kernel's float32 guess, operation for operation
            fr = ((k - clo).astype(np.float32) - np.float32(0.5)) / (chi - clo).astype(np.float32)
            guess = np.minimum(fr * ((w - 1) & 0xffffffff).astype(np.float32), np.float32(4294967040.0))
            off = np.minimum(guess.astype(np.int64), (w - 1) & 0xffffffff)
        t = lo + off + 1
        cnt = (S < t).sum(0)
        acc, rej = live & (cnt <= k - 1), live & (cnt > k - 1)
        lo[acc], clo[acc] = t[acc], cnt[acc]
        hm[rej], chi[rej] = t[rej] - 1, cnt[rej]
        steps += live
    up = (clo == k - 1) | (lo == hm)
    big = np.int64(1) << 40
    ans = np.where(up, np.where(S >= lo, S, big).min(0), np.where(S <= hm, S, -big).max(0))
    z = unkey(ans) + np.float32(0)
    waves_count, waves_close = [], []
    for i0 in range(0, H, WAVE_ROWS):
        for j0 in range(0, W, TILE_COLS):
            waves_count.append(int(steps[i0:i0 + WAVE_ROWS, j0:j0 + TILE_COLS].max()))
            waves_close.append(bool((lo != hm)[i0:i0 + WAVE_ROWS, j0:j0 + TILE_COLS].any()))
    return z, np.array(waves_count), np.array(waves_close)


def floor_ms(nframes, H, W, nt, count_sweeps, close_sweeps):
    waves = nframes * -(-H // WAVE_ROWS) * -(-W // TILE_COLS)
    per_wave = 4 * nt * (COUNT_OPS * count_sweeps + CLOSE_OPS * close_sweeps)     # 4 outputs per thread
    return waves * per_wave * VALU_CYCLES / (SIMDS * GHZ * 1e9) * 1e3, waves, per_wave


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--chain-frames", type=int, default=1199)
    ap.add_argument("--crop-rows", type=int, default=64, help="rows of frame 0 the sweep count is emulated on")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.target_detection import CFAR_2D, CFAR_2D_OS, CFAR_2D_abs, track_maps
    _lib.require_gpu()
    N, H, W, fw, gw, rank = args.frames, 1024, 177, 18, 4, 225
    nt = engine.cfar_training_cells(fw, gw)
    gen = torch.Generator(device="cuda").manual_seed(18)
    xc = torch.complex(torch.randn((N, H, W), generator=gen, device="cuda"), torch.randn((N, H, W), generator=gen, device="cuda"))
    xc = (xc * (0.5 ** 0.5)).contiguous()
    xf = xc.abs().contiguous()
    out = dict(tool="cfar_os_bench", reps=args.reps, frames=N, H=H, W=W, fw=fw, gw=gw, rank=rank, training_cells=nt,
               data="unit-power complex Gaussian noise (Rayleigh magnitudes), seed 18")

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
        return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(float(np.min(ts)), 3), ms_max=round(float(np.max(ts)), 3))

    # the library calls on preallocated buffers: the kernels alone
    o = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    stream = _lib.torch_stream_ptr()
    for name, x, cplx in (("f32", xf, False), ("c64", xc, True)):
        for scale in ("reference", "plain"):
            d = engine.cfar_os_desc(H, W, fw, gw, rank, scale, cplx)
            nws = engine.cfar_os_workspace_bytes(d, N)
            ws = torch.empty(max(nws, 8), dtype=torch.uint8, device="cuda")
            out[f"prc_cfar_os_{name}_{scale}"] = timed(lambda: engine.cfar_os_execute(d, x, o, None, N, ws if nws else None, stream))
    out["prc_cfar2d_f32"] = timed(lambda: _lib.check(_lib.lib().prc_cfar2d(xf.data_ptr(), H, W, fw, gw, 0, 0.0, o.data_ptr(), N, stream)))
    out["prc_cfar2d_c64"] = timed(lambda: _lib.check(_lib.lib().prc_cfar2d_c64(xc.data_ptr(), H, W, fw, gw, 0, 0.0, o.data_ptr(), N, stream)))
    out["os_over_mean_f32"] = round(out["prc_cfar_os_f32_reference"]["ms_median"] / out["prc_cfar2d_f32"]["ms_median"], 2)

    # the sweep count of the timed algorithm, on a crop of frame 0 run as a frame of its own, checked against the device
    crop = xf[0, :args.crop_rows].contiguous()
    z_emu, wc, wz = emulate(crop.cpu().numpy(), fw, gw, rank)
    _, z_dev = CFAR_2D_OS(crop, fw, gw, rank=rank, scale="plain", return_noise=True)
    same = bool(np.array_equal(z_emu.view(np.uint32), z_dev.cpu().numpy().view(np.uint32)))
    fl, waves, per_wave = floor_ms(N, H, W, nt, float(wc.mean()), float(wz.mean()))
    full, _, _ = floor_ms(N, H, W, nt, 32.0, 0.0)
    t = out["prc_cfar_os_f32_plain"]["ms_median"]
    out["sweeps"] = dict(emulated_on=f"frame 0, rows 0..{args.crop_rows - 1}, as a {args.crop_rows} x {W} frame",
                         emulation_equals_device_noise_map=same, counting_sweeps_per_wavefront_mean=round(float(wc.mean()), 3),
                         counting_sweeps_per_wavefront_max=int(wc.max()), closing_sweeps_per_wavefront_mean=round(float(wz.mean()), 3),
                         valu_instructions_per_wavefront=round(per_wave, 1), wavefronts=waves)
    out["floor"] = dict(derived_from="VALU instructions: 2 per (cell, training value, counting sweep), 3 per closing sweep, 2 cycles each "
                                     "on 1024 SIMDs at 2.4 GHz", floor_ms=round(fl, 3), measured_ms=t,
                        floor_share=round(fl / t, 4), plain_32_sweep_bisection_floor_ms=round(full, 3))

    # the chain: CFAR -> get_measurements -> multitarget_tracker, wall clock, device tensor in, records out
    xs = xc[:args.chain_frames]

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 2)

    ext = [256.0, 177.0]
    reps = max(2, args.reps // 2)
    out["track_maps"] = dict(frames=int(xs.shape[0]), wall_ms_mean=wall(lambda: track_maps(xs, ext), reps),
                             wall_ms_os=wall(lambda: track_maps(xs, ext, cfar="os"), reps))
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
