"""Times the map fusion (target_detection.fuse_maps, prc_fuse) on one MI355X.

The published stack's shape: 1199 frames of 1024 Doppler rows x 177 range columns per illuminator (125 m range columns,
+-256 Hz over the rows, wavelength 3 m: the config-2 geometry tools/tbd_bench.py uses), K illuminators on a ring of 12 .. 30 km
around the receiver, a grid of 256 x 256 position cells of 50 m at 3 km height and 33 x 33 velocity hypotheses of 15 m/s
(+-240 m/s).  Shapes timed: K = 4 with 33 x 33 and with 9 x 9 hypotheses, K = 2 and K = 8 with 33 x 33.  The maps are
|N(0, 1)| generated on the device from a seed (the time does not depend on the values: no branch reads them).
Per shape, each form on its own (1 = gathers from global memory, 2 = gathers from LDS where a tile's bands fit), warm, device
events around the call on preallocated buffers, median of --reps; the two forms' outputs are compared bit for bit; the share
of tiles whose bands fit the LDS is counted on the host from the same geometry.  No time here is a threshold.

Reported against: the NumPy oracle (tests/fuse_oracle.py) on one core for ONE frame of a 32 x 32 grid, K = 4, 33 x 33
hypotheses (scaled to the full shape by the ratio of gathers); the DERIVED floor of the LDS gathers -- one ds_read_b32 lane
per (frame, cell, hypothesis, illuminator) at the 75 TB/s all CUs reach with that instruction; and the HBM floor of one read
of the stacks at the 6.29 TB/s copy ceiling DESIGN.md uses.  Prints one JSON line.

    python tools/fuse_bench.py [--reps 3] [--frames 1199] [--grid 256] [--commit ID] [--out profiles/fuse_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

COPY_CEILING_TBS = 6.29
LDS_B32_TBS = 75.0          # ds_read_b32, every CU streaming


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", REPO, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def scene(K, H, W):
    """K illuminators on a ring, the axes of the published frame: 125 m columns (col = W - 1 - excess / 125), 0.5 Hz rows"""
    rx = (0.0, 0.0, 10.0)
    axes = (float(W - 1), -1.0 / 125.0, H / 2.0, -H / 512.0)
    il = []
    for k in range(K):
        ang, dist = 2.0 * np.pi * (k + 0.3) / K, 12000.0 + 18000.0 * ((5 * k) % 8) / 7.0
        il.append(((float(dist * np.cos(ang)), float(dist * np.sin(ang)), 150.0 + 25.0 * k), 3.0, axes))
    return rx, il


def staged_share(FO, il, rx, grid, z, H, W, lds_floats, tile=8):
    """share of the tiles whose K bands fit the LDS, and the mean band width, from the columns the oracle computes"""
    _, col = FO.cells(FO.illum_rows(il, rx), rx, grid, (0.0, 0.0, 1, 0.0, 0.0, 1), z)
    K, ny, nx = col.shape
    fit, widths = 0, []
    tiles = 0
    for ty in range(0, ny, tile):
        for tx in range(0, nx, tile):
            need = 0
            for k in range(K):
                c = col[k, ty:ty + tile, tx:tx + tile]
                c = c[(c >= 0) & (c <= W - 1)]
                bw = int(c.max() - c.min() + 1) if c.size else 0
                widths.append(bw)
                need += H * bw
            tiles += 1
            fit += need <= lds_floats
    return round(fit / tiles, 4), round(float(np.mean(widths)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1199)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--commit", default=None, help="commit id to record (default: git rev-parse HEAD of this tree)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch
    import fuse_oracle as FO
    from passiveradar_amd import _lib, engine
    _lib.require_gpu()
    N, H, W, G = args.frames, 1024, 177, args.grid
    z = 3000.0
    grid = (-25.0 * G, 50.0, G, -25.0 * G, 50.0, G)
    vel33, vel9 = (-240.0, 15.0, 33, -240.0, 15.0, 33), (-240.0, 60.0, 9, -240.0, 60.0, 9)
    lds_floats = (_lib.FUSE_LDS_BYTES - 2048) // 4
    out = dict(tool="fuse_bench", commit=args.commit or commit_id(), reps=args.reps, frames=N, H=H, W=W, grid=[G, G], cell_m=50.0,
               data="|N(0, 1)| float32 maps, seed 27; illuminators on a ring of 12 .. 30 km, wavelength 3 m, 125 m columns, 0.5 Hz rows",
               device=torch.cuda.get_device_name(0))

    # the oracle on one core: one frame, a 32 x 32 grid, K = 4, 33 x 33 hypotheses
    rx, il4 = scene(4, H, W)
    og = (-800.0, 50.0, 32, -800.0, 50.0, 32)
    ostat = np.abs(np.random.default_rng(27).standard_normal((4, 1, H, W))).astype(np.float32)
    rows4 = FO.illum_rows(il4, rx)
    t0 = time.perf_counter()
    obest, ovel = FO.fuse(ostat, rows4, rx, og, vel33, z)
    t_oracle = time.perf_counter() - t0
    from passiveradar_amd.target_detection import fuse_maps
    gbest, gvel = fuse_maps(ostat, il4, rx, og, vel33, z)
    out["numpy_oracle"] = dict(grid=[32, 32], frames=1, K=4, hypotheses=33 * 33, seconds=round(t_oracle, 3),
                               gathers=32 * 32 * 33 * 33 * 4, device_equals_oracle=bool(np.array_equal(gbest, obest) and np.array_equal(gvel, ovel)))

    def stats(ts):
        return dict(ms_median=round(float(np.median(ts)), 3), ms_min=round(float(np.min(ts)), 3), ms_max=round(float(np.max(ts)), 3))

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
        return stats(ts)

    gen = torch.Generator(device="cuda").manual_seed(27)
    stat = torch.empty((8, N, H, W), dtype=torch.float32, device="cuda")
    for k in range(8):
        stat[k] = torch.randn((N, H, W), generator=gen, device="cuda").abs_()
    best = torch.zeros((N, G, G), dtype=torch.float32, device="cuda")
    vel = torch.zeros((N, G, G), dtype=torch.int32, device="cuda")
    st = _lib.torch_stream_ptr()
    runs = []
    for K, vels in ((4, vel33), (4, vel9), (2, vel33), (8, vel33)):
        rx, il = scene(K, H, W)
        rows = FO.illum_rows(il, rx)
        nv = vels[2] * vels[5]
        gathers = N * G * G * nv * K
        tile = 8 if K <= 4 else 4                    # the LDS form's tile edge (fuse.hip)
        share, bw = staged_share(FO, il, rx, grid, z, H, W, lds_floats, tile)
        r = dict(K=K, hypotheses=[vels[2], vels[5]], gathers=gathers, lds_tile=[tile, tile], tiles_staged_share=share, mean_band_columns=bw,
                 floor_lds_gathers_ms=round(gathers * 4 / (LDS_B32_TBS * 1e12) * 1e3, 3),
                 floor_hbm_one_read_ms=round(K * N * H * W * 4 / (COPY_CEILING_TBS * 1e12) * 1e3, 3),
                 numpy_oracle_scaled_s=round(t_oracle * gathers / (32 * 32 * 33 * 33 * 4), 1))
        ref = None
        for form, name in ((_lib.FUSE_FORM_GLOBAL, "global"), (_lib.FUSE_FORM_LDS, "lds"), (_lib.FUSE_FORM_AUTO, "shipped")):
            d = engine.fuse_desc(K, H, W, grid, vels, rx, z, _lib.FUSE_SUM, form)
            r[name] = timed(lambda: engine.fuse_execute(d, rows, stat, N * H * W, H * W, N, best, vel, st))
            if ref is None:
                ref = (best.view(torch.int32).clone(), vel.clone())
            r[name]["same_bytes_as_global"] = bool(torch.equal(best.view(torch.int32), ref[0]) and torch.equal(vel, ref[1]))
        r["lds_over_floor"] = round(r["lds"]["ms_median"] / max(r["floor_lds_gathers_ms"], r["floor_hbm_one_read_ms"]), 2)
        runs.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    out["prc_fuse"] = runs
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
