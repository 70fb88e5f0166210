"""prc_fuse of include/prcore.h in NumPy, operation for operation: float64 geometry with every operation rounded on its own
(NumPy never fuses), the sample test in float64, the combine in float32, the reduction over ascending j with strict greater.
Plus the design scene of DESIGN.md section 27 that the host tests, the GPU tests and smoke() share."""
import numpy as np

SUM, MIN = 0, 1
C0 = 299792458.0


def baseline(tx, rx):
    a = [np.float64(tx[i]) - np.float64(rx[i]) for i in range(3)]
    return float(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))


def illum_rows(illuminators, rx):
    """[K, 9] float64: tx[3], wavelength, baseline, col0, col_per_m, row0, row_per_hz from (tx, wavelength, axes) triples"""
    return np.array([[*map(float, tx), float(lam), baseline(tx, rx), *map(float, axes)] for tx, lam, axes in illuminators],
                    dtype=np.float64).reshape(-1, 9)


def cells(illum, rx, grid, velocities, z):
    """(row, col) in float64, [K, ny, nx, nv] and [K, ny, nx], before any range test"""
    x0, dx, nx, y0, dy, ny = grid
    vx0, dvx, nvx, vy0, dvy, nvy = velocities
    f8 = np.float64
    px = (f8(x0) + np.arange(nx, dtype=f8) * f8(dx))[None, :] + np.zeros((ny, 1))
    py = (f8(y0) + np.arange(ny, dtype=f8) * f8(dy))[:, None] + np.zeros((1, nx))
    pz = np.full((ny, nx), f8(z))
    j = np.arange(nvx * nvy)
    vx = f8(vx0) + (j % nvx).astype(f8) * f8(dvx)
    vy = f8(vy0) + (j // nvx).astype(f8) * f8(dvy)

    def dist(ax, ay, az):
        return np.sqrt((ax * ax + ay * ay) + az * az)

    def quot(a, d):
        return np.where(d == 0.0, 0.0, a / np.where(d == 0.0, 1.0, d))

    rxx, rxy, rxz = px - f8(rx[0]), py - f8(rx[1]), pz - f8(rx[2])
    dr = dist(rxx, rxy, rxz)
    rows, cols = [], []
    with np.errstate(all="ignore"):
        for p in np.asarray(illum, dtype=f8).reshape(-1, 9):
            tx, ty, tz = px - p[0], py - p[1], pz - p[2]
            dt = dist(tx, ty, tz)
            cols.append(np.rint(p[5] + ((dt + dr) - p[4]) * p[6]))
            gx = (quot(tx, dt) + quot(rxx, dr)) / p[3]
            gy = (quot(ty, dt) + quot(rxy, dr)) / p[3]
            f = -(gx[:, :, None] * vx + gy[:, :, None] * vy)
            rows.append(np.rint(p[7] + f * p[8]))
    return np.stack(rows), np.stack(cols)


def fuse(stat, illum, rx, grid, velocities, z=0.0, combine=SUM):
    """stat [K, nframes, H, W] float32 -> best float32, vel int32 [nframes, ny, nx]"""
    stat = np.asarray(stat, dtype=np.float32)
    K, nframes, H, W = stat.shape
    row, col = cells(illum, rx, grid, velocities, z)
    col = np.broadcast_to(col[:, :, :, None], row.shape)
    with np.errstate(invalid="ignore"):
        hit = (row >= 0) & (row <= H - 1) & (col >= 0) & (col <= W - 1)          # float64 compares: a NaN misses
    r = np.where(hit, row, 0).astype(np.int64)
    c = np.where(hit, col, 0).astype(np.int64)
    S = None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            s = np.where(hit[k][None], stat[k][:, r[k], c[k]], np.float32(0.0)).astype(np.float32)   # [nframes, ny, nx, nv]
            if S is None:
                S = s
            elif combine == SUM:
                S = (S + s).astype(np.float32)
            else:
                S = np.where(s < S, s, S)
    key = np.where(np.isnan(S), -np.inf, S).astype(np.float32)
    vel = np.argmax(key, axis=-1).astype(np.int32)                                # the first, i.e. lowest, j of the maximum
    best = np.take_along_axis(key, vel[..., None].astype(np.int64), axis=-1)[..., 0]
    vel[best == -np.inf] = -1                                                      # nothing was > -Inf
    return best, vel


def cell_of(position, velocity, illum_row, rx):
    """the forward model for one target: (row, col) as integers, not clipped"""
    grid = (position[0], 0.0, 1, position[1], 0.0, 1)
    vels = (velocity[0], 0.0, 1, velocity[1], 0.0, 1)
    row, col = cells(np.asarray(illum_row).reshape(1, 9), rx, grid, vels, position[2])
    return int(row[0, 0, 0, 0]), int(col[0, 0, 0])


# ---- the design scene: R = 63, F = 32, n = 12000, fs = 240 kHz (H x W = 32 x 64), three illuminators, two targets ----------
R, F, N, FS = 63, 32, 12000, 240e3
H, W = F, R + 1
RX = (0.0, 0.0, 10.0)
TXS = ((-30000.0, 5000.0, 300.0), (20000.0, 25000.0, 200.0), (10000.0, -28000.0, 250.0))
LAM = 3.0
AXES = (float(R), -FS / C0, F / 2.0, -N / FS)                                      # bistatic_axes(R, F, N, FS)
GRID = (-16000.0, 2000.0, 17, -12000.0, 2000.0, 13)
VELS = (-200.0, 50.0, 9, -200.0, 50.0, 9)
Z = 3000.0
TARGET_A = ((6000.0, 4000.0, Z), (150.0, -100.0))                                  # cell (iy, ix) = (8, 11), j = 2 * 9 + 7 = 25
TARGET_B = ((-8000.0, -6000.0, Z), (-50.0, 200.0))                                 # cell (3, 4), j = 8 * 9 + 3 = 75
CELL_A, VEL_A, CELL_B, VEL_B = (8, 11), 25, (3, 4), 75


def design_illuminators():
    return [(tx, LAM, AXES) for tx in TXS]


def design_maps(targets, noise_seed=None, amplitude=1.0, nframes=1):
    """[3, nframes, H, W] float32: zeros (or seeded |N(0, 1)|) with ``amplitude`` added at every target's cell in every map"""
    if noise_seed is None:
        stat = np.zeros((len(TXS), nframes, H, W), np.float32)
    else:
        stat = np.abs(np.random.default_rng(noise_seed).standard_normal((len(TXS), nframes, H, W))).astype(np.float32)
    rows = illum_rows(design_illuminators(), RX)
    for pos, v in targets:
        for k in range(len(TXS)):
            r, c = cell_of(pos, v, rows[k], RX)
            assert 0 <= r < H and 0 <= c < W, (k, r, c)
            stat[k, :, r, c] += np.float32(amplitude)
    return stat


def random_case(seed, K, H, W, ny, nx, nvx, nvy, nframes, col_sign=None, row_sign=None):
    """seeded geometry whose columns span about [-0.2 W, 1.2 W] and whose rows span about [-0.2 H, 1.2 H] over the grid and
    the hypotheses (some of both fall off either end of the map), with |N(0, 1)| maps"""
    rng = np.random.default_rng(seed)
    rx = (0.0, 0.0, 10.0)
    grid = (float(rng.uniform(-9000, -3000)), float(rng.uniform(300, 900)), nx, float(rng.uniform(-9000, -3000)),
            float(rng.uniform(300, 900)), ny)
    vels = (float(rng.uniform(-300, -100)), float(rng.uniform(20, 60)), nvx, float(rng.uniform(-300, -100)),
            float(rng.uniform(20, 60)), nvy)
    z = float(rng.uniform(500, 4000))
    il = []
    for k in range(K):
        tx = tuple(float(v) for v in (*rng.uniform(-30000, 30000, 2), rng.uniform(50, 400)))
        lam = float(rng.uniform(0.5, 3.0))
        # the excess range and the Doppler this illuminator sees over the grid: unit axes first
        row, col = cells(illum_rows([(tx, lam, (0.0, 1.0, 0.0, 1.0))], rx), rx, grid, vels, z)
        cs = (col_sign or (1, -1)[int(rng.integers(2))]) * 1.4 * W / (col.max() - col.min() + 1.0)
        rs = (row_sign or (1, -1)[int(rng.integers(2))]) * 1.4 * H / (row.max() - row.min() + 1.0)
        il.append((tx, lam, (W / 2 - cs * 0.5 * (col.max() + col.min()), cs, H / 2 - rs * 0.5 * (row.max() + row.min()), rs)))
    stat = np.abs(rng.standard_normal((K, nframes, H, W))).astype(np.float32)
    return stat, il, rx, grid, vels, z
