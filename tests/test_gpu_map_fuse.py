"""prc_fuse / fuse_maps / locate_maps on the device against tests/fuse_oracle.py: best and vel are EQUAL to the oracle
(np.array_equal) for both combines and every form, on the design scene with noise, on seeded random shapes (odd sizes, partial
and several tiles, geometry that throws columns and rows off the map at both ends, axes of either sign, a map too tall for the
LDS so that the tile falls back to global gathers), and on the edge cases of the definition."""
import numpy as np
import pytest

import fuse_oracle as FO

pytestmark = pytest.mark.gpu

FORMS = (None, 1, 2)
COMBINES = (("sum", FO.SUM), ("min", FO.MIN))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_all(stat, il, rx, grid, vels, z, forms=FORMS, expect_off_map=False):
    """every combine and form against the oracle, through fuse_maps on device tensors"""
    from passiveradar_amd.target_detection import fuse_maps
    rows = FO.illum_rows(il, rx)
    if expect_off_map:
        r, c = FO.cells(rows, rx, grid, vels, z)
        H, W = stat.shape[2:]
        assert (c < 0).any() and (c > W - 1).any() and (r < 0).any() and (r > H - 1).any()
    x = dev(stat)
    for name, code in COMBINES:
        want_best, want_vel = FO.fuse(stat, rows, rx, grid, vels, z, code)
        for form in forms:
            best, vel = fuse_maps(x, il, rx, grid, vels, z, combine=name, form=form)
            assert best.is_cuda and vel.is_cuda
            assert np.array_equal(best.cpu().numpy(), want_best), (name, form)
            assert np.array_equal(vel.cpu().numpy(), want_vel), (name, form)


def test_design_scene_with_noise(gpu_ready):
    """|N(0, 1)| maps with both targets added at 6.0: the oracle, bit for bit, and the targets stand out under both combines"""
    stat = FO.design_maps([FO.TARGET_A, FO.TARGET_B], noise_seed=11, amplitude=6.0, nframes=2)
    check_all(stat, FO.design_illuminators(), FO.RX, FO.GRID, FO.VELS, FO.Z)
    from passiveradar_amd.target_detection import fuse_maps
    for combine in ("sum", "min"):
        best, vel = fuse_maps(stat, FO.design_illuminators(), FO.RX, FO.GRID, FO.VELS, FO.Z, combine=combine)     # NumPy in, NumPy out
        assert isinstance(best, np.ndarray) and best.dtype == np.float32 and vel.dtype == np.int32
        for f in range(2):
            top = np.argsort(best[f].ravel())[-2:]
            assert sorted(top.tolist()) == sorted([FO.CELL_A[0] * 17 + FO.CELL_A[1], FO.CELL_B[0] * 17 + FO.CELL_B[1]])
            assert vel[f][FO.CELL_A] == FO.VEL_A and vel[f][FO.CELL_B] == FO.VEL_B


def test_design_scene_closed_form(gpu_ready):
    """the noise-free scene of the issue on the device: 3.0 at A and B alone, vel 25 and 75, one ghost at 2.0"""
    from passiveradar_amd.target_detection import fuse_maps
    stat = FO.design_maps([FO.TARGET_A, FO.TARGET_B])
    best, vel = fuse_maps(stat, FO.design_illuminators(), FO.RX, FO.GRID, FO.VELS, FO.Z)
    assert np.argwhere(best[0] == 3.0).tolist() == [list(FO.CELL_B), list(FO.CELL_A)]
    assert vel[0][FO.CELL_A] == FO.VEL_A and vel[0][FO.CELL_B] == FO.VEL_B and int((best[0] == 2.0).sum()) == 1


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("H,W", [(33, 19), (5, 130)])
def test_random_shapes(gpu_ready, K, H, W):
    """grids 1 x 1, 5 x 7 and 17 x 13 (one cell, a partial tile, 3 x 2 tiles with partial ones), 1, 15 and 81 hypotheses (fewer
    than, about and more than the lanes of a cell), 1 and 3 frames"""
    seed = 1000 * K + H
    for ny, nx in ((1, 1), (5, 7), (17, 13)):
        for nvx, nvy in ((1, 1), (3, 5), (9, 9)):
            for nframes in (1, 3):
                seed += 1
                case = FO.random_case(seed, K, H, W, ny, nx, nvx, nvy, nframes)
                check_all(*case, expect_off_map=(ny * nx * nvx * nvy >= 35 * 15))


@pytest.mark.parametrize("col_sign,row_sign", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
def test_axes_of_either_sign_and_cells_off_the_map(gpu_ready, col_sign, row_sign):
    case = FO.random_case(77, 3, 24, 40, 9, 10, 5, 4, 2, col_sign, row_sign)
    assert all(np.sign(il[2][1]) == col_sign and np.sign(il[2][3]) == row_sign for il in case[1])
    check_all(*case, expect_off_map=True)


def test_a_map_too_tall_for_the_lds_falls_back(gpu_ready):
    """700 rows and one tile that sees columns 3 .. 63: a band of 167 KiB, more than the 154 KiB the LDS form has: form 2
    gathers from global memory, the same bytes; the neighbouring shape, 560 rows of columns 0 .. 62 (138 KiB), is staged"""
    for H in (700, 560):
        case = FO.random_case(5 + H, 1, H, 64, 8, 8, 7, 3, 2)
        r, c = FO.cells(FO.illum_rows(case[1], case[2]), *case[2:])
        assert c.min() <= 0 and c.max() >= 63
        check_all(*case, forms=(2, 1))


def test_cells_on_the_receiver_and_on_a_transmitter(gpu_ready):
    """distance 0: the quotient is 0, not 0 / 0"""
    rx = (0.0, 0.0, 10.0)
    txs = ((2000.0, -1000.0, 10.0), (-2000.0, 1000.0, 10.0), (9000.0, 9000.0, 200.0))
    grid, vels, z = (-2000.0, 1000.0, 5, -2000.0, 1000.0, 4), (-120.0, 60.0, 5, -90.0, 45.0, 5), 10.0
    il = [(tx, 2.0, (20.0, -0.004, 12.0, -0.2)) for tx in txs]
    rows = FO.illum_rows(il, rx)
    x0, dx, nx, y0, dy, ny = grid
    nodes = {(x0 + i * dx, y0 + j * dy, z) for i in range(nx) for j in range(ny)}
    assert rx in nodes and txs[0] in nodes and txs[1] in nodes
    stat = np.abs(np.random.default_rng(3).standard_normal((3, 2, 24, 40))).astype(np.float32)
    r, c = FO.cells(rows, rx, grid, vels, z)
    assert np.isfinite(r).all() and np.isfinite(c).all() and ((r >= 0) & (r <= 23)).any()
    check_all(stat, il, rx, grid, vels, z)


def test_nan_and_inf_in_a_map(gpu_ready):
    """a NaN is never chosen and, under sum, poisons only its own hypothesis; +Inf is chosen"""
    stat, il, rx, grid, vels, z = FO.random_case(31, 3, 24, 40, 6, 9, 5, 5, 2)
    rows = FO.illum_rows(il, rx)
    r, c = FO.cells(rows, rx, grid, vels, z)
    H, W = stat.shape[2:]
    ok = (r >= 0) & (r <= H - 1) & (c[..., None] >= 0) & (c[..., None] <= W - 1)
    hits = np.argwhere(ok)
    pick = hits[np.random.default_rng(4).choice(len(hits), 24, replace=False)]
    for n, (k, iy, ix, j) in enumerate(pick):
        stat[k, n % 2, int(r[k, iy, ix, j]), int(c[k, iy, ix])] = (np.nan, np.inf, -np.inf)[n % 3]
    stat[0, 0, :, 5] = np.nan                                   # a whole column of illuminator 0: s_0 = NaN stays under min
    want, _ = FO.fuse(stat, rows, rx, grid, vels, z, FO.SUM)
    assert np.isinf(want).any() and not np.isnan(want).any()
    check_all(stat, il, rx, grid, vels, z)
    stat[:] = np.nan                                            # nothing can be chosen: (-Inf, -1) everywhere
    from passiveradar_amd.target_detection import fuse_maps
    best, vel = fuse_maps(stat[:1], il[:1], rx, (grid[0], grid[1], 1, grid[3], grid[4], 1), (0.0, 1.0, 1, 0.0, 1.0, 1), z)
    r1, c1 = FO.cells(rows[:1], rx, (grid[0], grid[1], 1, grid[3], grid[4], 1), (0.0, 1.0, 1, 0.0, 1.0, 1), z)
    if 0 <= r1[0, 0, 0, 0] <= H - 1 and 0 <= c1[0, 0, 0] <= W - 1:
        assert (best == -np.inf).all() and (vel == -1).all()
    else:
        assert (best == 0.0).all() and (vel == 0).all()


@pytest.mark.parametrize("form", FORMS)
def test_strides_larger_than_the_map_and_no_vel(gpu_ready, form):
    """illum_stride and frame_stride with gaps that hold a NaN sentinel (read, it would change a result); both stride orders;
    vel = NULL leaves best unchanged"""
    import torch
    from passiveradar_amd import _lib, engine
    stat, il, rx, grid, vels, z = FO.random_case(52, 3, 24, 40, 9, 10, 5, 4, 2)
    K, nf, H, W = stat.shape
    rows = FO.illum_rows(il, rx)
    want_best, want_vel = FO.fuse(stat, rows, rx, grid, vels, z, FO.SUM)
    d = engine.fuse_desc(K, H, W, grid, vels, rx, z, _lib.FUSE_SUM, form)
    st = _lib.torch_stream_ptr()
    HW = H * W
    for s_illum, s_frame in ((nf * (HW + 13) + 7, HW + 13), (HW + 5, K * (HW + 5) + 3)):
        buf = torch.full(((K - 1) * s_illum + (nf - 1) * s_frame + HW,), float("nan"), device="cuda")
        buf.as_strided((K, nf, HW), (s_illum, s_frame, 1)).copy_(dev(stat).reshape(K, nf, HW))
        best = torch.full(want_best.shape, -7.0, device="cuda")
        vel = torch.full(want_vel.shape, -7, dtype=torch.int32, device="cuda")
        engine.fuse_execute(d, rows, buf, s_illum, s_frame, nf, best, vel, st)
        assert np.array_equal(best.cpu().numpy(), want_best) and np.array_equal(vel.cpu().numpy(), want_vel)
        best2 = torch.full(want_best.shape, -7.0, device="cuda")
        engine.fuse_execute(d, rows, buf, s_illum, s_frame, nf, best2, None, st)
        assert torch.equal(best2, best)


def test_strided_device_tensors_are_read_in_place_or_copied(gpu_ready):
    """every view gives the result of its contiguous copy: a frame step of two and a [nframes, K] stack permuted (both read
    in place through the two strides), a column slice (copied), float64 maps (converted), a list of stacks"""
    import torch
    from passiveradar_amd.target_detection import fuse_maps
    stat, il, rx, grid, vels, z = FO.random_case(53, 3, 24, 40, 9, 10, 5, 4, 4)
    rows = FO.illum_rows(il, rx)
    x = dev(stat)

    def run(t, s):
        want = FO.fuse(s, rows, rx, grid, vels, z, FO.SUM)
        got = fuse_maps(t, il, rx, grid, vels, z)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])

    run(x[:, ::2], stat[:, ::2])
    run(x.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3), stat)
    wide = torch.zeros((3, 4, 24, 50), device="cuda")
    wide[..., 3:43] = x
    run(wide[..., 3:43], stat)
    run(x.double(), stat)
    run([x[0], x[1], x[2]], stat)
    assert fuse_maps(x, il, rx, grid, vels, z, return_vel=False)[1] is None


def test_device_tensors_stay_on_the_current_stream(gpu_ready):
    import torch
    from passiveradar_amd.target_detection import fuse_maps
    stat, il, rx, grid, vels, z = FO.random_case(54, 2, 33, 19, 17, 13, 9, 9, 3)
    want = FO.fuse(stat, FO.illum_rows(il, rx), rx, grid, vels, z, FO.MIN)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = dev(stat)
        x = x + 0.0                                             # produced on s: only a launch on s sees it in order
        best, vel = fuse_maps(x, il, rx, grid, vels, z, combine="min")
        assert best.device == x.device and vel.device == x.device and best.dtype == torch.float32 and vel.dtype == torch.int32
        out = (best.clone(), vel.clone())                       # consumed on s
    s.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("form", [1, 2])
def test_capture_and_replay(gpu_ready, form):
    """one launch, captured in a linear graph, replays to the same bytes (and to the new input's result)"""
    import torch
    from passiveradar_amd import _lib, engine
    stat, il, rx, grid, vels, z = FO.random_case(55, 3, 24, 40, 9, 10, 5, 4, 2)
    K, nf, H, W = stat.shape
    rows = FO.illum_rows(il, rx)
    d = engine.fuse_desc(K, H, W, grid, vels, rx, z, _lib.FUSE_SUM, form)
    x = dev(stat)
    best = torch.zeros((nf, 9, 10), device="cuda")
    vel = torch.zeros((nf, 9, 10), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm up: the LDS opt-in of the kernel is set once, outside the capture
        engine.fuse_execute(d, rows, x, nf * H * W, H * W, nf, best, vel, _lib.torch_stream_ptr())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = (best.clone(), vel.clone())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine.fuse_execute(d, rows, x, nf * H * W, H * W, nf, best, vel, _lib.torch_stream_ptr())
    for _ in range(2):
        best.fill_(-1.0)
        vel.fill_(-9)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(best, eager[0]) and torch.equal(vel, eager[1])
    stat2 = np.abs(np.random.default_rng(56).standard_normal(stat.shape)).astype(np.float32)
    x.copy_(dev(stat2))
    g.replay()
    torch.cuda.synchronize()
    want = FO.fuse(stat2, rows, rx, grid, vels, z, FO.SUM)
    assert np.array_equal(best.cpu().numpy(), want[0]) and np.array_equal(vel.cpu().numpy(), want[1])


@pytest.mark.parametrize("device_side", [True, False])
def test_locate_maps_finds_both_targets(gpu_ready, device_side):
    """the chain on the design scene: Rayleigh noise, both targets at 40 in every map, CFAR -> fusion -> peaks: A and B come
    first, with their velocities, in both frames; the third slot is a ghost below them or empty"""
    from passiveradar_amd.target_detection import locate_maps
    rng = np.random.default_rng(21)
    mag = FO.design_maps([FO.TARGET_A, FO.TARGET_B], amplitude=40.0, nframes=2)
    mag += np.abs(rng.standard_normal(mag.shape) + 1j * rng.standard_normal(mag.shape)).astype(np.float32) / np.float32(np.sqrt(2))
    stacks = [dev(m) for m in mag] if device_side else [np.moveaxis(m, 0, 2) for m in mag]
    pos, v, score = locate_maps(stacks, FO.design_illuminators(), FO.RX, FO.GRID, FO.VELS, FO.Z, fw=8, gw=2, thresh=30.0, npeaks=3)
    if device_side:
        assert pos.is_cuda and v.is_cuda and score.is_cuda
        pos, v, score = pos.cpu().numpy(), v.cpu().numpy(), score.cpu().numpy()
    assert pos.shape == (2, 3, 2) and v.shape == (2, 3, 2) and score.shape == (2, 3)
    want = sorted([(*FO.TARGET_A[0][:2], *FO.TARGET_A[1]), (*FO.TARGET_B[0][:2], *FO.TARGET_B[1])])
    for f in range(2):
        got = sorted((*pos[f, n], *v[f, n]) for n in range(2))
        assert got == want, (f, got)
        assert score[f, 0] >= score[f, 1] > 30.0 and score[f, 1] > score[f, 2]
