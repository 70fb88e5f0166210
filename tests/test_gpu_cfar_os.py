"""CFAR_2D_OS / prc_cfar_os on the MI355X against tests/cfar_os_oracle.py: the selection is exact (the noise map equals the
oracle's bit for bit), the plain ratio is the IEEE float32 quotient, the reference ratio holds the TIGHT bar of
tests/test_gpu_bounds.py; the scene the feature exists for; complex input; scale, dead air; placement; the chains; capture."""
import math

import numpy as np
import pytest

import cfar_os_oracle as OS
from conftest import rel_err
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TIGHT = 2e-5          # tests/test_gpu_bounds.py
SHAPES = [(5, 7), (16, 64), (17, 65), (33, 130)]      # multiple wrap at fw = 18; one tile; one past a tile; several tiles
WINDOWS = [(3, 1), (9, 2), (18, 4), (33, 6)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, any NaN standing for any other (the sign and payload of a 0/0 are not arithmetic)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def ranks_of(fw, gw):
    nt = OS.training_cells(fw, gw)
    return sorted({1, nt, math.ceil(nt / 2), OS.default_rank(fw, gw)})


def rayleigh(rng, shape):
    return np.abs(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.float32) * np.float32(math.sqrt(0.5))


def selection_inputs(shape, seed):
    """the four maps of the exact-selection test as a stack of four frames"""
    rng = np.random.default_rng(seed)
    signed = rng.standard_normal(shape).astype(np.float32)
    signed.flat[0], signed.flat[-1] = -0.0, 0.0
    return np.stack([rayleigh(rng, shape), rng.integers(0, 4, shape).astype(np.float32), np.full(shape, 2.5, np.float32), signed])


@pytest.mark.parametrize("fw,gw", WINDOWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_selection(gpu_ready, shape, fw, gw):
    """Rayleigh noise, a map quantised to {0, 1, 2, 3} (ties everywhere), a constant map and a signed Gaussian map (with a
    -0 and a +0), as one stack of four frames, at ranks 1, Nt, ceil(Nt / 2) and the default"""
    from passiveradar_amd.target_detection import CFAR_2D_OS
    X = selection_inputs(shape, 100 * fw + shape[0])
    want = [OS.noise_at_ranks(x, fw, gw, ranks_of(fw, gw)) for x in X]
    for k in ranks_of(fw, gw):
        plain, z = CFAR_2D_OS(X, fw, gw, rank=k, scale="plain", return_noise=True)
        ref = CFAR_2D_OS(X, fw, gw, rank=k)
        if k == OS.default_rank(fw, gw):
            assert np.array_equal(ref, CFAR_2D_OS(X, fw, gw), equal_nan=True)
        for f, x in enumerate(X):
            zw = want[f][k]
            assert zw.dtype == np.float32 and np.array_equal(bits(z[f]), bits(zw)), (shape, fw, gw, k, f)
            with np.errstate(divide="ignore", invalid="ignore"):
                assert same(plain[f], x / zw), (shape, fw, gw, k, f)
            e = rel_err(ref[f], OS.ratios(x, zw, "reference"))
            assert e < TIGHT, (shape, fw, gw, k, f, e)


def test_largest_window(gpu_ready):
    """fw = 90 is the last window whose tile fits LDS (105 rows of 156 keys); 91 is refused, not run"""
    from passiveradar_amd.target_detection import CFAR_2D_OS
    rng = np.random.default_rng(90)
    x = rayleigh(rng, (17, 65))
    _, z = CFAR_2D_OS(x, 90, 4, scale="plain", return_noise=True)
    assert np.array_equal(bits(z), bits(OS.noise(x, 90, 4)))
    with pytest.raises(NotImplementedError):
        CFAR_2D_OS(x, 91, 4)


def feature_scene():
    rng = np.random.default_rng(225)
    noise = ((rng.standard_normal((64, 96)) + 1j * rng.standard_normal((64, 96))) * math.sqrt(0.5)).astype(np.complex64)
    scene = noise.copy()
    ti, tj = 30, 40
    scene[ti, tj] += 6.0
    for di, dj in ((7, 0), (0, 8), (-6, -6), (8, -7), (-8, 3), (3, -8)):
        scene[ti + di, tj + dj] += 200.0
    return np.abs(noise), np.abs(scene), (ti, tj)


def test_interferers_in_the_window_mask_the_cell_average_not_the_order_statistic(gpu_ready):
    """64 x 96 unit-power Rayleigh noise, a target of amplitude 6 at (30, 40), six interferers of amplitude 200 inside its
    (18, 4) annulus.  Each detector is thresholded at its own 99.9th percentile on the noise-only frame (from the oracles):
    the order statistic (plain scale, rank 225) detects the target cell, the cell average does not."""
    from passiveradar_amd.target_detection import CFAR_2D, CFAR_2D_OS
    noise, scene, (ti, tj) = feature_scene()
    c, e1, e2 = OS.window(18, 4)
    for di, dj in ((7, 0), (0, 8), (-6, -6), (8, -7), (-8, 3), (3, -8)):
        a, b = c - di, c - dj                     # the tap that reads (ti + di, tj + dj)
        assert 0 <= a < 18 and 0 <= b < 18 and not (e1 <= a < e2 and e1 <= b < e2)
    thr_os = float(np.percentile(OS.CFAR_2D_OS(noise, 18, 4, rank=225, scale="plain"), 99.9))
    thr_ca = float(np.percentile(O.CFAR_2D(noise, 18, 4), 99.9))
    # the scene does what it is meant to on the CPU oracles
    assert OS.CFAR_2D_OS(scene, 18, 4, rank=225, scale="plain")[ti, tj] > thr_os and O.CFAR_2D(scene, 18, 4)[ti, tj] < thr_ca
    r_os = CFAR_2D_OS(scene, 18, 4, rank=225, scale="plain")
    hit = CFAR_2D_OS(scene, 18, 4, thr_os, rank=225, scale="plain")
    r_ca = CFAR_2D(scene, 18, 4)
    print(f"order statistic {r_os[ti, tj]:.3f} against {thr_os:.3f}; cell average {r_ca[ti, tj]:.3f} against {thr_ca:.3f}")
    assert hit.dtype == bool and hit[ti, tj] and r_os[ti, tj] > thr_os
    assert r_ca[ti, tj] < thr_ca and not CFAR_2D(scene, 18, 4, thr_ca)[ti, tj]


def ulps(a, b):
    """distance in float32 steps (both finite, same sign or zero)"""
    ka, kb = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return np.abs(ka - kb)


@pytest.mark.parametrize("shape", [(17, 65), (33, 130)])
def test_complex_input(gpu_ready, shape):
    """|X| = hypotf on the tile load is the only inexact step: z within 4 float32 ulps of the oracle on np.abs(X)
    (neighbouring order statistics lie about 1e-3 apart), the ratios within TIGHT"""
    from passiveradar_amd.target_detection import CFAR_2D_OS
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((3,) + shape) + 1j * rng.standard_normal((3,) + shape)).astype(np.complex64)
    for fw, gw in ((18, 4), (9, 2)):
        plain, z = CFAR_2D_OS(x, fw, gw, scale="plain", return_noise=True)
        ref, z2 = CFAR_2D_OS(dev(x), fw, gw, return_noise=True)
        assert np.array_equal(bits(z), bits(z2.cpu().numpy()))
        for f in range(3):
            mag = np.abs(x[f])
            zw = OS.noise(mag, fw, gw)
            assert mag.dtype == np.float32 and ulps(z[f], zw).max() <= 4, ulps(z[f], zw).max()
            assert rel_err(plain[f], OS.ratios(mag, zw, "plain")) < TIGHT
            assert rel_err(ref[f].cpu().numpy(), OS.ratios(mag, zw, "reference")) < TIGHT


def test_scale_and_dead_air(gpu_ready):
    from passiveradar_amd.target_detection import CFAR_2D_OS
    rng = np.random.default_rng(8)
    x = rayleigh(rng, (33, 130))
    p1, z1 = CFAR_2D_OS(x, 18, 4, scale="plain", return_noise=True)
    for e in (-50, 50):                           # 2^-50 = 8.9e-16, 2^50 = 1.1e15
        s = np.float32(2.0 ** e)
        ps, zs = CFAR_2D_OS(x * s, 18, 4, scale="plain", return_noise=True)
        assert np.array_equal(bits(ps), bits(p1)), e
        assert np.array_equal(bits(zs), bits(z1.astype(np.float32) * s)), e
        r = CFAR_2D_OS(x * s, 18, 4)
        assert rel_err(r, OS.CFAR_2D_OS(x * s, 18, 4)) < TIGHT, e
    zero = np.zeros((17, 65), np.float32)
    for scale in ("reference", "plain"):
        r, z = CFAR_2D_OS(zero, 18, 4, scale=scale, return_noise=True)
        assert np.isnan(r).all() and np.array_equal(bits(z), bits(zero)), scale
        assert not CFAR_2D_OS(zero, 18, 4, 0.0, scale=scale).any() and not CFAR_2D_OS(dev(zero), 18, 4, -1.0, scale=scale).any()
    live = rayleigh(rng, (64, 96))
    live[10:50, 20:70] = 0.0                      # a zero patch larger than the window: 0 / 0 inside it ...
    live[30, 45] = 3.0                            # ... and x / 0 at one live cell in its middle
    got, z = CFAR_2D_OS(live, 18, 4, scale="plain", return_noise=True)
    want = OS.CFAR_2D_OS(live, 18, 4, scale="plain")
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert same(got, live / OS.noise(live, 18, 4))
    assert not np.signbit(z).any()


def test_placement_and_front_ends(gpu_ready):
    """a frame alone == the frame at positions 0, 1 and 2 of a stack; NumPy in == torch in; thresholded == ratio > thresh"""
    from passiveradar_amd.target_detection import CFAR_2D_OS
    rng = np.random.default_rng(9)
    a, b, c = (rayleigh(rng, (17, 65)) * np.float32(s) for s in (1.0, 30.0, 0.01))
    for fw, gw in ((18, 4), (9, 2)):
        for scale in ("reference", "plain"):
            alone = CFAR_2D_OS(a, fw, gw, scale=scale, return_noise=True)
            for pos, stack in enumerate((np.stack([a, b, c]), np.stack([b, a, c]), np.stack([c, b, a]))):
                r, z = CFAR_2D_OS(stack, fw, gw, scale=scale, return_noise=True)
                assert np.array_equal(bits(r[pos]), bits(alone[0])) and np.array_equal(bits(z[pos]), bits(alone[1])), (fw, scale, pos)
                rt, zt = CFAR_2D_OS(dev(stack), fw, gw, scale=scale, return_noise=True)
                assert rt.is_cuda and str(rt.dtype) == "torch.float32" and str(zt.dtype) == "torch.float32"
                assert np.array_equal(bits(rt.cpu().numpy()), bits(r)) and np.array_equal(bits(zt.cpu().numpy()), bits(z))
            r = CFAR_2D_OS(a, fw, gw, scale=scale)
            thr = float(np.percentile(r, 90))
            hit = CFAR_2D_OS(a, fw, gw, thr, scale=scale)
            assert hit.dtype == bool and np.array_equal(hit, r.astype(np.float32) > np.float32(thr))
            hit_t = CFAR_2D_OS(dev(a), fw, gw, thr, scale=scale)
            assert str(hit_t.dtype) == "torch.bool" and np.array_equal(hit_t.cpu().numpy(), hit)


def chain_maps(seed, N, H, W):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))).astype(np.complex64)
    for t in range(N):
        x[t, 40 + t // 6, 20] += 30.0
        x[t, 44 + t // 6, 26] += 200.0            # a strong neighbour inside the first one's window
    return x


def test_chains(gpu_ready):
    """the cfar="os" chains == CFAR_2D_OS followed by the consumer, byte for byte; cfar="mean" == no keyword"""
    from passiveradar_amd.plotting_tools import persistence, render_frames, render_maps
    from passiveradar_amd.target_detection import (CFAR_2D_OS, multitarget_tracker, simple_target_tracker, simple_track_maps,
                                                   track_maps)
    N, H, W = 12, 96, 48
    x = chain_maps(31, N, H, W)
    xd, xs = dev(x), np.moveaxis(x, 0, 2)          # torch [N, H, W]; numpy (H, W, N) as the scripts load it
    mag = np.abs(x)
    ext = [100.0, 80.0]
    cf = CFAR_2D_OS(xd, 18, 4)
    want = multitarget_tracker(cf, ext, 10)
    assert track_maps(xd, ext, 10, cfar="os").tobytes() == want.tobytes()
    assert track_maps(xs, ext, 10, cfar="os").tobytes() == want.tobytes()
    assert multitarget_tracker(np.moveaxis(CFAR_2D_OS(x, 18, 4), 0, 2), ext, 10).tobytes() == want.tobytes()
    assert track_maps(np.moveaxis(mag, 0, 2), ext, 10, cfar="os").tobytes() == multitarget_tracker(CFAR_2D_OS(dev(mag), 18, 4), ext, 10).tobytes()
    assert track_maps(xd, ext, 10, cfar="os", cfar_rank=150).tobytes() == multitarget_tracker(CFAR_2D_OS(xd, 18, 4, rank=150), ext, 10).tobytes()
    assert track_maps(xd, ext, 10, cfar="mean").tobytes() == track_maps(xd, ext, 10).tobytes()
    assert track_maps(xs, ext, 10, cfar="mean").tobytes() == track_maps(xs, ext, 10).tobytes()
    swant = simple_target_tracker(cf, 300.0, 200.0)
    assert simple_track_maps(xd, 300.0, 200.0, cfar="os").tobytes() == swant.tobytes()
    assert simple_track_maps(xs, 300.0, 200.0, cfar="os").tobytes() == swant.tobytes()
    assert simple_track_maps(xd, 300.0, 200.0, cfar="mean").tobytes() == simple_track_maps(xd, 300.0, 200.0).tobytes()
    assert simple_track_maps(xs, 300.0, 200.0, cfar="mean").tobytes() == simple_track_maps(xs, 300.0, 200.0).tobytes()
    hold = 3
    CF = np.moveaxis(CFAR_2D_OS(x, 18, 4), 0, 2)   # (H, W, N) float64
    rwant = np.concatenate([render_frames(persistence(CF, k, hold, 0.9)[:, :, None]) for k in range(N)])
    got = render_maps(xd, 18, 4, hold, 0.9, slab=5, cfar="os")
    assert got.shape == (N, W, H, 4) and np.array_equal(got.cpu().numpy(), rwant)
    assert np.array_equal(render_maps(xs, 18, 4, hold, 0.9, cfar="os"), rwant)
    assert np.array_equal(render_maps(xd, 18, 4, hold, 0.9, cfar="mean").cpu().numpy(), render_maps(xd, 18, 4, hold, 0.9).cpu().numpy())
    assert not np.array_equal(rwant, render_maps(xd, 18, 4, hold, 0.9).cpu().numpy())
    with pytest.raises(ValueError):
        track_maps(xd, ext, 10, cfar="median")


@pytest.mark.parametrize("scale", ["reference", "plain"])
def test_capture(gpu_ready, scale):
    """one prc_cfar_os call captured on a side stream and replayed twice on new inputs == the eager results"""
    import torch
    from passiveradar_amd import _lib, engine
    rng = np.random.default_rng(10)
    N, H, W = 3, 33, 130
    frames = [dev(rayleigh(rng, (N, H, W)) * np.float32(s)) for s in (1.0, 7.0, 0.02)]
    d = engine.cfar_os_desc(H, W, 18, 4, None, scale, False)
    nws = engine.cfar_os_workspace_bytes(d, N)
    assert nws == (0 if scale == "plain" else 4 * 64 * N)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda") if nws else None
    eager = []
    for x in frames:
        o, z = torch.empty_like(x), torch.empty_like(x)
        engine.cfar_os_execute(d, x, o, z, N, ws, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        eager.append((o.cpu().numpy(), z.cpu().numpy()))
    xin, o, z = frames[0].clone(), torch.zeros_like(frames[0]), torch.zeros_like(frames[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.cfar_os_execute(d, xin, o, z, N, ws, _lib.torch_stream_ptr())
    side.synchronize()
    for k in (1, 2):
        xin.copy_(frames[k])
        o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(o.cpu().numpy()), bits(eager[k][0])) and np.array_equal(bits(z.cpu().numpy()), bits(eager[k][1])), k
