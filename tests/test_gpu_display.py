"""display_limits / render_frames / render_maps on the MI355X against np.percentile and the NumPy restatement of the
display contract (tests/display_oracle.py, itself held to matplotlib by tests/test_display_host.py).  Selection is exact
and every later operation a single rounded float64 operation in a fixed order, so everything is compared for equality."""
import ctypes as C

import numpy as np
import pytest

import display_oracle as D
import guard

pytestmark = pytest.mark.gpu

PAIRS = ((35, 99), (0, 100), (50, 50))


def small_cases():
    c = D.frame_cases()
    c["dense_100x45"] = np.random.default_rng(5).exponential(1.0, (100, 45))     # two tiles each way, neither full
    return c


_BIG = {}


def big_batch():
    """three 1024 x 177 frames of different statistics, (H, W, 3): counters above 2^16, frames not mixed up"""
    if not _BIG:
        rng = np.random.default_rng(21)
        a = rng.exponential(1.0, (1024, 177))
        b = rng.exponential(3.0, (1024, 177))
        b[rng.random(b.shape) < 0.5] = 0.0
        c = rng.standard_normal((1024, 177)) * 5.0 - 2.0
        _BIG["x"] = np.stack([a, b, c], axis=2)
    return _BIG["x"]


def np_limits(f, p_lo, p_hi, hi_scale=1.5):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([np.percentile(f.flatten(), p_lo), hi_scale * np.percentile(f.flatten(), p_hi)])


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("p", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_display_limits_equal_numpy(gpu_ready, p):
    from passiveradar_amd.plotting_tools import display_limits
    for name, f in small_cases().items():
        got = display_limits(f[:, :, None], *p)
        assert got.shape == (1, 2) and got.dtype == np.float64
        assert np.array_equal(got[0], np_limits(f, *p), equal_nan=True), (name, got)
        assert np.array_equal(got[0], D.limits(f, *p), equal_nan=True), (name, got)
    x = big_batch()
    got = display_limits(dev(np.moveaxis(x, 2, 0)), *p).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], np_limits(x[:, :, k], *p)), k


def test_display_limits_float32_is_the_widened_contract(gpu_ready):
    from passiveradar_amd.plotting_tools import display_limits
    for name, f in small_cases().items():
        f32 = f.astype(np.float32)
        for p in PAIRS:
            got = display_limits(f32[:, :, None], *p)
            assert np.array_equal(got[0], D.limits(f32.astype(np.float64), *p), equal_nan=True), (name, p, got)
    x = big_batch().astype(np.float32)
    got = display_limits(dev(np.moveaxis(x, 2, 0)), 35, 99, 2.0).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], D.limits(x[:, :, k].astype(np.float64), 35, 99, 2.0)), k


def test_render_frames_equal_the_oracle(gpu_ready):
    from passiveradar_amd.plotting_tools import render_frames
    table = np.random.default_rng(3).integers(0, 256, (256, 4), dtype=np.uint8)
    for name, f in small_cases().items():
        H, W = f.shape
        for orient in ("plot", "stored"):
            for lut in (None, table):
                got = render_frames(f[:, :, None], lut=lut, orient=orient)
                assert got.dtype == np.uint8 and got.shape == ((1, W, H, 4) if orient == "plot" else (1, H, W, 4))
                assert np.array_equal(got[0], D.render(f, lut=lut, orient=orient)), (name, orient, lut is None)
        f32 = f.astype(np.float32)
        assert np.array_equal(render_frames(f32[:, :, None])[0], D.render(f32.astype(np.float64))), name
    x = big_batch()
    got = render_frames(dev(np.moveaxis(x, 2, 0)), lut=table).cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], D.render(x[:, :, k], lut=table)), k


def test_render_frames_with_given_limits(gpu_ready):
    from passiveradar_amd.plotting_tools import gnuplot2_lut, render_frames
    c = small_cases()
    x = np.stack([c["negative"], c["dense_64x48"], c["negative"], c["dense_64x48"] * 0 + 0.5], axis=2)   # (64, 48, 4)
    x[7, 9, 1] = np.nan
    lim = np.array([[-2.0, 3.0], [0.5, 0.5], [3.0, -2.0], [np.nan, 1.0]])
    lut = gnuplot2_lut()
    for orient in ("plot", "stored"):
        got = render_frames(x, limits=lim, orient=orient)
        for k in range(4):
            assert np.array_equal(got[k], D.render(x[:, :, k], lim=lim[k], orient=orient)), (orient, k)
        assert np.all(got[1] == lut[0])          # vmin == vmax: lut[0] everywhere, the NaN cell included
        assert not got[2].any()                  # vmin > vmax: the deviation from matplotlib, which raises
        assert not got[3].any()                  # NaN limits: every cell bad
        again = render_frames(dev(np.moveaxis(x, 2, 0)), limits=dev(lim), orient=orient)
        assert np.array_equal(again.cpu().numpy(), got)
        assert np.array_equal(render_frames(dev(np.moveaxis(x, 2, 0)), limits=lim, orient=orient).cpu().numpy(), got)


def test_numpy_and_device_paths_and_a_side_stream_agree(gpu_ready):
    import torch
    from passiveradar_amd.plotting_tools import display_limits, render_frames
    c = small_cases()
    x = np.stack([c["dense_37x23"], c["half_zero"], c["two_values"], c["one_nan"], c["one_inf"]], axis=2)
    xd = dev(np.moveaxis(x, 2, 0))
    lim, px = display_limits(x), render_frames(x)
    ld, pd = display_limits(xd), render_frames(xd)
    assert ld.is_cuda and ld.dtype == torch.float64 and pd.is_cuda and pd.dtype == torch.uint8
    assert pd.shape == (5, 23, 37, 4) and pd.is_contiguous()
    assert np.array_equal(ld.cpu().numpy(), lim, equal_nan=True) and np.array_equal(pd.cpu().numpy(), px)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ls, ps = display_limits(xd), render_frames(xd)
    side.synchronize()
    assert np.array_equal(ls.cpu().numpy(), lim, equal_nan=True) and np.array_equal(ps.cpu().numpy(), px)
    empty = render_frames(torch.empty((0, 4, 3), dtype=torch.float64, device="cuda"))
    assert empty.shape == (0, 3, 4, 4) and render_frames(np.empty((4, 3, 0))).shape == (0, 3, 4, 4)


def test_render_maps_equals_cfar_persistence_oracle(gpu_ready):
    from passiveradar_amd.plotting_tools import persistence, render_maps
    from passiveradar_amd.target_detection import CFAR_2D_abs
    rng = np.random.default_rng(17)
    L, H, W, hold = 8, 64, 48, 3
    x = (rng.standard_normal((L, H, W)) + 1j * rng.standard_normal((L, H, W))).astype(np.complex64)
    for k in range(L):
        x[k, 20 + k, 30] += 9.0
    CF = np.moveaxis(CFAR_2D_abs(x, 8, 2), 0, 2)                                   # (H, W, L) float64
    want = np.stack([D.render(persistence(CF, k, hold, 0.9)) for k in range(L)])
    got = render_maps(dev(x), 8, 2, hold, 0.9, slab=3)                             # slab edges at frames 3 and 6
    assert got.shape == (L, W, H, 4) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(render_maps(dev(x), 8, 2, hold, 0.9).cpu().numpy(), want)            # one slab
    assert np.array_equal(render_maps(np.moveaxis(x, 0, 2), 8, 2, hold, 0.9, slab=5), want)    # numpy (H, W, L)
    lim = np.tile([0.5, 4.0], (L, 1))
    fixed = render_maps(dev(x), 8, 2, hold, 0.9, slab=3, limits=lim, orient="stored").cpu().numpy()
    for k in range(L):
        assert np.array_equal(fixed[k], D.render(persistence(CF, k, hold, 0.9), lim=lim[k], orient="stored")), k


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_guard_bands(gpu_ready, dtype):
    """both entry points on guarded frames, limits and out: nothing outside the documented extents is read as data or
    written, and the result does not depend on the poison"""
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    L, H, W = 3, 70, 45
    n = H * W
    f = np.random.default_rng(2).exponential(1.0, (L, H, W)).astype(dtype)
    f[1][np.random.default_rng(3).random((H, W)) < 0.5] = 0.0
    code = _lib.REAL_F32 if dtype == "float32" else _lib.REAL_F64
    st = _lib.torch_stream_ptr()
    want = np.stack([D.limits(f[k].astype(np.float64)) for k in range(L)])

    def run_limits(a, s):
        _lib.check(lib.prc_display_limits(a["frames"].data_ptr(), code, n, L, 35.0, 99.0, 1.5, a["limits"].data_ptr(), st))
        torch.cuda.synchronize()
    got = guard.check(run_limits, {"frames": guard.In(dev(f.reshape(1, L * n)))},
                      {"limits": guard.Out(1, 2 * L, torch.float64)})
    assert np.array_equal(got.tight["limits"].cpu().numpy().reshape(L, 2), want)

    for orient in (_lib.DISPLAY_PLOT, _lib.DISPLAY_STORED):
        def run_rgba(a, s):
            _lib.check(lib.prc_display_rgba(a["frames"].data_ptr(), code, H, W, L, a["limits"].data_ptr(), None, orient,
                                            a["out"].data_ptr(), st))
            torch.cuda.synchronize()
        # one RGBA pixel per int32 element (the alpha byte of the sentinel, 0x7f, is no alpha the table holds)
        got = guard.check(run_rgba, {"frames": guard.In(dev(f.reshape(1, L * n))), "limits": guard.In(dev(want.reshape(1, 2 * L)))},
                          {"out": guard.Out(1, L * n, torch.int32)})
        px = got.tight["out"].cpu().numpy().view(np.uint8).reshape(L, n, 4)
        for k in range(L):
            exp = D.render(f[k].astype(np.float64), orient="plot" if orient == _lib.DISPLAY_PLOT else "stored")
            assert np.array_equal(px[k], exp.reshape(n, 4)), (orient, k)


def test_bad_arguments_write_nothing(gpu_ready):
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.plotting_tools import display_limits, render_frames
    lib = _lib.lib()
    x = torch.ones((2, 4, 3), dtype=torch.float64, device="cuda")
    lim = torch.full((2, 2), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((2 * 12 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    E = _lib.PRC_EINVAL
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.prc_display_limits(p(x), 7, 12, 2, 35.0, 99.0, 1.5, p(lim), None) == E
    assert lib.prc_display_limits(p(x), 1, 12, 2, 35.0, 101.0, 1.5, p(lim), None) == E
    assert lib.prc_display_limits(p(x), 1, 0, 2, 35.0, 99.0, 1.5, p(lim), None) == E
    assert lib.prc_display_limits(p(x), 1, 12, -2, 35.0, 99.0, 1.5, p(lim), None) == E
    assert lib.prc_display_rgba(p(x), 1, 4, 3, 2, p(lim), None, 5, p(out), None) == E
    assert lib.prc_display_rgba(p(x), 9, 4, 3, 2, p(lim), None, 0, p(out), None) == E
    assert lib.prc_display_rgba(p(x), 1, 4, 0, 2, p(lim), None, 0, p(out), None) == E
    assert lib.prc_display_rgba(p(x), 1, 4, 3, 2, None, None, 0, p(out), None) == E
    torch.cuda.synchronize()
    assert bool((lim == 7.0).all()) and bool((out == 0xA5).all())
    for bad in (dict(p_lo=-1), dict(p_hi=float("nan"))):
        with pytest.raises(ValueError):
            display_limits(x, **bad)
    with pytest.raises(ValueError):
        render_frames(x, orient="upside-down")
    with pytest.raises(ValueError):
        render_frames(x, limits=lim[:1])
    with pytest.raises(ValueError):
        render_frames(x[0])
