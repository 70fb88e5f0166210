"""The NumPy call and the torch call of every front door give the same bits on the same data, once the device result is
brought to the host and cast as the docstring says (float32 -> float64, or bool).  Two frames of 16 x 24 cells: the smallest
stack where a frame stride, or a swapped H and W, can go wrong."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 2, 16, 24
EXT = [250.0, 0.125 * (W - 1)]
FW, GW = 8, 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def maps():
    """complex maps [N, H, W]: unit noise with one strong echo per frame outside the guards"""
    rng = np.random.default_rng(5)
    x = ((rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))) * np.sqrt(0.5)).astype(np.complex64)
    for k in range(N):
        x[k, 3, 10 + k] += 6.0
    return x


def hwn(x):
    """[N, H, W] as the scripts load it: (H, W, N)"""
    return np.moveaxis(x, 0, 2)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,cplx", [("CFAR_2D", False), ("CFAR_2D_abs", True), ("CFAR_2D_abs", False), ("CFAR_2D_OS", True),
                                       ("CFAR_2D_OS", False)])
def test_cfar(gpu_ready, name, cplx):
    """CFAR_2D takes magnitudes (CFAR_2D_abs is its complex form); the other two take either"""
    import torch
    from passiveradar_amd import target_detection as T
    x = maps() if cplx else np.abs(maps())
    fn = getattr(T, name)
    for arg in (x, x[0]):
        got, want = fn(dev(arg), FW, GW), fn(arg, FW, GW)
        assert got.dtype == torch.float32 and want.dtype == np.float64
        assert same(host(got).astype(np.float64), want)
        got, want = fn(dev(arg), FW, GW, 1.5), fn(arg, FW, GW, 1.5)
        assert got.dtype == torch.bool and want.dtype == bool and want.any() and not want.all()
        assert same(host(got), want)
    if name == "CFAR_2D_OS":
        (got, gz), (want, wz) = fn(dev(x), FW, GW, scale="plain", return_noise=True), fn(x, FW, GW, scale="plain", return_noise=True)
        assert same(host(got).astype(np.float64), want) and same(host(gz).astype(np.float64), wz)


def test_measure_and_track(gpu_ready):
    from passiveradar_amd.target_detection import CFAR_2D_abs, get_measurements, multitarget_tracker, track_maps
    x = maps()
    cf = CFAR_2D_abs(x, FW, GW).astype(np.float32)
    counts, meas, index = (host(t) for t in get_measurements(dev(cf), 99.8, EXT))
    assert counts.dtype == np.int32 and meas.dtype == np.float64 and index.dtype == np.int64
    for f in range(N):
        one = get_measurements(cf[f], 99.8, EXT)
        assert one.shape == (3, counts[f])
        assert same(meas[f, :, :counts[f]], one)
    assert counts.sum() >= 1
    assert same(multitarget_tracker(dev(cf), EXT, 3), multitarget_tracker(hwn(cf), EXT, 3))
    for kw in (dict(), dict(cfar="os"), dict(measure="plots", plot_thresh=1.5), dict(measure="plots", plot_thresh=1.5, cfar="os")):
        assert same(track_maps(dev(x), EXT, 3, FW, GW, **kw), track_maps(hwn(x), EXT, 3, FW, GW, **kw)), kw
    assert same(track_maps(dev(np.abs(x)), EXT, 3, FW, GW), track_maps(hwn(np.abs(x)), EXT, 3, FW, GW))


def test_plots(gpu_ready):
    from passiveradar_amd.target_detection import CFAR_2D_abs, extract_plots
    x = maps()
    cf = CFAR_2D_abs(x, FW, GW).astype(np.float32)
    for weight in (None, x, np.abs(x)):
        got = extract_plots(dev(cf), 1.5, EXT, weight=None if weight is None else dev(weight), return_info=True)
        want = extract_plots(cf, 1.5, EXT, weight=weight, return_info=True)
        assert want[0].sum() >= 1
        for g, w in zip(got[:3], want[:3]):
            assert same(host(g), w)
        assert same(host(got[3]).reshape(-1), want[3].view(np.uint8).reshape(-1)) and same(host(got[4]), want[4])
    one = extract_plots(cf[1], 1.5, EXT)
    counts, meas, _ = extract_plots(cf, 1.5, EXT)
    assert same(one, meas[1, :, :counts[1]])


def test_tbd(gpu_ready):
    from passiveradar_amd.target_detection import CFAR_2D_abs, tbd_maps, tbd_paths, tbd_row_shifts, track_before_detect
    x = maps()
    cf = CFAR_2D_abs(x, FW, GW).astype(np.float32)
    shifts = tbd_row_shifts(H, W, EXT, 0.5, 3.0)
    assert shifts.any()
    prev = np.abs(cf[0])[::-1].copy()
    for kw in (dict(), dict(row_shifts=shifts, prev=prev, clip=4.0), dict(return_back=False)):
        tkw = {k: dev(v) if k == "prev" else v for k, v in kw.items()}
        gs, gb = track_before_detect(dev(cf), EXT, **tkw)
        ws, wb = track_before_detect(cf, EXT, **kw)
        assert ws.dtype == np.float32 and same(host(gs), ws)
        assert (gb is None and wb is None) if kw.get("return_back") is False else (wb.dtype == np.uint8 and same(host(gb), wb))
    gs, gb = track_before_detect(dev(cf[1]), EXT)
    ws, wb = track_before_detect(cf[1], EXT)
    assert ws.shape == (H, W) and same(host(gs), ws) and same(host(gb), wb)
    score, back = track_before_detect(cf, EXT, row_shifts=shifts)
    ends = np.array([[1, 3 * W + 11], [0, 5], [2, 0]], np.int32)
    want = tbd_paths(back, ends, 3, shifts)
    assert want.shape == (3, 3) and want[0, 0] == 3 * W + 11 and (want[2] == -1).all()
    assert same(host(tbd_paths(dev(back), dev(ends), 3, shifts)), want)
    for cfar in ("os", "mean"):
        got = tbd_maps(dev(x), EXT, 0.5, 3.0, thresh=3.0, depth=2, fw=FW, gw=GW, cfar=cfar)
        want = tbd_maps(hwn(x), EXT, 0.5, 3.0, thresh=3.0, depth=2, fw=FW, gw=GW, cfar=cfar)
        assert want[0].sum() >= 1
        for g, w in zip(got, want):
            assert same(host(g), w)


def test_simple_tracker(gpu_ready):
    from passiveradar_amd.target_detection import CFAR_2D_abs, simple_target_tracker, simple_track_maps
    x = maps()
    for cf in (CFAR_2D_abs(x, FW, GW).astype(np.float32), CFAR_2D_abs(x, FW, GW)):
        want = simple_target_tracker(hwn(cf), 300.0, 200.0)
        assert want.shape == (N,) and same(simple_target_tracker(dev(cf), 300.0, 200.0), want)
        assert same(simple_target_tracker(dev(cf), 300.0, 200.0, state=want[-1]), simple_target_tracker(hwn(cf), 300.0, 200.0, state=want[-1]))
    for kw in (dict(), dict(cfar="os")):
        assert same(simple_track_maps(dev(x), 300.0, 200.0, FW, GW, **kw), simple_track_maps(hwn(x), 300.0, 200.0, FW, GW, **kw))


def test_refine_peaks(gpu_ready):
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import refine_peaks
    rng = np.random.default_rng(9)
    X = (rng.standard_normal((2, 5, 7)) + 1j * rng.standard_normal((2, 5, 7))).astype(np.complex64)
    X[0, 2, 3] += 9.0
    X[1, 0, 6] += 9.0
    want = refine_peaks(X, [4, -3], [10.0, -2.5], 0.5)
    got = refine_peaks(dev(X), [4, -3], [10.0, -2.5], 0.5)
    assert want.dtype == _lib.PATCH_PEAK_DTYPE and (want["d"].tolist(), want["l"].tolist()) == ([2, 0], [3, 6])
    for k in ("lag", "doppler", "amplitude", "d", "l", "flags"):
        assert same(host(got[k]).view(want[k].dtype), want[k]), k          # flags: the uint32 word as torch's int32


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_display(gpu_ready, dtype):
    from passiveradar_amd import plotting_tools as P
    x = np.abs(maps()).astype(dtype)
    for k in (0, 1):
        want = P.persistence(hwn(x), k, 2, 0.9)
        assert want.shape == (H, W) and want.dtype == np.float64 and same(host(P.persistence(dev(x), k, 2, 0.9)), want)
    for odt in (np.float64, np.float32):
        want = P.persistence_stack(hwn(x), 2, 0.9, odt)
        assert want.shape == (H, W, N) and want.dtype == odt
        assert same(np.moveaxis(host(P.persistence_stack(dev(x), 2, 0.9, odt)), 0, 2), want)
    lim = P.display_limits(hwn(x))
    assert lim.shape == (N, 2) and lim.dtype == np.float64 and same(host(P.display_limits(dev(x))), lim)
    for kw in (dict(), dict(orient="stored"), dict(limits=lim[::-1].copy()), dict(lut=P.gnuplot2_lut()[::-1].copy())):
        want = P.render_frames(hwn(x), **kw)
        assert want.shape == ((N, H, W, 4) if kw.get("orient") == "stored" else (N, W, H, 4)) and want.dtype == np.uint8
        tkw = {k: dev(v) if k == "limits" else v for k, v in kw.items()}
        assert same(host(P.render_frames(dev(x), **tkw)), want), kw


def test_render_maps(gpu_ready):
    from passiveradar_amd.plotting_tools import render_maps
    x = maps()
    for arg in (x, np.abs(x)):
        for kw in (dict(), dict(cfar="os")):
            assert same(host(render_maps(dev(arg), FW, GW, 2, 0.9, **kw)), render_maps(hwn(arg), FW, GW, 2, 0.9, **kw))


def test_cancel_echoes(gpu_ready):
    from passiveradar_amd.clutter_removal import cancel_echoes
    rng = np.random.default_rng(11)
    n, fs = 4096, 1.0e5
    ref = ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))) * np.sqrt(0.5)).astype(np.complex64)
    i = np.arange(n)
    srv = np.stack([np.roll(ref[b], 7 + b) * np.exp(2j * np.pi * (40.0 + b) * i / fs) for b in range(2)])
    srv = (srv + 0.01 * (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))).astype(np.complex64)
    lags, dops = [[7], [8, 30]], [[40.0], [41.0, -15.0]]
    want = cancel_echoes(ref, srv, fs, lags, dops, wrap=True, return_fit=True)
    got = cancel_echoes(dev(ref), dev(srv), fs, lags, dops, wrap=True, return_fit=True)
    assert want[0].dtype == np.complex64 and want[0].shape == srv.shape and same(host(got[0]), want[0])
    assert np.abs(want[0]).max() < 0.5 * np.abs(srv).max()
    for g, w in zip(got[1:], want[1:]):
        assert len(g) == len(w) == 2 and all(same(a, b) for a, b in zip(g, w))
    one = cancel_echoes(ref[0], srv[0], fs, lags[0], dops[0])
    assert one.shape == (n,) and same(host(cancel_echoes(dev(ref[0]), dev(srv[0]), fs, lags[0], dops[0])), one)


def test_work_is_ordered_on_the_callers_stream(gpu_ready):
    """under ``with torch.cuda.stream(s)`` the launches go to s: s.synchronize() alone makes the results readable"""
    import torch
    from passiveradar_amd.target_detection import CFAR_2D_abs, track_before_detect
    x = maps()
    want_cf = CFAR_2D_abs(x, FW, GW)
    want_score, want_back = track_before_detect(want_cf.astype(np.float32), EXT)
    xt = dev(x)
    pin_cf = torch.empty((N, H, W), dtype=torch.float32).pin_memory()
    pin_score, pin_back = torch.empty_like(pin_cf).pin_memory(), torch.empty((N, H, W), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        cf = CFAR_2D_abs(xt, FW, GW)
        score, back = track_before_detect(cf, EXT)
        for p, t in ((pin_cf, cf), (pin_score, score), (pin_back, back)):
            p.copy_(t, non_blocking=True)
    s.synchronize()
    assert same(pin_cf.numpy().astype(np.float64), want_cf)
    assert same(pin_score.numpy(), want_score) and same(pin_back.numpy(), want_back)
