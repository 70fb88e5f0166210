"""Exact ambiguity patches on the GPU (prc_xambg_patch, prc_xambg_patch_peaks; range_doppler_processing.xambg_patch,
target_detection.refine_peaks) against the float64 oracle of tests/xambg_patch_oracle.py.

The accuracy bar of every value test: max|X_gpu - X_oracle| <= 1e-6 ||w ref||_2 ||srv||_2, the Cauchy-Schwarz bound on any
cell (a noise-floor patch's own peak is 100x below an echo's, so peak-relative error is the wrong scale).  1e-6 is 2.5x
above the worst legitimate float32 form (exact phasors, a plain sequential float32 sum over 1024 samples: 3.9e-7) and below
what an un-reseeded 1024-step recurrence gives (1.8e-6).  Every test prints the figure it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import xambg_patch_oracle as PO
from conftest import load_golden, rel_err
from passiveradar_amd import scene

pytestmark = pytest.mark.gpu

BAR = 1e-6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case_scene(n):
    """(ref, srv, Kaiser-5 window): clutter at 0 Hz, lags 2 / 9 / 40, echoes at 80, -35 and 120 Hz; CPI 1 s"""
    ref, srv = scene.make_scene(n, float(n), 16, scene.scene_seed(97, n % 7))
    return ref, srv, np.kaiser(n, 5.0).astype(np.float32)


def value_calls(n):
    """(name, lags, dopplers, nlags, ndoppler, step): five patches in one call at the common shape 16 x 16, step 0.5 --
    around the clutter, across the wrap, near Nyquist, at a negative Doppler, and far out on a negative lag -- then the
    spacings and the shape that are per call: the Nyquist patch at step 0.3, the negative-Doppler patch at the fine step
    0.1, and a patch of one cell; then the lag counts either side of the kernel's two forms"""
    fs = float(n)
    return (("five", [-3, n - 5, 0, 4, -(n - 1)], [-4.0, -4.0, 0.37 * fs, -38.7, 77.25], 16, 16, 0.5),
            ("nyquist", [0], [0.37 * fs], 16, 16, 0.3),
            ("fine", [4], [-35.8], 16, 16, 0.1),
            ("cell", [9], [0.0], 1, 1, 0.5),
            # up to 32 lags a workgroup takes 16 lags in four sample slices per wavefront, above that 64 lags: both sides of
            # the threshold, and 27 lags as two groups of 16 with a ragged end
            ("lags27", [-3, n - 20], [-4.0, 77.0], 27, 16, 0.5),
            ("lags32", [-3], [-4.0], 32, 16, 0.5),
            ("lags33", [-3], [-4.0], 33, 16, 0.5),
            ("lags64", [-20, n - 30], [-4.0, -38.7], 64, 16, 0.5))


@functools.lru_cache(maxsize=None)
def value_oracle(n, windowed, wrap):
    ref, srv, w = case_scene(n)
    w = w if windowed else None
    return tuple(PO.patches(ref, srv, float(n), lags, dops, nl, nd, step, w, wrap) for _, lags, dops, nl, nd, step in value_calls(n))


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("n", [4096, 6001, 65553])
def test_values_against_the_oracle(gpu_ready, n, windowed, wrap):
    """whole tiles, a ragged tail, many tiles (where a drifting phase shows); window None and Kaiser-5; both wrap rules"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    ref, srv, w = case_scene(n)
    w = w if windowed else None
    scale = PO.bound(ref, srv, w)
    for (name, lags, dops, nl, nd, step), want in zip(value_calls(n), value_oracle(n, windowed, wrap)):
        X = xambg_patch(ref, srv, float(n), lags, dops, nl, nd, step, w, wrap)
        assert X.shape == (len(lags), nd, nl) and X.dtype == np.complex64
        err = np.abs(X - want).reshape(len(lags), -1).max(axis=1) / scale
        print(f"n {n} window {windowed} wrap {wrap} {name}: err / bound per patch {np.array2string(err, precision=3)}, "
              f"largest cell / bound {np.abs(want).max() / scale:.3g}")
        assert err.max() <= BAR, name


def test_group_loops_and_ragged_ends(gpu_ready):
    """nlags = 130 (three lag groups, the last of two lanes), ndoppler = 40 (three Doppler groups, the last of eight rows)"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 6001
    ref, srv, w = case_scene(n)
    for wrap in (True, False):
        X = xambg_patch(ref, srv, float(n), [-60], [-10.0], 130, 40, 0.5, w, wrap)
        err = np.abs(X - PO.patches(ref, srv, float(n), [-60], [-10.0], 130, 40, 0.5, w, wrap)).max() / PO.bound(ref, srv, w)
        print(f"130 x 40, wrap {wrap}: {err:.3g}")
        assert err <= BAR


def test_largest_patch_on_a_frame_shorter_than_a_tile(gpu_ready):
    """nlags = 1024, ndoppler = 4096 (the limits) on n = 61: the lag span laps the frame sixteen times"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 61
    ref, srv = scene.make_scene(n, float(n), 16, 5)
    for wrap in (True, False):
        X = xambg_patch(ref, srv, float(n), [-30], [-7.0], 1024, 4096, 0.01, None, wrap)
        err = np.abs(X - PO.patches(ref, srv, float(n), [-30], [-7.0], 1024, 4096, 0.01, None, wrap)).max() / PO.bound(ref, srv)
        print(f"1024 x 4096 on n = 61, wrap {wrap}: {err:.3g}")
        assert err <= BAR


def test_seventy_patches_in_one_call(gpu_ready):
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 4096
    ref, srv, w = case_scene(n)
    rng = np.random.default_rng(70)
    lags = rng.integers(-(n - 1), n, 70)
    dops = rng.uniform(-0.5 * n, 0.5 * n, 70)
    X = xambg_patch(ref, srv, float(n), lags, dops, 4, 4, 0.25, w, True)
    err = np.abs(X - PO.patches(ref, srv, float(n), lags, dops, 4, 4, 0.25, w, True)).max() / PO.bound(ref, srv, w)
    print(f"70 patches: {err:.3g}")
    assert err <= BAR


def test_two_frames_in_a_stack(gpu_ready):
    """patches on both frames: a dense NumPy stack, and a torch view whose rows are frame_stride = n + 37 apart"""
    import torch
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 6001
    a, b = case_scene(n), scene.make_scene(n, float(n), 16, 11)
    ref, srv = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    lags, dops, frame = [-3, 1, 7, n - 2], [-4.0, -4.0, 78.0, 0.0], [0, 1, 1, 0]
    want = PO.patches(ref, srv, float(n), lags, dops, 16, 16, 0.5, a[2], True, frame)
    scale = max(PO.bound(ref[k], srv[k], a[2]) for k in range(2))
    X = xambg_patch(ref, srv, float(n), lags, dops, 16, 16, 0.5, a[2], True, frame)
    big_r = torch.full((2, n + 37), float("nan"), dtype=torch.complex64, device="cuda")
    big_s = torch.full((2, n + 37), float("nan"), dtype=torch.complex64, device="cuda")
    big_r[:, :n], big_s[:, :n] = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()
    Xt = xambg_patch(big_r[:, :n], big_s[:, :n], float(n), lags, dops, 16, 16, 0.5, torch.from_numpy(a[2]).cuda(), True, frame)
    err = np.abs(X - want).max() / scale
    print(f"two frames: {err:.3g}")
    assert err <= BAR
    assert np.array_equal(bits(Xt.cpu().numpy()), bits(X))


def test_direct_xambg_golden_on_the_device(gpu_ready):
    """the reference-made direct_xambg surface through xambg_patch: 2e-6 of the peak, the bar of the small goldens"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    g = load_golden("direct_xambg")
    for t in "ab":
        ref, srv, R, F, fs = g[f"ref_{t}"], g[f"srv_{t}"], int(g[f"R_{t}"]), int(g[f"F_{t}"]), float(g[f"fs_{t}"])
        cpi = ref.shape[0] / fs
        X = xambg_patch(ref, srv, fs, [0], [-0.5 * F / cpi], R + 1, F, 1.0 / cpi, None, wrap=False)[0][:, ::-1]
        err = rel_err(X, g[f"out_{t}"][:, :, 0])
        print(f"direct_xambg golden {t}: {err:.3g}")
        assert err < 2e-6


@pytest.mark.parametrize("windowed", [False, True])
def test_closed_form_on_the_device(gpu_ready, windowed):
    """srv = roll(ref, D) exp(j 2 pi f i / Fs), f n / Fs an integer, wrap: X(D, f) = exp(-j 2 pi f D / Fs) sum w |ref|^2"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n, D, f = 65553, 7, 5.0
    fs = float(n)
    ref = scene.white_reference(n, 5)
    srv = (np.roll(ref, D).astype(np.complex128) * np.exp(2j * np.pi * f * np.arange(n) / fs)).astype(np.complex64)
    w = np.kaiser(n, 5.0).astype(np.float32) if windowed else None
    X = xambg_patch(ref, srv, fs, [D - 1], [f - 2.0], 3, 5, 1.0, w, True)[0]
    want = np.exp(-2j * np.pi * f * D / fs) * np.sum((1.0 if w is None else w.astype(np.float64)) * np.abs(ref.astype(np.complex128)) ** 2)
    err = abs(X[2, 1] - want) / PO.bound(ref, srv, w)
    print(f"closed form, window {windowed}: {err:.3g} (cell / bound {abs(want) / PO.bound(ref, srv, w):.3g})")
    assert err <= BAR
    assert np.unravel_index(np.argmax(np.abs(X)), X.shape) == (2, 1)


REFINE = dict(n=65536, fs=65536.0, R=16, seed=779, delay=5)


def refine_scene(fd):
    s = REFINE
    ref, srv = scene.make_scene(s["n"], s["fs"], s["R"], s["seed"], targets=((s["delay"], fd, 1.0),), clutter=())
    return ref, srv, np.kaiser(s["n"], 5.0).astype(np.float32)


def assert_peaks_equal(got, want, step):
    assert got["d"].tolist() == want["d"].tolist() and got["l"].tolist() == want["l"].tolist()
    assert got["flags"].tolist() == want["flags"].tolist()
    assert np.abs(got["lag"] - want["lag"]).max() <= 1e-9
    assert np.abs(got["doppler"] - want["doppler"]).max() <= 1e-9 * abs(step)
    assert np.all(np.abs(got["amplitude"] - want["amplitude"]) <= 2.0 ** -23 * want["amplitude"])   # one float32 rounding


@pytest.mark.parametrize("fd", [3.3, 28.3, -30.6])
def test_refinement(gpu_ready, fd):
    import torch
    from passiveradar_amd.range_doppler_processing import xambg_patch
    from passiveradar_amd.target_detection import refine_peaks
    ref, srv, w = refine_scene(fd)
    fs, step = REFINE["fs"], 0.25
    # the patch of the issue, then the argmax forced onto the Doppler edge (row 0) and onto the lag edge (column 0)
    lags, dops = [4, 4, 5], [round(fd) - 2.0, round(fd) + 1.0, round(fd) - 2.0]
    X = xambg_patch(ref, srv, fs, lags, dops, 3, 17, step, w, True)
    pk = refine_peaks(X, lags, dops, step)
    want = PO.refine(X, lags, dops, step)
    print(f"fd {fd}: refined {pk['doppler'][0]:.5f} Hz, lag {pk['lag'][0]:.4f}, amplitude {pk['amplitude'][0]:.1f}; "
          f"oracle on the same cells {want['doppler'][0]:.5f}")
    assert pk["l"][0] == 1 and pk["flags"][0] == 0 and abs(pk["doppler"][0] - fd) <= 0.005
    assert_peaks_equal(pk, want, step)
    assert pk["flags"][1] == 1 and pk["d"][1] == 0 and pk["l"][1] == 1 and pk["doppler"][1] == dops[1]
    assert pk["flags"][2] == 2 and pk["l"][2] == 0 and pk["lag"][2] == 5.0
    # device tensors in, device tensors out
    t = refine_peaks(torch.from_numpy(X).cuda(), lags, dops, step)
    assert all(v.is_cuda for v in t.values())
    for k in ("lag", "doppler", "amplitude", "d", "l", "flags"):
        assert np.array_equal(t[k].cpu().numpy().astype(pk[k].dtype), pk[k]), k


def test_refinement_ties_edges_and_flat_patches(gpu_ready):
    """hand-made cells: the first of equal cells wins, edges are flagged and left uninterpolated, a flat patch is cell (0, 0)"""
    from passiveradar_amd.target_detection import refine_peaks
    X = np.zeros((6, 5, 4), np.complex64)
    X[0, 2, 1], X[0, 1, 1], X[0, 3, 1], X[0, 2, 0], X[0, 2, 2] = 4, 2, 3, 1, 1
    X[1, 0, 2] = 1j
    X[2, 3, 3], X[2, 3, 2] = -2, 2
    X[4] = 3 - 4j                                              # flat and not zero
    X[5, 4, 3] = 1e-20                                         # the last cell: both edges
    lags, dops = [10, 20, 30, 40, 50, 60], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    pk = refine_peaks(X, lags, dops, 0.5)
    assert_peaks_equal(pk, PO.refine(X, lags, dops, 0.5), 0.5)
    assert pk["flags"].tolist() == [0, 1, 0, 7, 7, 3]
    big = np.zeros((1, 70, 130), np.complex64)                 # more cells than lanes, the peak late in the scan
    big[0, 66, 127], big[0, 65, 127], big[0, 67, 127] = 5, 4, 1
    assert_peaks_equal(refine_peaks(big, [0], [0.0], 1.0), PO.refine(big, [0], [0.0], 1.0), 1.0)


@pytest.mark.parametrize("gain", [1e-3, 1e3])
def test_amplitude_ladder(gpu_ready, gain):
    """inputs scaled by 1e-3 and 1e3 hold the same bar; the bound scales with them"""
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 6001
    ref, srv, w = case_scene(n)
    ref, srv = (ref * np.float32(gain)).astype(np.complex64), (srv * np.float32(gain)).astype(np.complex64)
    lags, dops = [-3, n - 5, 4], [-4.0, 0.37 * n, -38.7]
    X = xambg_patch(ref, srv, float(n), lags, dops, 16, 16, 0.5, w, True)
    err = np.abs(X - PO.patches(ref, srv, float(n), lags, dops, 16, 16, 0.5, w, True)).max() / PO.bound(ref, srv, w)
    print(f"gain {gain:g}: {err:.3g}")
    assert err <= BAR


def test_dead_air(gpu_ready):
    from passiveradar_amd.range_doppler_processing import xambg_patch
    from passiveradar_amd.target_detection import refine_peaks
    n = 6001
    z = np.zeros(n, np.complex64)
    lags, dops = [-3, 7], [-4.0, 100.0]
    X = xambg_patch(z, z, float(n), lags, dops, 16, 16, 0.5, np.kaiser(n, 5.0), True)
    assert not bits(X).any()
    pk = refine_peaks(X, lags, dops, 0.5)
    assert np.all(pk["flags"] & 4) and pk["d"].tolist() == [0, 0] and pk["l"].tolist() == [0, 0]
    assert pk["lag"].tolist() == [-3.0, 7.0] and pk["doppler"].tolist() == dops and pk["amplitude"].tolist() == [0.0, 0.0]
    assert np.array_equal(bits(xambg_patch(z, z, float(n), lags, dops, 16, 16, 0.5, np.kaiser(n, 5.0), True)), bits(X))
    pk2 = refine_peaks(X, lags, dops, 0.5)
    assert pk2.tobytes() == pk.tobytes()


def test_determinism_device_path_and_workspace(gpu_ready):
    """two calls give the same bits; torch tensors on a side stream give the bits of the NumPy path; the result does not
    depend on what the workspace held"""
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 65553
    ref, srv, w = case_scene(n)
    lags, dops = [-3, n - 5, 4], [-4.0, 0.37 * n, -38.7]
    X = xambg_patch(ref, srv, float(n), lags, dops, 16, 16, 0.5, w, True)
    assert np.array_equal(bits(xambg_patch(ref, srv, float(n), lags, dops, 16, 16, 0.5, w, True)), bits(X))
    tr, ts, tw = (torch.from_numpy(v).cuda() for v in (ref, srv, w))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rs = tr * 1                                            # produced on the side stream: the launch must follow it
        Xt = xambg_patch(rs, ts, float(n), lags, dops, 16, 16, 0.5, tw, True)
    side.synchronize()
    assert Xt.is_cuda and Xt.dtype == torch.complex64
    assert np.array_equal(bits(Xt.cpu().numpy()), bits(X))
    # a poisoned workspace
    desc = engine.patch_desc(n, 16, 16, float(n), 0.5, True)
    rec = torch.from_numpy(engine.patch_list(lags, dops, None, 1, n).view(np.uint8)).cuda()
    nws = engine.xambg_patch_workspace_bytes(desc, 3)
    for fill in (0xFF, 0x00, 0x7F):
        ws = torch.full((nws,), fill, dtype=torch.uint8, device="cuda")
        out = torch.full((3, 16, 16), float("nan"), dtype=torch.complex64, device="cuda")
        engine.xambg_patch_execute(desc, tr, ts, tw, rec, 3, out, ws, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(X)), fill


def test_errors(gpu_ready):
    """each PRC_EINVAL case raises (ValueError), as do mismatched shapes; a device-built list with a bad record yields zeros
    for that patch and leaves the rest intact"""
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.range_doppler_processing import xambg_patch
    n = 4096
    ref, srv, _ = case_scene(n)
    good = dict(lags=[0], dopplers=[0.0], nlags=4, ndoppler=4, doppler_step=0.5)
    with pytest.raises(ValueError, match="same length"):
        xambg_patch(ref, srv[:-1], float(n), **good)
    for bad in (dict(nlags=0), dict(nlags=1025), dict(ndoppler=0), dict(ndoppler=4097), dict(lags=[n]), dict(lags=[-n]),
                dict(doppler_step=float("inf")), dict(dopplers=[float("nan")]), dict(frame=[1]), dict(frame=[-1])):
        with pytest.raises(ValueError):
            xambg_patch(ref, srv, float(n), **{**good, **bad})
    for rate in (float("nan"), float("inf"), 0.0):
        with pytest.raises(ValueError):
            xambg_patch(ref, srv, rate, **good)
    tr, ts = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()
    desc = engine.patch_desc(n, 4, 4, float(n), 0.5, True)
    rec = engine.patch_list([1, 2, 3, 4, 5], [0.0, 1.0, 2.0, 3.0, 4.0], None, 1, n)
    ws = torch.empty(engine.xambg_patch_workspace_bytes(desc, 5), dtype=torch.uint8, device="cuda")
    out = torch.empty((5, 4, 4), dtype=torch.complex64, device="cuda")
    st = _lib.torch_stream_ptr()
    d_rec = torch.from_numpy(rec.view(np.uint8)).cuda()
    for args in ((None, ts, d_rec, out, ws), (tr, None, d_rec, out, ws), (tr, ts, None, out, ws), (tr, ts, d_rec, None, ws),
                 (tr, ts, d_rec, out, None)):
        with pytest.raises(ValueError, match="null pointer"):
            engine.xambg_patch_execute(desc, args[0], args[1], None, args[2], 5, args[3], args[4], st)
    with pytest.raises(ValueError):
        engine.xambg_patch_execute(desc, tr, ts, None, d_rec, -1, out, ws, st)
    engine.xambg_patch_execute(desc, tr, ts, None, d_rec, 5, out, ws, st)
    torch.cuda.synchronize()
    want = out.cpu().numpy()
    assert np.abs(want).min() > 0
    # records no host check has seen: a frame outside the stack, a lag origin outside the frame, a Doppler that is no number
    rec["frame"][1], rec["lag0"][2], rec["doppler0"][3] = 7, n, np.nan
    rec["frame"][4] = -1
    d_rec = torch.from_numpy(rec.view(np.uint8)).cuda()
    out.fill_(float("nan"))
    ws.fill_(0xFF)
    engine.xambg_patch_execute(desc, tr, ts, None, d_rec, 5, out, ws, st)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[0]), bits(want[0])) and not bits(got[1:]).any()
    assert C.sizeof(_lib.Patch) == rec.dtype.itemsize
