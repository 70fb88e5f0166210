"""get_measurements / multitarget_tracker / track_maps on the MI355X against the reference's goldens and the NumPy
restatement (tests/tracker_oracle.py), including the edge frames, capacity overflow and the published size."""
import numpy as np
import pytest

import tracker_oracle as T
from conftest import load_golden
from test_tracker_host import check_candidates, check_history, measure_frames

pytestmark = pytest.mark.gpu


def dev_measure(frame, ext, **kw):
    """device candidates of one frame as the restatement's dict"""
    from passiveradar_amd.target_detection import _device_measure
    m = _device_measure(np.asarray(frame, np.float32), ext, **kw)
    c = m.candidates()[0][:min(int(m.counts[0]), m.capacity)]
    return dict(range=c["range"], doppler=c["doppler"], strength=c["strength"], idx=c["index"], count=int(m.counts[0]))


def history_of(h):
    ks = h["kalman_state"]
    return dict(status=h["status"], lifetime=h["lifetime"], measurement=h["measurement"], estimate=h["estimate"],
                hist=h["measurement_history"], x=ks["x"], P=ks["P"], S=ks["S"])


def same_as_restatement(f, ext):
    d = dev_measure(f, ext)
    r = T.measure(np.asarray(f, np.float32), ext)
    assert d["count"] == r["count"]
    check_candidates(d, np.stack((r["range"], r["doppler"], r["strength"])), r["idx"], False)
    return d


def test_get_measurements_matches_the_golden(gpu_ready):
    from passiveradar_amd.target_detection import get_measurements
    for f, ext, cand, idx, tied in measure_frames():
        check_candidates(dev_measure(f, ext), cand, idx, tied)
        out = get_measurements(f, 99.8, ext)                  # the drop-in: (3, M) float64
        assert out.shape == cand.shape and out.dtype == np.float64
        if not tied:
            assert np.array_equal(out[:2], cand[:2])


def test_multitarget_tracker_matches_the_golden(gpu_ready):
    from passiveradar_amd.target_detection import multitarget_tracker, target_track_dtype
    g = load_golden("tracker_scene")
    frames = g["frames"].astype(np.float64) / 256.0
    h = multitarget_tracker(frames, list(g["extent"]), int(g["ntracks"]))
    assert h.dtype == target_track_dtype and h.shape == g["status"].shape
    check_history(history_of(h), g)
    assert np.array_equal(h["kalman_state"]["F1"][3, 2], T.F1) and np.array_equal(h["kalman_state"]["R"][0, 0], T.R)


def test_degenerate_frames_have_no_candidates(gpu_ready):
    ext = [100.0, 50.0]
    zero = np.zeros((40, 30), np.float32)
    assert dev_measure(zero, ext)["count"] == 0
    for bad in (np.nan, np.inf, -np.inf):
        f = np.random.default_rng(1).exponential(1.0, (40, 30)).astype(np.float32)
        f[20, 15] = bad
        assert dev_measure(f, ext)["count"] == 0
        assert T.measure(f, ext)["count"] == 0


def test_mostly_zero_frame_takes_every_cell(gpu_ready):
    """threshold 0: every cell is a candidate (count = n, beyond what one workgroup sorts in LDS), ties broken by
    descending flat index"""
    f = np.zeros((128, 96), np.float32)
    f[60, 40] = 5.0
    f[10, 20] = 3.0
    d = same_as_restatement(f, [30.0, 90.0])
    assert d["count"] == f.size


def test_planted_ties_follow_the_stable_flip_rule(gpu_ready):
    rng = np.random.default_rng(5)
    f = rng.exponential(1.0, (64, 48)).astype(np.float32)
    for h, w in ((10, 20), (50, 30), (12, 9), (40, 38)):
        f[h, w] = 40.0                                  # four equal strongest cells
    f[5, 12] = f[6, 13] = 30.0
    d = same_as_restatement(f, [120.0, 60.0])
    assert np.all(np.diff(d["idx"][:4]) < 0)


def test_minimum_frames(gpu_ready):
    rng = np.random.default_rng(9)
    for H, W in ((8, 17), (9, 17), (8, 18)):
        f = rng.exponential(1.0, (H, W)).astype(np.float32)
        same_as_restatement(f, [10.0, 20.0])


@pytest.mark.parametrize("p", [0.0, 100.0, 50.0])
def test_percentile_bounds_through_the_c_abi(gpu_ready, p):
    rng = np.random.default_rng(11)
    f = rng.exponential(1.0, (48, 40)).astype(np.float32)
    d = dev_measure(f, [10.0, 20.0], percentile=p, capacity=f.size)
    r = T.measure(f, [10.0, 20.0], p)
    assert d["count"] == r["count"]
    check_candidates(d, np.stack((r["range"], r["doppler"], r["strength"])), r["idx"], False)


def test_capacity_overflow(gpu_ready):
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import _device_measure, multitarget_tracker
    g = load_golden("tracker_scene")
    frames = (g["frames"].astype(np.float64) / 256.0)[:, :, :40]
    x = np.ascontiguousarray(np.moveaxis(frames, 2, 0), dtype=np.float32)
    small = _device_measure(x, list(g["extent"]), 10, capacity=4)
    assert int(small.counts.max()) > 4
    c = small.candidates()
    for i in (0, 17, 39):                               # the first `capacity` candidates, in order
        r = T.measure(x[i], list(g["extent"]))
        assert np.array_equal(c[i]["index"], r["idx"][:4])
    rec = small.run()
    assert np.array_equal(rec["overflow"][:, 0], (small.counts > 4).astype(np.int32))
    ample = multitarget_tracker(frames, list(g["extent"]), 10)
    check_history(history_of(ample), {k: g[k][:40] for k in ("status", "lifetime", "history", "measurement",
                                                              "estimate", "x", "P", "S")})
    assert _lib.TRACK_RECORD_DTYPE.itemsize == 256


def published_batch(torch, N=1199, H=1024, W=177):
    """the published batch on the device: exponential clutter and three targets moving as the tracker's model says
    (range rate -0.003 km per Hz per frame)"""
    ext = [250.0, 300.0]
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = -torch.log1p(-torch.rand((N, H, W), generator=gen, device="cuda", dtype=torch.float32) * 0.999999)
    dpts = np.linspace(-ext[0], ext[0], H)
    rpts = np.linspace(ext[1], 0, W)
    targets = []
    for f0, r0 in ((-20.0, 80.0), (30.0, 250.0), (-5.0, 150.0)):
        t = np.arange(N)
        rr = r0 - 0.003 * f0 * t
        ff = np.full(N, f0)
        w = np.interp(rr, rpts[::-1], np.arange(W)[::-1])
        c = np.interp(ff, dpts, np.arange(H))                 # fliplr column
        h = H - 1 - c
        targets.append((rr, ff, h, w))
    hh = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    ww = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    for (_, _, h, w) in targets:
        th = torch.tensor(h, device="cuda", dtype=torch.float32)[:, None, None]
        tw = torch.tensor(w, device="cuda", dtype=torch.float32)[:, None, None]
        x += 60.0 * torch.exp(-((hh - th) ** 2 / 2.0 + (ww - tw) ** 2 / 1.0))
    return x.contiguous(), ext, targets, (rpts[0] - rpts[1]), (dpts[1] - dpts[0])


def test_published_size(gpu_ready):
    import torch
    from passiveradar_amd.target_detection import _device_measure, _records_to_history
    x, ext, targets, rcell, dcell = published_batch(torch)
    m = _device_measure(x, ext, 10)
    c = m.candidates()
    for i in np.linspace(0, x.shape[0] - 1, 16).astype(int):
        r = T.measure(x[i].cpu().numpy(), ext)
        assert int(m.counts[i]) == r["count"]
        got = c[i][:r["count"]]
        assert np.array_equal(got["index"], r["idx"])
        assert np.array_equal(got["range"], r["range"]) and np.array_equal(got["doppler"], r["doppler"])
        np.testing.assert_allclose(got["strength"], r["strength"], rtol=1e-12, atol=0)
    h = history_of(_records_to_history(m.run(), 10))
    lists = [(c[i]["range"][:int(m.counts[i])], c[i]["doppler"][:int(m.counts[i])]) for i in range(x.shape[0])]
    ref = T.history_arrays(T.track(lists, 10))
    assert np.array_equal(h["status"], ref["status"])
    assert np.array_equal(h["lifetime"], ref["lifetime"]) and np.array_equal(h["hist"], ref["hist"])
    np.testing.assert_allclose(h["estimate"], ref["estimate"], rtol=1e-9, atol=1e-9)
    # every injected target is followed by a confirmed track, within 2 cells, after a warm-up (the reference's gates
    # span tens of Doppler cells at this resolution, so further confirmed tracks ride on clutter: not checked)
    for rr, ff, _, _ in targets:
        on = [any(h["status"][t, j] == 2 and abs(h["estimate"][t, j, 0] - rr[t]) <= 2 * rcell
                  and abs(h["estimate"][t, j, 1] - ff[t]) <= 2 * dcell for j in range(10))
              for t in range(50, x.shape[0])]
        assert np.mean(on) >= 0.9, np.mean(on)


def test_track_maps_is_cfar_then_tracker(gpu_ready):
    import torch
    from passiveradar_amd.target_detection import CFAR_2D_abs, multitarget_tracker, track_maps
    gen = torch.Generator(device="cuda").manual_seed(3)
    N, H, W = 48, 256, 64
    xr = torch.randn((N, H, W), generator=gen, device="cuda")
    xi = torch.randn((N, H, W), generator=gen, device="cuda")
    t = torch.arange(N, device="cuda")
    xr[t, 100 + t // 8, 30] += 40.0
    xr[t, 180, 40 - t // 12] += 30.0
    x = torch.complex(xr, xi)
    a = track_maps(x, [100.0, 80.0], 10)
    b = multitarget_tracker(CFAR_2D_abs(x, 18, 4), [100.0, 80.0], 10)
    assert a.tobytes() == b.tobytes()
    assert (a["status"] == 2).any()


def test_track_maps_numpy_input_matches_the_torch_chain(gpu_ready):
    """track_maps' numpy branch (script layout (H, W, Nframes), its own staging) against the torch chain"""
    import torch
    from passiveradar_amd.target_detection import CFAR_2D, CFAR_2D_abs, multitarget_tracker, track_maps
    rng = np.random.default_rng(21)
    N, H, W = 24, 128, 48
    x = (rng.standard_normal((H, W, N)) + 1j * rng.standard_normal((H, W, N))).astype(np.complex64)
    for t in range(N):
        x[40 + t // 6, 20, t] += 30.0
    a = track_maps(x, [100.0, 80.0], 10)
    xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 2, 0))).cuda()
    b = multitarget_tracker(CFAR_2D_abs(xt, 18, 4), [100.0, 80.0], 10)
    assert a.tobytes() == b.tobytes()
    mag = np.abs(x)                                           # a real magnitude stack takes CFAR_2D
    c = track_maps(mag, [100.0, 80.0], 10)
    magt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(mag, 2, 0))).cuda()
    assert c.tobytes() == multitarget_tracker(CFAR_2D(magt, 18, 4), [100.0, 80.0], 10).tobytes()


def test_wrapper_rebuilds_a_small_starting_capacity(gpu_ready):
    """starting below the counts, the wrapper rebuilds the plan at the exact maximum and measures again: the tracker's
    records equal those of a run that started with ample capacity, bit for bit, and carry no overflow"""
    from passiveradar_amd.target_detection import _device_measure
    g = load_golden("tracker_scene")
    x = np.ascontiguousarray(np.moveaxis(g["frames"].astype(np.float64) / 256.0, 2, 0), dtype=np.float32)
    small = _device_measure(x, list(g["extent"]), 10, start_capacity=4)
    assert small.rebuilt and small.capacity == int(small.counts.max()) > 4
    ample = _device_measure(x, list(g["extent"]), 10)
    assert not ample.rebuilt
    a, b = small.run(), ample.run()
    assert not a["overflow"].any()
    assert a.tobytes() == b.tobytes()


def test_tie_run_beyond_the_lds_bound_of_the_tracker(gpu_ready):
    """a frame of more than 2^19 cells whose threshold is 0: every cell is a candidate, the wrapper's plan is rebuilt at
    capacity n > 2^19 and the tracker's per-candidate bits live in the plan's workspace"""
    from passiveradar_amd.target_detection import _device_measure, _records_to_history
    H, W = 1024, 640
    x = np.zeros((2, H, W), np.float32)
    x[:, 300, 100] = 9.0
    x[0, 700, 400] = 7.0
    x[1, 702, 401] = 7.5
    ext = [200.0, 300.0]
    m = _device_measure(x, ext, 10)
    assert m.rebuilt and m.capacity == H * W > (1 << 19)
    c = m.candidates()
    lists = []
    for i in range(2):
        r = T.measure(x[i], ext)
        assert int(m.counts[i]) == r["count"] == H * W
        assert np.array_equal(c[i]["index"], r["idx"])
        assert np.array_equal(c[i]["range"], r["range"]) and np.array_equal(c[i]["doppler"], r["doppler"])
        lists.append((r["range"], r["doppler"]))
    h = history_of(_records_to_history(m.run(), 10))
    ref = T.history_arrays(T.track(lists, 10))
    assert np.array_equal(h["status"], ref["status"]) and np.array_equal(h["hist"], ref["hist"])
    np.testing.assert_allclose(h["x"], ref["x"], rtol=1e-9, atol=1e-9)
