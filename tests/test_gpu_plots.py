"""Plot extraction on the MI355X (prc_plots, extract_plots, track_maps(measure="plots")) against tests/plots_oracle.py.

Bars (include/prcore.h states the definition): counts, ncells and per plot index, ncells, box, peak, strength are exact;
mass is relative 1e-12; hbar / wbar / range / doppler are within 1e-12 of the axis length or extent -- what up to 4096
non-negative float64 terms allow in any order (4096 * 2^-52 = 9.1e-13), scaled with max_cells where a test holds more."""
import numpy as np
import pytest

import plots_oracle as PO
import tracker_oracle as T

pytestmark = pytest.mark.gpu

EXT = [250.0, 300.0]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def extract(stat, thresh, front="numpy", weight=None, **kw):
    """extract_plots of a stack through either front end -> (counts, meas, index, info, ncells) as NumPy"""
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import extract_plots
    if front == "torch":
        out = extract_plots(dev(stat), thresh, EXT, weight=None if weight is None else dev(weight), return_info=True, **kw)
        counts, meas, index, info, ncells = (t.cpu().numpy() for t in out)
        info = np.ascontiguousarray(info).view(_lib.PLOT_INFO_DTYPE)[..., 0]
        return counts, meas, index, info, ncells
    return extract_plots(stat, thresh, EXT, weight=weight, return_info=True, **kw)


def check_frame(got, f, want, capacity=None, scale=1.0, shape=None):
    """frame f of an extract() result against the oracle's dict, at the bars of the module docstring"""
    counts, meas, index, info, ncells = got
    H, W = shape
    assert int(ncells[f]) == want["ncells_total"] and int(counts[f]) == want["count"], (f, ncells[f], counts[f], want["count"])
    k = want["count"] if capacity is None else min(want["count"], capacity)
    assert np.array_equal(index[f][:k], want["index"][:k])
    assert np.array_equal(meas[f][2][:k], want["strength"][:k])
    for name in ("ncells", "h0", "h1", "w0", "w1", "peak"):
        assert np.array_equal(info[f][name][:k], want[name][:k]), name
    np.testing.assert_allclose(info[f]["mass"][:k], want["mass"][:k], rtol=1e-12 * scale, atol=0, equal_nan=True)
    for arr, name, span in ((info[f]["hbar"], "hbar", H), (info[f]["wbar"], "wbar", W), (meas[f][0], "range", EXT[1]),
                            (meas[f][1], "doppler", EXT[0])):
        err = np.abs(arr[:k] - want[name][:k]).max() if k else 0.0
        assert err <= 1e-12 * scale * span, (name, err)


def check_stack(stat, thresh, weight=None, fronts=("numpy", "torch"), scale=1.0, **kw):
    okw = {k: v for k, v in kw.items() if k in ("connectivity", "range_guard", "doppler_guard")}
    want = [PO.plots(stat[f], thresh, EXT, None if weight is None else weight[f], **okw) for f in range(stat.shape[0])]
    res = []
    for front in fronts:
        got = extract(stat, thresh, front, weight, **kw)
        for f in range(stat.shape[0]):
            check_frame(got, f, want[f], scale=scale, shape=stat.shape[1:])
        res.append(got)
    return want, res


def same_bytes(a, b):
    return all(np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes() for u, v in zip(a, b))


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["none", "f32", "c64"])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", [(9, 17), (24, 40), (33, 130)])
def test_parity(gpu_ready, shape, connectivity, wkind):
    H, W = shape
    rng = np.random.default_rng(H * 100 + connectivity + len(wkind))
    for density in (0.02, 0.3, 0.6):
        for guards in ((0, 0), (8, 4)):
            if guards != (0, 0) and W <= 16:
                continue
            stat = rng.random((3, H, W)).astype(np.float32)
            weight = None
            if wkind == "f32":
                weight = rng.exponential(1.0, (3, H, W)).astype(np.float32)
            elif wkind == "c64":
                weight = (rng.standard_normal((3, H, W)) + 1j * rng.standard_normal((3, H, W))).astype(np.complex64)
            want, _ = check_stack(stat, 1.0 - density, weight, connectivity=connectivity, range_guard=guards[0],
                                  doppler_guard=guards[1])
            if guards == (0, 0):
                assert abs(want[0]["ncells_total"] - density * H * W) < 5 * np.sqrt(H * W) + 2


def test_single_frame_returns_get_measurements_shape(gpu_ready):
    from passiveradar_amd.target_detection import extract_plots
    rng = np.random.default_rng(2)
    stat = rng.random((24, 40)).astype(np.float32)
    want = PO.plots(stat, 0.9, EXT, range_guard=0, doppler_guard=0)
    m = extract_plots(stat, 0.9, EXT, range_guard=0, doppler_guard=0)
    assert m.shape == (3, want["count"]) and m.dtype == np.float64 and want["count"] > 3
    assert np.array_equal(m[2], want["strength"]) and np.all(np.diff(m[2]) <= 0)
    m2, info, ncells = extract_plots(stat, 0.9, EXT, range_guard=0, doppler_guard=0, return_info=True)
    assert np.array_equal(m, m2) and ncells == want["ncells_total"] and np.array_equal(info["peak"], want["peak"])


# ---- shapes that break labelling ------------------------------------------------------------------------------------------
def serpentine(H=15, W=17):
    m = np.zeros((H, W), bool)
    m[0::2, :] = True
    for k, h in enumerate(range(1, H, 2)):
        m[h, W - 1 if k % 2 == 0 else 0] = True
    return m


def comb(H=15, W=17):
    m = np.zeros((H, W), bool)
    m[:, 0::2] = True
    m[H - 1, :] = True
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["full", "serpentine", "comb", "checkerboard", "diagonal"])
def test_hard_shapes(gpu_ready, name, connectivity):
    if name == "full":
        m = np.ones((24, 40), bool)
    elif name == "serpentine":
        m = serpentine()
    elif name == "comb":
        m = comb()
    elif name == "checkerboard":
        m = (np.add.outer(np.arange(15), np.arange(17)) % 2) == 0
    else:
        m = np.zeros((15, 17), bool)
        m[2:5, 3:6] = True
        m[5:8, 6:9] = True                               # touches the first block at one corner only
    rng = np.random.default_rng(5)
    stat = np.where(m, 1.0 + rng.random(m.shape), 0.0).astype(np.float32)[None]
    want, _ = check_stack(stat, 0.5, connectivity=connectivity, range_guard=0, doppler_guard=0)
    ncomp = {("full", 4): 1, ("full", 8): 1, ("serpentine", 4): 1, ("serpentine", 8): 1, ("comb", 4): 1, ("comb", 8): 1,
             ("checkerboard", 4): int(m.sum()), ("checkerboard", 8): 1, ("diagonal", 4): 2, ("diagonal", 8): 1}
    assert want[0]["count"] == ncomp[(name, connectivity)]
    if name == "full":
        assert want[0]["ncells"][0] == 960


# ---- ties and special values ------------------------------------------------------------------------------------------------
def test_ties(gpu_ready):
    stat = np.zeros((1, 24, 40), np.float32)
    stat[0, 3:6, 4:9] = 2.0                                # a plateau: the peak is its smallest storage index
    stat[0, 10, 10] = stat[0, 12, 30] = stat[0, 20, 5] = stat[0, 2, 38] = 3.0     # equal strengths: descending index
    stat[0, 15:17, 20:22] = 3.0
    want, _ = check_stack(stat, 1.0, range_guard=0, doppler_guard=0)
    w = want[0]
    assert w["count"] == 6 and w["peak"][-1] == 3 * 40 + 4
    assert np.all(w["strength"][:5] == 3.0) and np.all(np.diff(w["index"][:5]) < 0)


def test_special_values(gpu_ready):
    H, W = 24, 40
    stat = np.zeros((4, H, W), np.float32)
    stat[0, 2, 3] = np.nan
    stat[0, 5, 5] = -np.inf
    stat[0, 7, 7] = np.inf
    stat[0, 7, 8] = 5.0
    stat[0, 12, 30] = 9.0
    stat[0, 20, 20:23] = [np.nan, 4.0, np.nan]
    weight = np.ones((4, H, W), np.float32)
    stat[1, 4:6, 4:7] = [[2.0, 3.0, 2.5], [2.0, 2.0, 2.0]]
    weight[1, 4, 4] = np.nan                               # NaN weight: the centroid falls back to the peak cell
    stat[1, 15:17, 15:17] = [[2.0, 2.0], [2.0, 6.0]]
    weight[1, 15:17, 15:17] = 0.0                          # all-zero weights: the same
    stat[2] = -1.0                                         # nothing above the threshold
    stat[3, 9, 9] = 4.0
    want, res = check_stack(stat, 1.0, weight, range_guard=0, doppler_guard=0)
    w0, w1 = want[0], want[1]
    assert w0["count"] == 3 and w0["strength"][0] == np.inf and w0["peak"][0] == 7 * W + 7 and w0["ncells"][0] == 2
    assert w1["count"] == 2 and (w1["hbar"][0], w1["wbar"][0]) == (16, 16) and (w1["hbar"][1], w1["wbar"][1]) == (4, 5)
    assert want[2]["count"] == 0 and want[2]["ncells_total"] == 0 and want[3]["count"] == 1
    # stat as its own weight: a +Inf member makes the mass infinite, the centroid is the peak cell
    want, _ = check_stack(stat[:1], 1.0, None, range_guard=0, doppler_guard=0)
    assert want[0]["mass"][0] == np.inf and (want[0]["hbar"][0], want[0]["wbar"][0]) == (7, 7)
    # a negative threshold: -Inf still never detects, zeros do
    want, _ = check_stack(stat[:1, :9, :17], -0.5, None, range_guard=0, doppler_guard=0)
    assert want[0]["ncells_total"] == 9 * 17 - 2


# ---- bounds --------------------------------------------------------------------------------------------------------------
def bounds_stack():
    rng = np.random.default_rng(8)
    stat = rng.random((3, 33, 130)).astype(np.float32)
    stat[1] += 0.5                                         # frame 1: about 60 % of the cells detect at 0.9
    return stat


def test_frame_over_max_cells(gpu_ready):
    stat = bounds_stack()
    okw = dict(range_guard=0, doppler_guard=0)
    want = [PO.plots(stat[f], 0.9, EXT, **okw) for f in range(3)]
    mc = max(want[0]["ncells_total"], want[2]["ncells_total"])
    assert want[1]["ncells_total"] > mc
    for front in ("numpy", "torch"):
        got = extract(stat, 0.9, front, max_cells=mc, capacity=512, **okw)
        counts, meas, index, info, ncells = got
        assert counts[1] == 0 and ncells[1] == want[1]["ncells_total"]
        assert not meas[1].any() and not index[1].any() and not info[1]["ncells"].any()      # nothing written
        for f in (0, 2):
            check_frame(got, f, want[f], shape=stat.shape[1:])


def test_plots_over_capacity(gpu_ready):
    stat = bounds_stack()
    okw = dict(range_guard=0, doppler_guard=0)
    want = [PO.plots(stat[f], 0.9, EXT, **okw) for f in range(3)]
    assert min(want[0]["count"], want[2]["count"]) > 7
    for front in ("numpy", "torch"):
        got = extract(stat, 0.9, front, capacity=7, **okw)
        assert got[1].shape == (3, 3, 7)
        for f in range(3):
            check_frame(got, f, want[f], capacity=7, shape=stat.shape[1:])


def test_sizing_step_from_small_starting_values(gpu_ready):
    stat = bounds_stack()
    okw = dict(range_guard=0, doppler_guard=0)
    for front in ("numpy", "torch"):
        want, res = check_stack(stat, 0.9, fronts=(front,), start_max_cells=4, start_capacity=1, **okw)
        assert res[0][1].shape[2] == max(w["count"] for w in want)          # the exact maximum
    from passiveradar_amd.target_detection import _device_plots
    m = _device_plots(stat, 0.9, EXT, None, start_max_cells=4, start_capacity=1, **okw)
    assert m.runs == 3 and m.max_cells == max(w["ncells_total"] for w in want) and not m.overflowed()
    assert _device_plots(stat, 0.9, EXT, None, **okw).runs == 1


# ---- both storage paths, determinism ------------------------------------------------------------------------------------------
def test_workspace_path_on_the_all_detecting_frame(gpu_ready):
    from passiveradar_amd import _lib
    rng = np.random.default_rng(4)
    stat = (1.0 + rng.random((1, 33, 130))).astype(np.float32)
    mc = 33 * 130                                          # 4290: above PRC_PLOTS_LDS_CELLS, the least that holds the frame
    assert mc > _lib.PLOTS_LDS_CELLS
    want, _ = check_stack(stat, 0.5, scale=4290 / 4096, max_cells=mc, range_guard=0, doppler_guard=0)
    assert want[0]["count"] == 1 and want[0]["ncells"][0] == 4290
    # the sizing step arrives on the workspace path by itself
    check_stack(stat, 0.5, fronts=("torch",), scale=4290 / 4096, range_guard=0, doppler_guard=0)


def test_both_paths_and_repeated_runs_give_the_same_bytes(gpu_ready):
    from passiveradar_amd import _lib
    rng = np.random.default_rng(6)
    stat = rng.random((3, 33, 130)).astype(np.float32)
    weight = (rng.standard_normal(stat.shape) + 1j * rng.standard_normal(stat.shape)).astype(np.complex64)
    for thresh in (0.98, 0.7):
        want, (lds,) = check_stack(stat, thresh, weight, fronts=("torch",), max_cells=_lib.PLOTS_LDS_CELLS)
        ws = extract(stat, thresh, "torch", weight, max_cells=_lib.PLOTS_LDS_CELLS + 1)
        again = extract(stat, thresh, "torch", weight, max_cells=_lib.PLOTS_LDS_CELLS)
        assert same_bytes(lds, ws) and same_bytes(lds, again)
        assert same_bytes(ws, extract(stat, thresh, "numpy", weight, max_cells=_lib.PLOTS_LDS_CELLS + 1))


# ---- the chain ---------------------------------------------------------------------------------------------------------------
CHAIN_EXT = [100.0, 80.0]


def chain_scene():
    rng = np.random.default_rng(12)
    N, H, W = 40, 32, 64
    x = ((rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))) * np.sqrt(0.5)).astype(np.complex64)
    for t in range(N):
        h0, w0 = 6, 12 + t
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                x[t, h0 + dh, w0 + dw] += np.float32(12.0 * np.exp(-0.35 * (dh * dh + dw * dw)))
    return x


def history_of(h):
    ks = h["kalman_state"]
    return dict(status=h["status"], lifetime=h["lifetime"], measurement=h["measurement"], estimate=h["estimate"],
                hist=h["measurement_history"], x=ks["x"], P=ks["P"], S=ks["S"])


@pytest.mark.parametrize("cfar", ["os", "mean"])
def test_chain(gpu_ready, cfar):
    """track_maps(measure="plots") == the restated tracker fed the oracle's plots of the device's own CFAR map, at the bars
    tests/test_gpu_tracker.py holds the same record fields to"""
    from passiveradar_amd.target_detection import CFAR_2D_abs, CFAR_2D_OS, os_cfar_threshold, track_maps
    x = chain_scene()
    xt = dev(x)
    if cfar == "os":
        thr = os_cfar_threshold(1e-4, 299, 225)
        stat = CFAR_2D_OS(xt, 18, 4, scale="plain").cpu().numpy()
    else:
        thr = 4.0
        stat = CFAR_2D_abs(xt, 18, 4).cpu().numpy()
    lists = []
    for f in range(x.shape[0]):
        p = PO.plots(stat[f], thr, CHAIN_EXT, weight=x[f])
        lists.append((p["range"], p["doppler"]))
    ref = T.history_arrays(T.track(lists, 6))
    assert (ref["status"] > 0).any()
    for arg in (xt, np.moveaxis(x, 0, 2)):
        h = history_of(track_maps(arg, CHAIN_EXT, 6, cfar=cfar, measure="plots", plot_thresh=thr))
        assert np.array_equal(h["status"], ref["status"]) and np.array_equal(h["lifetime"], ref["lifetime"])
        assert np.array_equal(h["hist"], ref["hist"])
        for k in ("measurement", "estimate", "x", "P", "S"):
            np.testing.assert_allclose(h[k], ref[k], rtol=1e-9, atol=1e-9, err_msg=k)


def test_chain_percentile_is_unchanged_and_pinned_bounds_raise(gpu_ready):
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import CFAR_2D_abs, multitarget_tracker, track_maps
    x = chain_scene()
    xt = dev(x)
    a = track_maps(xt, CHAIN_EXT, 6)
    assert a.tobytes() == track_maps(xt, CHAIN_EXT, 6, measure="percentile").tobytes()
    assert a.tobytes() == multitarget_tracker(CFAR_2D_abs(xt, 18, 4), CHAIN_EXT, 6).tobytes()
    assert a.tobytes() == track_maps(np.moveaxis(x, 0, 2), CHAIN_EXT, 6, measure="percentile").tobytes()
    for kw in (dict(plot_max_cells=3), dict(plot_capacity=1)):
        with pytest.raises(_lib.PrcoreError):
            track_maps(xt, CHAIN_EXT, 6, measure="plots", plot_thresh=1.5, **kw)


# ---- capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "workspace"])
def test_capture(gpu_ready, path):
    """one prc_plots call captured on a side stream and replayed on new inputs == the eager results"""
    import torch
    from passiveradar_amd import _lib, engine
    rng = np.random.default_rng(10)
    N, H, W, cap = 3, 33, 130, 64
    frames = [dev(rng.random((N, H, W)).astype(np.float32) * np.float32(s)) for s in (1.0, 1.02, 0.99)]
    wts = [dev((rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))).astype(np.complex64)) for _ in range(3)]
    d = engine.plots_desc(H, W, 0.97, EXT, max_cells=_lib.PLOTS_LDS_CELLS + (path == "workspace"), capacity=cap, complex_weight=True)
    nws = engine.plots_workspace_bytes(d, N)
    assert (nws > 0) == (path == "workspace")
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda") if nws else None

    def outputs():
        return (torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
                torch.zeros(N * cap * 32, dtype=torch.uint8, device="cuda"), torch.zeros(N * cap * 48, dtype=torch.uint8, device="cuda"))

    eager = []
    for x, w in zip(frames, wts):
        o = outputs()
        engine.plots_execute(d, x, w, N, o[0], o[1], o[2], o[3], ws, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        eager.append([t.cpu().numpy().tobytes() for t in o])
    assert eager[0] != eager[1] and eager[1] != eager[2]
    xin, win, o = frames[0].clone(), wts[0].clone(), outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.plots_execute(d, xin, win, N, o[0], o[1], o[2], o[3], ws, _lib.torch_stream_ptr())
    side.synchronize()
    for k in (1, 2):
        xin.copy_(frames[k])
        win.copy_(wts[k])
        for t in o:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert [t.cpu().numpy().tobytes() for t in o] == eager[k], k
