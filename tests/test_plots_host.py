"""Plot extraction without a GPU: the oracle (tests/plots_oracle.py) against scipy's labelling and against get_measurements'
axes, the scene the feature exists for on the oracle alone, the argument checks (host arithmetic) and the ABI layout."""
import numpy as np
import pytest

import cfar_os_oracle as OS
import plots_oracle as PO
import tracker_oracle as T

EXT = [250.0, 300.0]


def same_partition(a, b):
    """two label maps describe the same partition of the same mask"""
    if not np.array_equal(a > 0, b > 0):
        return False
    pairs = {(int(u), int(v)) for u, v in zip(a[a > 0].ravel(), b[a > 0].ravel())}
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("density", [0.05, 0.3, 0.6])
@pytest.mark.parametrize("shape", [(9, 17), (24, 40)])
def test_labelling_matches_scipy(shape, density, connectivity):
    from scipy import ndimage
    rng = np.random.default_rng(int(1000 * density) + shape[0] + connectivity)
    for _ in range(4):
        mask = rng.random(shape) < density
        want, n = ndimage.label(mask, structure=np.ones((3, 3)) if connectivity == 8 else None)
        got = PO.label(mask, connectivity)
        assert got.max() == n and same_partition(got, want)


def test_same_partition_tells_partitions_apart():
    a = np.array([[1, 1, 0, 2]])
    assert same_partition(a, np.array([[5, 5, 0, 3]]))
    assert not same_partition(a, np.array([[1, 2, 0, 3]])) and not same_partition(a, np.array([[1, 1, 0, 1]]))
    assert not same_partition(a, np.array([[1, 1, 1, 2]]))


@pytest.mark.parametrize("guards", [(0, 0), (8, 4)])
def test_isolated_cells_sit_on_get_measurements_axes(guards):
    H, W = 33, 130
    stat = np.zeros((H, W), np.float32)
    cells = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (5, 9), (20, 77), (31, 120), (16, 64), (10, 8), (12, 121)]
    for k, (h, w) in enumerate(cells):
        stat[h, w] = 2.0 + k
    p = PO.plots(stat, 1.0, EXT, connectivity=8, range_guard=guards[0], doppler_guard=guards[1])
    det = PO.detections(stat, 1.0, *guards)
    kept = [(h, w) for h, w in cells if det[h, w]]
    assert p["count"] == p["ncells_total"] == len(kept) and (guards != (0, 0) or len(kept) == len(cells))
    rpts, dpts = T.linspace(EXT[1], 0, W), T.linspace(-EXT[0], EXT[0], H)
    by_peak = {int(pk): k for k, pk in enumerate(p["peak"])}
    for h, w in kept:
        k = by_peak[h * W + w]
        assert p["index"][k] == w * H + (H - 1 - h) and p["ncells"][k] == 1
        assert abs(p["range"][k] - rpts[w]) <= 1e-12 * EXT[1]
        assert abs(p["doppler"][k] - dpts[H - 1 - h]) <= 1e-12 * EXT[0]
        assert (p["hbar"][k], p["wbar"][k], p["strength"][k]) == (h, w, stat[h, w])
    assert np.all(np.diff(p["strength"]) < 0)


DEMO_TARGETS = ((20, 30), (40, 60), (50, 20))
DEMO_SEED = 1


def demo_scene(seed=DEMO_SEED, nframes=20, H=64, W=96):
    """unit complex Gaussian noise plus three 3 x 3 targets 12 exp(-0.35 d^2)"""
    rng = np.random.default_rng(seed)
    x = ((rng.standard_normal((nframes, H, W)) + 1j * rng.standard_normal((nframes, H, W))) * np.sqrt(0.5)).astype(np.complex64)
    for h0, w0 in DEMO_TARGETS:
        for dh in (-1, 0, 1):
            for dw in (-1, 0, 1):
                x[:, h0 + dh, w0 + dw] += np.float32(12.0 * np.exp(-0.35 * (dh * dh + dw * dw)))
    return x


def test_demonstration_scene():
    """20 frames of 64 x 96: OS-CFAR (18, 4), plain scale, at the threshold for Pfa = 1e-4, default guards, connectivity 8,
    weights |X|: every target yields 9 detecting cells and exactly one plot in every frame, its centroid within 0.1 cell of
    the truth"""
    from passiveradar_amd.target_detection import os_cfar_threshold
    x = demo_scene()
    thr = os_cfar_threshold(1e-4, 299, 225)
    false_plots, worst = [], 0.0
    for f in range(x.shape[0]):
        mag = np.abs(x[f])
        stat = OS.CFAR_2D_OS(mag, 18, 4, scale="plain").astype(np.float32)
        p = PO.plots(stat, thr, EXT, weight=mag)
        lab = p["labels"]
        mine = set()
        for h0, w0 in DEMO_TARGETS:
            block = lab[h0 - 1:h0 + 2, w0 - 1:w0 + 2]
            assert (block > 0).all(), (f, h0, w0)                      # 9 detecting cells ...
            assert len(set(block.ravel().tolist())) == 1, (f, h0, w0)  # ... in exactly one plot
            k = [j for j in range(p["count"]) if lab.ravel()[p["peak"][j]] == block[0, 0]]
            assert len(k) == 1
            k = k[0]
            mine.add(k)
            assert p["ncells"][k] == 9, (f, h0, w0, p["ncells"][k])
            err = max(abs(p["hbar"][k] - h0), abs(p["wbar"][k] - w0))
            worst = max(worst, err)
            assert err <= 0.1, (f, h0, w0, err)
        assert len(mine) == 3
        false_plots.append(p["count"] - 3)
    print(f"demonstration: {np.mean(false_plots):.2f} false plots per frame, worst centroid error {worst:.3f} cell")
    assert np.mean(false_plots) < 2.0          # Pfa 1e-4 on 64 x 96 cells less the guards: about 0.5 expected


def test_argument_errors_need_no_device():
    from passiveradar_amd.target_detection import extract_plots, track_maps
    s = np.ones((24, 40), np.float32)
    bad = [dict(connectivity=5), dict(range_guard=-1), dict(doppler_guard=-1), dict(max_cells=0), dict(capacity=0),
           dict(max_cells=-3), dict(weight=np.ones((24, 41), np.float32)), dict(weight=np.ones((2, 24, 40), np.float32))]
    for kw in bad:
        with pytest.raises(ValueError):
            extract_plots(s, 0.5, EXT, **kw)
    with pytest.raises(ValueError):
        extract_plots(s, float("nan"), EXT)
    for shape in ((40,), (1, 40), (24, 1), (2, 1, 40), (2, 3, 4, 5)):
        with pytest.raises(ValueError):
            extract_plots(np.ones(shape, np.float32), 0.5, EXT)
    x = np.ones((24, 40, 3), np.complex64)
    with pytest.raises(ValueError):
        track_maps(x, EXT, 4, measure="plots")
    with pytest.raises(ValueError):
        track_maps(x, EXT, 4, measure="clusters", plot_thresh=2.0)
    with pytest.raises(ValueError):
        track_maps(x, EXT, 4, measure="plots", plot_thresh=2.0, plot_connectivity=6)


def test_c_abi_argument_errors_need_no_device():
    """the same through the C ABI: PRC_EINVAL / PRC_ESHAPE from host arithmetic, nframes == 0 a no-op"""
    import ctypes
    from passiveradar_amd import _lib, engine
    lib = _lib.lib()

    def rc(**kw):
        d = engine.plots_desc(kw.pop("H", 24), kw.pop("W", 40), kw.pop("thresh", 1.0), EXT, **kw)
        nb = ctypes.c_size_t(7)
        return lib.prc_plots_workspace_bytes(ctypes.byref(d), 3, ctypes.byref(nb)), nb.value, d

    assert rc()[:2] == (_lib.PRC_OK, 0)
    assert rc(H=33, W=130, max_cells=_lib.PLOTS_LDS_CELLS)[:2] == (_lib.PRC_OK, 0)
    assert rc(H=33, W=130, max_cells=_lib.PLOTS_LDS_CELLS + 1)[:2] == (_lib.PRC_OK, 3 * 20 * 8192)
    assert rc(H=1)[0] == _lib.PRC_ESHAPE and rc(W=1)[0] == _lib.PRC_ESHAPE and rc(H=65536, W=65536)[0] == _lib.PRC_ESHAPE
    for kw in (dict(connectivity=5), dict(range_guard=-1), dict(doppler_guard=-2), dict(max_cells=0), dict(capacity=0),
               dict(thresh=float("nan"))):
        assert rc(**kw)[0] == _lib.PRC_EINVAL, kw
    d = rc()[2]
    assert lib.prc_plots(ctypes.byref(d), None, None, 0, None, None, None, None, None, None) == _lib.PRC_OK
    assert lib.prc_plots(ctypes.byref(d), None, None, 2, None, None, None, None, None, None) == _lib.PRC_EINVAL
    assert lib.prc_plots(ctypes.byref(d), None, None, -1, None, None, None, None, None, None) == _lib.PRC_EINVAL
    d.struct_size = 40
    assert lib.prc_plots(ctypes.byref(d), None, None, 0, None, None, None, None, None, None) == _lib.PRC_EINVAL


def test_descriptors_match_the_header(tmp_path):
    """sizeof / offsetof of prc_plots_desc and prc_plot_info as gcc lays them out == the ctypes mirrors; both symbols are
    declared and exported"""
    import ctypes
    import shutil
    import subprocess
    from conftest import REPO
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    dfields = [n for n, _ in _lib.PlotsDesc._fields_]
    ifields = [n for n, _ in _lib.PlotInfo._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(prc_plots_desc, {n}));\n' for n in dfields)
    body += "".join(f'  printf("%zu\\n", offsetof(prc_plot_info, {n}));\n' for n in ifields)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  printf("%zu %zu %u %u %d\\n", sizeof(prc_plots_desc), sizeof(prc_plot_info), PRC_PLOTS_DESC_SIZE_MIN,\n'
                   '         PRC_PLOT_INFO_SIZE, PRC_PLOTS_LDS_CELLS);\n' + body + '  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    D, I = _lib.PlotsDesc, _lib.PlotInfo
    assert [int(v) for v in lines[0].split()] == [ctypes.sizeof(D), ctypes.sizeof(I), ctypes.sizeof(D), 48, _lib.PLOTS_LDS_CELLS]
    assert _lib.PLOTS_LDS_CELLS >= 4096
    want = [getattr(D, n).offset for n in dfields] + [getattr(I, n).offset for n in ifields]
    assert [int(v) for v in lines[1:]] == want
    assert _lib.PLOT_INFO_DTYPE.itemsize == 48
    assert [_lib.PLOT_INFO_DTYPE.fields[n][1] for n in ifields] == [getattr(I, n).offset for n in ifields]
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("prc_plots_workspace_bytes", "prc_plots"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(handle, sym)
