"""simple_target_tracker / simple_track_maps / persistence on the MI355X against the reference's goldens and the NumPy
restatement (tests/simple_tracker_oracle.py): golden scenes and edge frames in float64, float32 and device tensors, a run
resumed with state=, the published size, and persistence bitwise."""
import numpy as np
import pytest

import simple_tracker_oracle as O
from conftest import load_golden
from test_simple_tracker_host import STRACK, check_strack, persistence_cases, strack_frames

pytestmark = pytest.mark.gpu


def arrays_of(h):
    ks = h["kalman_state"]
    return dict(lock_mode=h["lock_mode"], measurement=h["measurement"], measurement_idx=h["measurement_idx"],
                estimate=h["estimate"], x=ks["x"], P=ks["P"].reshape(-1, 16), S=ks["S"].reshape(-1, 4))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", STRACK)
def test_simple_target_tracker_matches_the_golden(gpu_ready, name):
    import torch
    from passiveradar_amd.target_detection import simple_target_tracker, target_track_dtype_simple
    g = load_golden(name)
    f = strack_frames(g)
    ext = g["ext"]
    h = simple_target_tracker(f, ext[0], ext[1])                          # float64 numpy, as the script passes it
    assert h.dtype == target_track_dtype_simple and h.shape == (f.shape[2],)
    check_strack(arrays_of(h), g)
    assert np.all(h["range_extent"] == ext[0]) and np.array_equal(h["kalman_state"]["F1"][0], O.F1)
    assert np.array_equal(h["kalman_state"]["Q"][0], O.Q) and np.array_equal(h["kalman_state"]["R"][0], O.R)
    if "q" in g:                                                          # exact in float32 too
        check_strack(arrays_of(simple_target_tracker(f.astype(np.float32), ext[0], ext[1])), g)
        dev = torch.from_numpy(np.ascontiguousarray(np.moveaxis(f, 2, 0), np.float32)).cuda()
        check_strack(arrays_of(simple_target_tracker(dev, ext[0], ext[1])), g)
    dev64 = torch.from_numpy(np.ascontiguousarray(np.moveaxis(f, 2, 0))).cuda()
    check_strack(arrays_of(simple_target_tracker(dev64, ext[0], ext[1])), g)


def test_probe_frames(gpu_ready):
    """the reference's probes: all-zero and NaN frames -> (8, 0), +Inf -> that cell, W <= 16 -> (0, 0)"""
    from passiveradar_amd.target_detection import simple_target_tracker
    f = np.ones((64, 40, 4))
    f[:, :, 0] = 0.0
    f[5, 5, 1] = np.nan
    f[64 - 1 - 30, 20, 2] = np.inf
    f[:, :, 3] = -1.0
    h = simple_target_tracker(f, 100.0, 100.0)
    assert h["measurement_idx"].tolist() == [[8, 0], [8, 0], [20, 30], [0, 0]]
    h = simple_target_tracker(np.zeros((40, 16, 2)), 100.0, 100.0)
    assert h["measurement_idx"].tolist() == [[0, 0], [0, 0]]


def test_resumed_run_equals_one_run(gpu_ready):
    from passiveradar_amd.target_detection import simple_target_tracker
    g = load_golden("strack_walk")
    f = strack_frames(g)
    ext = g["ext"]
    whole = simple_target_tracker(f, ext[0], ext[1])
    a = simple_target_tracker(f[:, :, :37], ext[0], ext[1])
    b = simple_target_tracker(f[:, :, 37:], ext[0], ext[1], state=a[-1])
    both = np.concatenate((a, b))
    for k in ("lock_mode", "measurement", "measurement_idx", "estimate"):
        assert np.array_equal(both[k], whole[k]), k
    for k in ("x", "P", "S"):
        assert np.array_equal(both["kalman_state"][k], whole["kalman_state"][k]), k


def published_scene(N=1199, H=1024, W=177, seed=11):
    """exponential clutter, a target wandering in range and Doppler that fades in and out, a few empty frames"""
    rng = np.random.default_rng(seed)
    f = rng.exponential(1.0, (N, H, W)).astype(np.float32)
    r, c = 90.0, 600.0
    for i in range(N):
        r = min(max(r + rng.normal(0, 0.4), 12), W - 12)
        c = min(max(c + rng.normal(0, 1.0), 40), H - 40)
        if (i // 150) % 4 != 3:
            f[i, H - 1 - int(round(c)), int(round(r))] += 60.0
    f[500] = 0.0
    f[501, 3, 3] = np.nan
    return f


def test_published_size_matches_the_restatement(gpu_ready):
    import torch
    from passiveradar_amd.target_detection import simple_target_tracker
    f = published_scene()
    ext = (375.0, 256 / 1.092)
    h = simple_target_tracker(torch.from_numpy(f).cuda(), *ext)
    o = O.simple_target_tracker(np.moveaxis(f, 0, 2), *ext)
    assert np.abs(o["badness"] - 12).min() > 1e-6
    check_strack(arrays_of(h), o)
    assert len(np.unique(np.argmax(o["lock_mode"], axis=1))) == 4


def test_simple_track_maps_equals_cfar_then_tracker(gpu_ready):
    import torch
    from passiveradar_amd.target_detection import CFAR_2D_abs, simple_target_tracker, simple_track_maps
    rng = np.random.default_rng(3)
    N, H, W = 40, 256, 64
    x = (rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))).astype(np.complex64)
    for i in range(N):
        x[i, 100 + i // 4, 30] += 12.0
    xd = torch.from_numpy(x).cuda()
    chain = simple_track_maps(xd, 300.0, 200.0)
    ref = simple_target_tracker(CFAR_2D_abs(xd, 18, 4), 300.0, 200.0)
    assert chain.tobytes() == ref.tobytes()
    host = simple_track_maps(np.moveaxis(x, 0, 2), 300.0, 200.0)        # numpy (H, W, N) as the script loads it
    assert host.tobytes() == ref.tobytes()


def test_persistence_matches_the_golden_bitwise(gpu_ready):
    import torch
    from passiveradar_amd.plotting_tools import persistence
    n = 0
    for X, k, hold, decay, out in persistence_cases():
        got = persistence(X, k, hold, decay)
        assert got.dtype == np.float64 and same_bits(got, out), (X.dtype, k, hold, decay)
        dev = persistence(torch.from_numpy(np.ascontiguousarray(np.moveaxis(X, 2, 0))).cuda(), k, hold, decay)
        assert same_bits(dev.cpu().numpy(), out), (X.dtype, k, hold, decay)
        n += 1
    assert n == 240


def test_persistence_edges(gpu_ready):
    from passiveradar_amd.plotting_tools import persistence
    X = np.ones((3, 2, 4), np.float32)
    with pytest.raises(IndexError):
        persistence(X, 4, 2, 0.9)
    assert np.array_equal(persistence(X, 4, 0, 0.9), np.zeros((3, 2)))
    assert np.array_equal(persistence(X, -3, 5, 0.9), np.zeros((3, 2)))
    # a NumPy float64 decay is not a weak scalar: float64 products, as the reference forms them
    got = persistence(X * np.float32(0.1), 3, 4, np.float64(0.9))
    assert same_bits(got, O.persistence(X * np.float32(0.1), 3, 4, 0.9, weak=False))


def test_persistence_stack_equals_the_per_k_calls(gpu_ready):
    import torch
    from passiveradar_amd.plotting_tools import persistence, persistence_stack
    rng = np.random.default_rng(9)
    X = rng.exponential(1.0, (33, 21, 40)).astype(np.float32)
    for hold, decay in ((20, 0.9), (1, 0.5), (100, -0.5), (300, 0.999)):
        st = persistence_stack(X, hold, decay)
        assert st.shape == X.shape and st.dtype == np.float64
        for k in range(X.shape[2]):
            assert same_bits(st[:, :, k], persistence(X, k, hold, decay)), (hold, k)
            assert same_bits(st[:, :, k], O.persistence(X, k, hold, decay)), (hold, k)
        s32 = persistence_stack(X, hold, decay, out_dtype=np.float32)
        assert s32.dtype == np.float32 and np.array_equal(s32, st.astype(np.float32))
    # more than one launch of terms (300 > 256) into a float64 out
    X64 = rng.standard_normal((5, 4, 300))
    st = persistence_stack(torch.from_numpy(np.ascontiguousarray(np.moveaxis(X64, 2, 0))).cuda(), 300, 0.99)
    for k in (0, 255, 256, 299):
        assert same_bits(st[k].cpu().numpy(), O.persistence(X64, k, 300, 0.99)), k


def test_persistence_stack_published_size(gpu_ready):
    import torch
    from passiveradar_amd.plotting_tools import persistence_stack
    L, H, W = 1199, 1024, 177
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((L, H, W), generator=gen, device="cuda", dtype=torch.float32)
    st = persistence_stack(x, 20, 0.9)
    assert st.shape == (L, H, W) and st.dtype == torch.float64
    rows = np.random.default_rng(2).integers(0, H, 3)
    for k in (0, 7, 19, 20, 600, L - 1):
        xs = x[max(0, k - 19):k + 1, rows, :].cpu().numpy()              # (n, 3, W): only the frames the sum reads
        want = O.persistence(np.moveaxis(xs, 0, 2), xs.shape[0] - 1, 20, 0.9)
        assert same_bits(st[k, rows, :].cpu().numpy(), want), k
