"""prc_tbd / prc_tbd_trace on the GPU against tests/tbd_oracle.py: score and back are bit-identical to the oracle in every
case (TO.same_bits: where both are NaN only that is compared -- IEEE 754 leaves the sign and payload of a produced NaN
open), in the time-blocked form at every K and band height and in the one-frame-per-launch form, whole and split, eager and
captured; paths equal the oracle's; the tbd_maps chain equals its stages run one by one through the oracles.
The recursion is causal, so the oracle of the longest stack is the oracle of every shorter one: it is computed once per case."""
import numpy as np
import pytest

import plots_oracle as PO
import tbd_oracle as TO

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (16, 64), (17, 65), (33, 130)]
REACHES = [(0, 0), (1, 1), (2, 3), (1, 5)]
ALPHAS = [1.0, 0.9, 0.5]
I32 = np.iinfo(np.int32)


def shipped_k():
    from passiveradar_amd import _lib
    return _lib.TBD_FRAMES


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(stat, reach, alpha, shifts=None, prev=None, clip=None, guards=(0, 0), want_back=True, frames_per_launch=None,
        band_rows=None):
    """one prc_tbd call on device tensors: (score, back) as NumPy"""
    import torch
    from passiveradar_amd import _lib, engine
    N, H, W = stat.shape
    d = engine.tbd_desc(H, W, alpha, reach[0], reach[1], clip, guards[0], guards[1])
    x, s, p = dev(stat), dev(shifts), dev(prev)
    score = torch.full((N, H, W), 7.0, dtype=torch.float32, device="cuda")
    back = torch.full((N, H, W), 77, dtype=torch.uint8, device="cuda") if want_back else None
    engine.tbd_execute(d, x, s, p, N, score, back, _lib.torch_stream_ptr(), frames_per_launch, band_rows)
    torch.cuda.synchronize()
    return score.cpu().numpy(), (back.cpu().numpy() if want_back else None)


def shift_kinds(H, W, qr, rng):
    alt = np.where(np.arange(H) % 2 == 0, I32.max, I32.min).astype(np.int32)
    return {"none": None,
            "ramp": np.rint(np.linspace(-3, 3, H)).astype(np.int32),
            "random": rng.integers(-4, 5, H).astype(np.int32),
            "at W": (W + np.arange(H) % 2).astype(np.int32),          # every entry >= W: only dw > 0 can reach back in bounds
            "beyond": (W + qr + np.arange(H)).astype(np.int32),       # >= W + qr: no predecessor in bounds, back is all 255
            "int32 max": np.full(H, I32.max, np.int32),
            "int32 min": np.full(H, I32.min, np.int32),
            "alternating extremes": alt}


def assert_same(got, want, what):
    gs, gb = got
    ws, wb = want
    assert TO.same_bits(gs, ws), f"{what}: score differs in {int((gs.view(np.uint32) != ws.view(np.uint32)).sum())} cell(s)"
    if gb is not None:
        assert np.array_equal(gb, wb), f"{what}: back differs in {int((gb != wb).sum())} cell(s)"


@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_grid(gpu_ready, shape, reach):
    """every shift kind x every alpha x nframes 1, 2, K, K + 1, 2 K + 3 (Rayleigh noise; guards and clip alternate)"""
    H, W = shape
    K = shipped_k()
    lengths = [1, 2, K, K + 1, 2 * K + 3]
    rng = np.random.default_rng(H * 1000 + W * 10 + reach[0] * 3 + reach[1])
    stat = rng.rayleigh(1.0, (max(lengths), H, W)).astype(np.float32)
    n = 0
    for name, shifts in shift_kinds(H, W, reach[1], rng).items():
        for alpha in ALPHAS:
            guards, clip = ((0, 0), (8, 4))[n % 2], (None, 2.0)[(n // 2) % 2]
            n += 1
            want = TO.tbd(stat, reach[0], reach[1], alpha, np.inf if clip is None else clip, guards[0], guards[1], shifts)
            if name in ("beyond", "int32 max", "int32 min", "alternating extremes") or (name == "at W" and reach[1] == 0):
                assert (want[1] == TO.NONE).all()
            for N in lengths:
                got = run(stat[:N], reach, alpha, shifts, clip=clip, guards=guards)
                assert_same(got, (want[0][:N], want[1][:N]), f"{name}, alpha {alpha}, {N} frames, guards {guards}, clip {clip}")


def input_kinds(N, H, W, rng):
    ray = rng.rayleigh(1.0, (N, H, W)).astype(np.float32)
    special = ray.copy()
    flat = special.reshape(N, -1)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for f in range(N):
            flat[f, rng.choice(H * W, 6, replace=False)] = v
    special[1, 2:4, :] = -np.inf                                       # whole rows without a predecessor worth choosing
    special[2, :, 3] = np.nan
    return {"rayleigh": ray,
            "quantised": rng.integers(0, 3, (N, H, W)).astype(np.float32),      # full of ties: the smallest code wins
            "constant": np.full((N, H, W), 1.25, np.float32),
            "special": special,
            "2^40": ray * np.float32(2.0 ** 40),
            "2^-40": ray * np.float32(2.0 ** -40)}


@pytest.mark.parametrize("reach", [(1, 1), (2, 3)])
@pytest.mark.parametrize("shape", [(17, 65), (33, 130)])
def test_inputs_and_options(gpu_ready, shape, reach):
    H, W = shape
    N = shipped_k() + 2
    rng = np.random.default_rng(H + W + reach[1])
    shifts = rng.integers(-4, 5, H).astype(np.int32)
    for name, stat in input_kinds(N, H, W, rng).items():
        scale = float(np.nanmax(np.abs(np.where(np.isfinite(stat), stat, 0))))
        for clip in (None, 1.5 * scale / 4):
            for guards in ((8, 4), (0, 0)):
                want = TO.tbd(stat, reach[0], reach[1], 0.9, np.inf if clip is None else clip, guards[0], guards[1], shifts)
                what = f"{name}, clip {clip}, guards {guards}"
                for form in (None, 1):
                    assert_same(run(stat, reach, 0.9, shifts, clip=clip, guards=guards, frames_per_launch=form), want, what)
                got = run(stat, reach, 0.9, shifts, clip=clip, guards=guards, want_back=False)       # back NULL
                assert_same(got, want, what + ", no back")
        if name == "special":
            nan_in = np.isnan(stat) & ~TO.excluded(H, W, 0, 0)
            assert np.isnan(want[0][nan_in]).all()                       # a NaN stays in its own cell's score ...
            later = np.isnan(want[0][1:]) & ~np.isnan(stat[1:])
            inf_clash = np.isinf(stat[1:]) & later                       # ... and only Inf - Inf makes a new one
            assert np.array_equal(later, inf_clash)
        if name == "quantised":
            assert len(np.unique(want[1][1:])) > 3


def test_constant_map_and_ties(gpu_ready):
    """a constant map is all ties: every cell takes its smallest in-bounds code"""
    stat = np.ones((3, 5, 7), np.float32)
    score, back = run(stat, (1, 1), 0.5)
    assert back[1, 0, 0] == 4 and back[1, 2, 3] == 0 and back[1, 0, 3] == 3 and back[1, 2, 0] == 1 and (back[0] == 255).all()
    assert (score[1] == 1.5).all() and (score[2] == 1.75).all()


@pytest.mark.parametrize("reach", [(1, 1), (2, 3), (0, 0)])
def test_split_with_prev_equals_whole(gpu_ready, reach):
    """a stack run whole == the same stack split at every frame boundary with prev carried over"""
    rng = np.random.default_rng(11)
    N, H, W = 7, 17, 65
    stat = rng.rayleigh(1.0, (N, H, W)).astype(np.float32)
    shifts = rng.integers(-4, 5, H).astype(np.int32)
    whole = run(stat, reach, 0.9, shifts, guards=(8, 4))
    assert_same(whole, TO.tbd(stat, reach[0], reach[1], 0.9, row_shift=shifts), "whole")
    for cut in range(1, N):
        for form in (None, 1):
            a = run(stat[:cut], reach, 0.9, shifts, guards=(8, 4), frames_per_launch=form)
            b = run(stat[cut:], reach, 0.9, shifts, prev=a[0][-1], guards=(8, 4), frames_per_launch=form)
            got = (np.concatenate((a[0], b[0])), np.concatenate((a[1], b[1])))
            assert_same(got, whole, f"cut at {cut}, form {form}")
    # prev of any content, NaN and Inf included, is I_{-1}
    prev = rng.rayleigh(1.0, (H, W)).astype(np.float32)
    prev[3, 5], prev[4, 6], prev[9, :] = np.nan, np.inf, -np.inf
    want = TO.tbd(stat[:3], reach[0], reach[1], 0.9, row_shift=shifts, prev=prev)
    for form in (None, 1):
        assert_same(run(stat[:3], reach, 0.9, shifts, prev=prev, guards=(8, 4), frames_per_launch=form), want, f"prev, form {form}")


@pytest.mark.parametrize("reach", [(1, 1), (2, 3), (1, 5), (0, 0)])
def test_forms_agree(gpu_ready, reach):
    """the blocked form at every K and band height == the one-frame-per-launch form == the oracle; repeated runs give the
    same bytes"""
    from passiveradar_amd import _lib
    rng = np.random.default_rng(13)
    N, H, W = 2 * shipped_k() + 3, 33, 130
    stat = rng.integers(0, 4, (N, H, W)).astype(np.float32) + rng.integers(0, 2, (N, H, W)).astype(np.float32) * np.float32(0.5)
    shifts = rng.integers(-4, 5, H).astype(np.int32)
    prev = rng.rayleigh(1.0, (H, W)).astype(np.float32)
    want = TO.tbd(stat, reach[0], reach[1], 0.9, 3.0, 8, 4, shifts, prev)
    forms = [(1, None), (None, None), (2, None), (3, 1), (5, 7), (shipped_k(), 33), (shipped_k(), 4096), (_lib.TBD_FRAMES_MAX, None),
             (_lib.TBD_FRAMES_MAX, 2)]
    first = None
    for K, B in forms:
        for rep in range(2):
            got = run(stat, reach, 0.9, shifts, prev, 3.0, (8, 4), frames_per_launch=K, band_rows=B)
            assert_same(got, want, f"frames per launch {K}, band rows {B}")
            raw = got[0].tobytes() + got[1].tobytes()
            first = first or raw
            assert raw == first, f"frames per launch {K}, band rows {B}, run {rep}: bytes differ from the first run"
    assert _lib.get_option(_lib.OPT_TBD_FRAMES) == 0 and _lib.get_option(_lib.OPT_TBD_ROWS) == 0


@pytest.mark.parametrize("case", ["too wide for two frames", "K lowered to what LDS holds"])
def test_wide_frames(gpu_ready, case):
    """the thresholds between the forms: 8 (W + 2 qr)(1 + 4 qd) > PRC_TBD_LDS_BYTES runs one frame per launch; just below, the
    blocked form runs with fewer frames per launch than shipped"""
    from passiveradar_amd import _lib
    (H, W), reach = ((3, 4000), (1, 1)) if case == "too wide for two frames" else ((12, 2000), (2, 0))
    rows = _lib.TBD_LDS_BYTES // (8 * (W + 2 * reach[1]))
    assert (rows < 1 + 4 * reach[0]) == (case == "too wide for two frames") and rows < 1 + 2 * shipped_k() * reach[0]
    rng = np.random.default_rng(17)
    stat = rng.rayleigh(1.0, (5, H, W)).astype(np.float32)
    shifts = rng.integers(-40, 41, H).astype(np.int32)
    want = TO.tbd(stat, reach[0], reach[1], 0.9, row_shift=shifts)
    for form in (None, 1):
        assert_same(run(stat, reach, 0.9, shifts, guards=(8, 4), frames_per_launch=form), want, f"{case}, form {form}")


@pytest.mark.parametrize("form", [None, 1])
def test_capture(gpu_ready, form):
    """one prc_tbd call captured on a side stream and replayed on new inputs == the eager bytes"""
    import torch
    from passiveradar_amd import _lib, engine
    rng = np.random.default_rng(19)
    N, H, W = shipped_k() + 3, 33, 130
    stacks = [rng.rayleigh(1.0, (N, H, W)).astype(np.float32) for _ in range(3)]
    shifts = rng.integers(-4, 5, H).astype(np.int32)
    eager = [run(s, (1, 1), 0.9, shifts, guards=(8, 4), frames_per_launch=form) for s in stacks]      # (also the LDS opt-in)
    d = engine.tbd_desc(H, W, 0.9, 1, 1, None, 8, 4)
    xin, sh = dev(stacks[0]).clone(), dev(shifts)
    score = torch.zeros((N, H, W), dtype=torch.float32, device="cuda")
    back = torch.zeros((N, H, W), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.tbd_execute(d, xin, sh, None, N, score, back, _lib.torch_stream_ptr(), form)
    side.synchronize()
    for k in (1, 2, 0):
        xin.copy_(dev(stacks[k]))
        score.zero_()
        back.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same((score.cpu().numpy(), back.cpu().numpy()), eager[k], f"replay on stack {k}")


# ---- trace ----------------------------------------------------------------------------------------------------------------------
def gpu_paths(back, ends, depth, reach, shifts):
    from passiveradar_amd.target_detection import tbd_paths
    return tbd_paths(dev(back), dev(np.asarray(ends, dtype=np.int32)), depth, shifts, doppler_reach=reach[0],
                     range_reach=reach[1]).cpu().numpy()


@pytest.mark.parametrize("reach", [(1, 1), (2, 3)])
def test_trace(gpu_ready, reach):
    rng = np.random.default_rng(23)
    N, H, W = 6, 17, 65
    stat = rng.rayleigh(1.0, (N, H, W)).astype(np.float32)
    for shifts in (None, rng.integers(-4, 5, H).astype(np.int32), np.where(np.arange(H) % 3 == 0, I32.min, 2).astype(np.int32)):
        _, back = run(stat, reach, 0.9, shifts)
        ends = [[f, c] for f in range(N) for c in rng.choice(H * W, 40, replace=False)]
        ends += [[-1, 0], [N, 0], [0, -1], [0, H * W], [I32.max, 5], [I32.min, 5], [2, I32.max], [2, I32.min], [N - 1, H * W - 1], [0, 0]]
        for depth in (1, 3, N, N + 4):
            want = TO.trace(back, ends, depth, reach[0], reach[1], shifts)
            got = gpu_paths(back, ends, depth, reach, shifts)
            assert got.dtype == np.int32 and np.array_equal(got, want), depth
            assert (want[-10:-2] == -1).all() and want[-1, 0] == 0
        # NumPy in, NumPy out
        from passiveradar_amd.target_detection import tbd_paths
        assert np.array_equal(tbd_paths(back, ends, 4, shifts, doppler_reach=reach[0], range_reach=reach[1]),
                              TO.trace(back, ends, 4, reach[0], reach[1], shifts))


def test_trace_of_a_back_array_with_out_of_range_codes(gpu_ready):
    """a `back` that prc_tbd did not write: codes >= ncodes and codes that leave the frame end the path; nothing outside the
    array is read (tests/test_gpu_tbd_bounds.py holds the extents)"""
    rng = np.random.default_rng(29)
    N, H, W = 5, 9, 13
    back = rng.integers(0, 256, (N, H, W)).astype(np.uint8)
    back[:, ::2, ::3] = rng.integers(0, 9, back[:, ::2, ::3].shape).astype(np.uint8)
    ends = [[f, c] for f in range(N) for c in range(H * W)]
    for shifts in (None, rng.integers(-20, 21, H).astype(np.int32), np.full(H, I32.max, np.int32),
                   np.where(np.arange(H) % 2 == 0, I32.max, I32.min).astype(np.int32)):
        want = TO.trace(back, ends, N + 1, 1, 1, shifts)
        assert np.array_equal(gpu_paths(back, ends, N + 1, (1, 1), shifts), want)
    assert (want[:, 1:] == -1).all() and (TO.trace(back, ends, N + 1, 1, 1, None)[:, 1:] >= 0).any()


# ---- public functions and the chain ------------------------------------------------------------------------------------------------
def test_track_before_detect_fronts(gpu_ready):
    from passiveradar_amd.target_detection import track_before_detect
    rng = np.random.default_rng(31)
    stat = rng.rayleigh(1.0, (4, 17, 65)).astype(np.float32)
    shifts = rng.integers(-4, 5, 17).astype(np.int32)
    want = TO.tbd(stat, 1, 2, 0.8, 2.0, 3, 2, shifts)
    kw = dict(alpha=0.8, doppler_reach=1, range_reach=2, row_shifts=shifts, clip=2.0, range_guard=3, doppler_guard=2)
    s, b = track_before_detect(stat, **kw)
    assert isinstance(s, np.ndarray) and s.dtype == np.float32 and b.dtype == np.uint8
    assert_same((s, b), want, "numpy")
    ts, tb = track_before_detect(dev(stat), **kw)
    assert ts.is_cuda and tb.is_cuda
    assert_same((ts.cpu().numpy(), tb.cpu().numpy()), want, "torch")
    s2, b2 = track_before_detect(stat[2:], prev=s[1], return_back=False, **kw)
    assert b2 is None and TO.same_bits(s2, want[0][2:])
    s1, b1 = track_before_detect(stat[0], **kw)                       # one frame
    assert s1.shape == (17, 65) and TO.same_bits(s1, want[0][0]) and (b1 == 255).all()


def chain_scene():
    """10 frames of 33 x 48 complex noise with one echo walking 2 range columns a frame in Doppler row 4"""
    rng = np.random.default_rng(37)
    N, H, W = 10, 33, 48
    x = ((rng.standard_normal((N, H, W)) + 1j * rng.standard_normal((N, H, W))) * np.sqrt(0.5)).astype(np.complex64)
    for k in range(N):
        x[k, 4, 10 + 2 * k] += 4.0
    return x


@pytest.mark.parametrize("cfar", ["os", "mean"])
def test_chain(gpu_ready, cfar):
    """tbd_maps == the device's own CFAR map (held to its oracle by its own tests) through the oracles of the later stages one
    by one: tbd_row_shifts, TO.tbd, PO.plots on the score, TO.trace from the plots' peak cells"""
    from passiveradar_amd.target_detection import CFAR_2D_abs, CFAR_2D_OS, tbd_maps, tbd_row_shifts
    x = chain_scene()
    N, H, W = x.shape
    ext = [250.0, 0.125 * (W - 1)]                                     # 125 m range columns
    shifts = tbd_row_shifts(H, W, ext, 0.5, 3.0)
    assert shifts[4] == 2 and shifts[16] == 0
    xt = dev(x)
    cf = (CFAR_2D_OS(xt, 8, 2, scale="plain") if cfar == "os" else CFAR_2D_abs(xt, 8, 2)).cpu().numpy()
    score, back = TO.tbd(cf, 1, 1, 0.9, row_shift=shifts)
    thresh = float(np.sort(score[1:].ravel())[-300])
    want = [PO.plots(score[f], thresh, ext, range_guard=8, doppler_guard=4) for f in range(N)]
    assert sum(w["count"] for w in want) >= 5
    for front in ("torch", "numpy"):
        arg = xt if front == "torch" else np.moveaxis(x, 0, 2)
        counts, meas, index, paths = tbd_maps(arg, ext, 0.5, 3.0, thresh=thresh, depth=6, fw=8, gw=2, cfar=cfar)
        if front == "torch":
            counts, meas, index, paths = (t.cpu().numpy() for t in (counts, meas, index, paths))
        assert counts.tolist() == [w["count"] for w in want] and paths.shape == (N, index.shape[1], 6) and paths.dtype == np.int32
        hit = False
        for f, w in enumerate(want):
            k = w["count"]
            assert np.array_equal(index[f, :k], w["index"][:k]) and np.array_equal(meas[f, 2, :k], w["strength"][:k])
            assert np.abs(meas[f, 0, :k] - w["range"][:k]).max(initial=0) <= 1e-12 * ext[1]
            assert np.abs(meas[f, 1, :k] - w["doppler"][:k]).max(initial=0) <= 1e-12 * ext[0]
            ends = [[f, int(p)] for p in w["peak"][:k]]
            assert np.array_equal(paths[f, :k], TO.trace(back, ends, 6, 1, 1, shifts).reshape(k, 6))
            assert (paths[f, k:] == -1).all()
            hit = hit or (f == N - 1 and 4 * W + 10 + 2 * f in paths[f, :k, 0])
        assert hit                                                     # the echo's last cell is a plot's peak in the last frame
