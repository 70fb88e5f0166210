"""batch_xambg / prc_batch_xambg and ofdm_symbol_start / prc_ofdm_timing on the MI355X against the float64 definition of
tests/batch_xambg_oracle.py.

Accuracy bar: GPU_BAR = 2e-6 of the peak, the project's CAF parity bar; a float32 emulation of the definition stays below
1.2e-7 (tests/test_batch_xambg_host.py holds it to a quarter of the bar).  Timing: the metric within 1e-10 of its peak (float64
sums of exact products) and the same argmax.  The shapes are the smallest at which each thing can go wrong: both batch lengths,
every tile width of the Doppler kernel that a shape reaches, a column count that is and is not a multiple of it, overlapping
batches, the widest lag span of each length."""
import numpy as np
import pytest

import batch_xambg_oracle as O

pytestmark = pytest.mark.gpu

BAR = O.GPU_BAR

# (L, F, R, hop, start)
SHAPES = [(1024, 256, 64, 1152, 165), (1024, 512, 0, 1024, 0), (1024, 256, 1023, 700, 0), (4096, 256, 64, 4608, 549),
          (4096, 256, 1030, 4608, 549), (4096, 256, 4095, 4096, 0), (1024, 1024, 7, 1024, 5)]
_inputs, _want = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_resident(gpu_ready):
    yield
    O.release_device_leftovers()


def length(L, F, hop, start):
    return start + (F - 1) * hop + L


def inputs(n, seed=0):
    """a white reference and a surveillance channel with three echoes (one past most lag spans) and noise, computed once"""
    key = (n, seed)
    if key not in _inputs:
        ref = O.white(n, 1000 + seed)
        srv = (0.8 * np.roll(ref, 3) + 0.3 * np.roll(ref, 50) * np.exp(2j * np.pi * 7.3 * np.arange(n) / n) + 0.2 * np.roll(ref, 900)
               + 0.05 * O.white(n, 2000 + seed)).astype(np.complex64)
        ref.setflags(write=False)
        srv.setflags(write=False)
        _inputs[key] = (ref, srv)
    return _inputs[key]


def want(n, seed, **a):
    key = (n, seed, tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in a.items())))
    if key not in _want:
        _want[key] = O.surface(*inputs(n, seed), **a)
        _want[key].setflags(write=False)
    return _want[key]


def dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()                                  # a copy: the shared inputs are read-only


def same_bits(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run(ref, srv, L, F, R, hop, start, filt=O.RECIPROCAL, floor=0.1, window=None):
    from passiveradar_amd.range_doppler_processing import batch_xambg
    X = batch_xambg(ref, srv, R, F, L, hop=hop, start=start, filter=filt, floor=floor, window=window)
    assert X.shape == (F, R + 1, 1) and X.dtype == np.complex64
    return X[:, :, 0]


@pytest.mark.parametrize("filt", [O.RECIPROCAL, O.MATCHED])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d_F%d_R%d_hop%d_start%d" % s)
def test_accuracy(gpu_ready, shape, filt):
    L, F, R, hop, start = shape
    n = length(L, F, hop, start)
    ref, srv = inputs(n)
    got = run(ref, srv, L, F, R, hop, start, filt)
    err = O.rel_err(got, want(n, 0, L=L, F=F, R=R, hop=hop, start=start, filt=filt))
    print(f"batch_xambg {shape} {filt}: {err:.3g}")
    assert np.isfinite(got).all() and err <= BAR, (shape, filt, err)


@pytest.mark.parametrize("L,hop,start", [(1024, 1152, 165), (4096, 4608, 549)])
def test_window_and_floors(gpu_ready, L, hop, start):
    F, R = 256, 40
    n = length(L, F, hop, start)
    ref, srv = inputs(n)
    win = np.kaiser(F, 4.0).astype(np.float32)
    for filt, floor, w in ((O.RECIPROCAL, 0.03, None), (O.RECIPROCAL, 1.0, None), (O.RECIPROCAL, 0.1, win), (O.MATCHED, 0.1, win)):
        got = run(ref, srv, L, F, R, hop, start, filt, floor, w)
        a = dict(L=L, F=F, R=R, hop=hop, start=start, filt=filt, floor=floor)
        err = O.rel_err(got, want(n, 0, window=w, **a) if w is not None else want(n, 0, **a))
        print(f"L = {L} {filt} floor {floor} window {w is not None}: {err:.3g}")
        assert err <= BAR, (L, filt, floor, err)
    # the window's name goes through scipy's get_window over the batches
    from scipy.signal import get_window
    got = run(ref, srv, L, F, R, hop, start, window=("kaiser", 5.0))
    assert O.rel_err(got, O.surface(ref, srv, L, F, R, hop, start, window=get_window(("kaiser", 5.0), F).astype(np.float32))) <= BAR
    # the floors are told apart by the test: 0.03 and 1.0 differ by far more than the bar
    assert O.rel_err(want(n, 0, L=L, F=F, R=R, hop=hop, start=start, filt=O.RECIPROCAL, floor=0.03),
                     want(n, 0, L=L, F=F, R=R, hop=hop, start=start, filt=O.RECIPROCAL, floor=1.0)) > 0.1


@pytest.mark.parametrize("L,hop,start", [(1024, 1152, 165), (4096, 4608, 549)])
def test_frames_at_an_odd_stride_and_pointers_one_element_in(gpu_ready, L, hop, start):
    import torch
    from passiveradar_amd import _lib, engine
    F, R, nf = 256, 33, 3
    n = length(L, F, hop, start)
    stride = n + 13
    rs = [inputs(n, seed) for seed in range(nf)]
    ref = torch.full((1 + nf * stride,), float("nan"), dtype=torch.complex64, device="cuda")
    srv = torch.full((1 + nf * stride,), float("nan"), dtype=torch.complex64, device="cuda")
    for b, (r, s) in enumerate(rs):
        ref[1 + b * stride:1 + b * stride + n] = dev(r)
        srv[1 + b * stride:1 + b * stride + n] = dev(s)
    win = torch.full((F + 1,), float("nan"), device="cuda")
    w = np.hanning(F + 2)[1:-1].astype(np.float32)
    win[1:] = dev(w)
    got = {}
    for name, filt in ((O.RECIPROCAL, _lib.BATCH_RECIPROCAL), (O.MATCHED, _lib.BATCH_MATCHED)):
        d = engine.batch_xambg_desc(n, L, R, F, hop, start, filt, 0.1)
        ws = torch.empty(engine.batch_xambg_workspace_bytes(d, nf) + 8, dtype=torch.uint8, device="cuda")
        out = torch.zeros(1 + nf * F * (R + 1), dtype=torch.complex64, device="cuda")
        engine.batch_xambg_execute(d, ref[1:], srv[1:], stride, win[1:], out[1:], nf, ws[8:], _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        got[name] = out[1:].cpu().numpy().reshape(nf, F, R + 1)
        for b in range(nf):
            err = O.rel_err(got[name][b], want(n, b, L=L, F=F, R=R, hop=hop, start=start, filt=name, window=w))
            assert err <= BAR, (L, name, b, err)
    # the stack front door: the same frames, dense, give the same bytes
    from passiveradar_amd.range_doppler_processing import batch_xambg
    for name in got:
        X = batch_xambg(np.stack([r for r, _ in rs]), np.stack([s for _, s in rs]), R, F, L, hop=hop, start=start, filter=name, window=w)
        assert X.shape == (nf, F, R + 1) and same_bits(X, got[name]), name


@pytest.mark.parametrize("L,hop,start", [(1024, 1152, 165), (4096, 4608, 549)])
def test_off_unit_amplitude(gpu_ready, L, hop, start):
    F, R = 256, 20
    n = length(L, F, hop, start)
    ref, srv = inputs(n)
    small, large = (ref * np.float32(2.0 ** -10)).astype(np.complex64), (srv * np.float32(2.0 ** 7)).astype(np.complex64)
    for filt, factor in ((O.RECIPROCAL, 2.0 ** 17), (O.MATCHED, 2.0 ** -3)):
        unit = want(n, 0, L=L, F=F, R=R, hop=hop, start=start, filt=filt)
        got = run(small, large, L, F, R, hop, start, filt)
        err = O.rel_err(got, factor * unit)
        print(f"L = {L} {filt}: ref 2^-10, srv 2^7: {err:.3g} of {factor} x the unit result")
        assert err <= BAR, (L, filt, err)


@pytest.mark.parametrize("L,hop,start", [(1024, 1152, 165), (4096, 4608, 549)])
def test_dead_air(gpu_ready, L, hop, start):
    F, R = 256, 20
    n = length(L, F, hop, start)
    ref, srv = inputs(n)
    dead = ref.copy()
    dead[start + 5 * hop:start + 5 * hop + L] = 0                                # batch 5 of the reference is silent
    for filt in (O.RECIPROCAL, O.MATCHED):
        w = O.surface(dead, srv, L, F, R, hop, start, filt)
        got = run(dead, srv, L, F, R, hop, start, filt)
        assert np.isfinite(got).all() and O.rel_err(got, w) <= BAR, (L, filt)
        # the silent batch's profile is zero: the surface is the one of the other 255 batches
        c = O.profiles(dead, srv, L, hop, start, F, R, filt)
        assert np.all(c[5] == 0)
        zero = run(np.zeros(n, np.complex64), srv, L, F, R, hop, start, filt)
        assert np.all(zero == 0), (L, filt)
        zero = run(np.zeros(n, np.complex64), np.zeros(n, np.complex64), L, F, R, hop, start, filt)
        assert np.all(zero == 0), (L, filt)


@pytest.mark.parametrize("L", [1024, 4096])
def test_exact_shift(gpu_ready, L):
    """srv is, batch by batch, the cyclic shift of a r_j by d: the reciprocal filter's profile of every batch is a at lag d and
    nothing elsewhere; read through F = 256 batches at Doppler 0 (row F / 2: the sum of the batch profiles)"""
    F, R, d, a, floor = 256, 30, 11, 0.6 - 0.3j, 0.01
    n = F * L
    ref = O.white(n, 77)
    srv = (a * np.roll(ref.reshape(F, L), d, axis=1)).reshape(-1).astype(np.complex64)
    for name, X in (("oracle", O.surface(ref, srv, L, F, R, floor=floor)), ("device", run(ref, srv, L, F, R, L, 0, floor=floor))):
        row = X[F // 2] / F                                                      # mean batch profile, column k = lag R - k
        print(f"L = {L} {name}: lag d {abs(row[R - d] - np.conj(a)):.3g} from conj(a), elsewhere {np.abs(np.delete(row, R - d)).max():.3g}")
        assert abs(row[R - d] - np.conj(a)) <= 1e-3 * abs(a), (name, row[R - d])
        assert np.abs(np.delete(row, R - d)).max() < 1e-3 * abs(a), name
        assert np.abs(np.delete(X, F // 2, axis=0)).max() < 1e-3 * abs(a) * F, name


def test_design_scene_end_to_end_and_detection(gpu_ready):
    from passiveradar_amd.range_doppler_processing import batch_xambg, ofdm_symbol_start
    from passiveradar_amd.target_detection import CFAR_2D, extract_plots
    D = O.DESIGN
    ref, srv = O.design_scene()
    at = ofdm_symbol_start(ref, D["L"], D["cp"])
    assert at == D["symbol_start"]
    kw = dict(hop=D["L"] + D["cp"], start=at + D["cp"])
    Xr = batch_xambg(ref, srv, D["R"], D["F"], D["L"], **kw)
    Xm = batch_xambg(ref, srv, D["R"], D["F"], D["L"], filter="matched", **kw)
    for X, filt in ((Xr, O.RECIPROCAL), (Xm, O.MATCHED)):
        err = O.rel_err(X[:, :, 0], O.surface(ref, srv, **O.design_args(filt)))
        print(f"design scene, {filt}: {err:.3g}")
        assert err <= BAR
    c = O.design_conditions(Xr[:, :, 0], Xm[:, :, 0])
    print(c)
    O.check_design(c)
    # the map goes through the detector and the plot extractor as fast_xambg's does: both echoes come out as plots
    W = D["R"] + 1
    stat = CFAR_2D(np.abs(Xr[:, :, 0]), 8, 2)
    meas, info, _ = extract_plots(stat, 8.0, [D["F"] / 2.0, float(D["R"])], range_guard=0, doppler_guard=0, return_info=True)
    peaks = {(int(p) // W, int(p) % W) for p in info["peak"]}
    print(f"{meas.shape[1]} plots, peaks {sorted(peaks)[:8]}")
    assert c["strong"] in peaks and c["weak"] in peaks, peaks


def test_numpy_and_device_tensors_give_the_same_bytes(gpu_ready):
    import torch
    from passiveradar_amd.range_doppler_processing import batch_xambg, ofdm_symbol_start
    for L, F, R, hop, start in (SHAPES[0], SHAPES[3]):
        n = length(L, F, hop, start)
        ref, srv = inputs(n)
        w = np.hamming(F).astype(np.float32)
        for filt in (O.RECIPROCAL, O.MATCHED):
            a = batch_xambg(ref, srv, R, F, L, hop=hop, start=start, filter=filt, window=w)
            b = batch_xambg(dev(ref), dev(srv), R, F, L, hop=hop, start=start, filter=filt, window=w)
            c = batch_xambg(dev(ref), dev(srv), R, F, L, hop=hop, start=start, filter=filt, window=dev(w))
            assert b.is_cuda and b.dtype == torch.complex64 and tuple(b.shape) == (F, R + 1, 1)
            assert same_bits(a, b) and same_bits(a, c), (L, filt)
    ref = O.design_scene()[0]
    s0, m0 = ofdm_symbol_start(ref, 1024, 128, return_metric=True)
    s1, m1 = ofdm_symbol_start(dev(ref), 1024, 128, return_metric=True)
    assert s0 == s1 == 37 and m1.is_cuda and m1.dtype == torch.float64 and same_bits(m0.view(np.uint32), m1.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("L,F,R,hop,start", [SHAPES[0], SHAPES[3]])
def test_capture_and_replay(gpu_ready, L, F, R, hop, start):
    """one call -- the batch kernel and the Doppler kernel on one stream -- captured in a linear graph replays to the same
    bytes, and to the new input's result"""
    import torch
    from passiveradar_amd import _lib, engine
    n = length(L, F, hop, start)
    ref, srv = inputs(n)
    d = engine.batch_xambg_desc(n, L, R, F, hop, start, _lib.BATCH_RECIPROCAL, 0.1)
    x, y = dev(ref), dev(srv)
    ws = torch.empty(engine.batch_xambg_workspace_bytes(d, 1), dtype=torch.uint8, device="cuda")
    out = torch.zeros((F, R + 1), dtype=torch.complex64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm up: the twiddle tables are made once, outside the capture
        engine.batch_xambg_execute(d, x, y, n, None, out, 1, ws, _lib.torch_stream_ptr())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine.batch_xambg_execute(d, x, y, n, None, out, 1, ws, _lib.torch_stream_ptr())
    for _ in range(2):
        out.fill_(-1.0)
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.float32), eager.view(torch.float32))
    ref2, srv2 = inputs(n, 1)
    x.copy_(dev(ref2))
    y.copy_(dev(srv2))
    g.replay()
    torch.cuda.synchronize()
    assert O.rel_err(out.cpu().numpy(), want(n, 1, L=L, F=F, R=R, hop=hop, start=start, filt=O.RECIPROCAL)) <= BAR


TIMING = [(1024, 128, 5, 300), (4096, 512, 2, 1111), (100, 7, 3, 55)]


@pytest.mark.parametrize("nfft,cp,nsym,at", TIMING, ids=lambda v: str(v))
def test_timing(gpu_ready, nfft, cp, nsym, at):
    """OFDM-like symbols (white noise bodies behind their cyclic prefixes) starting at ``at``; the shortest legal length, and one
    sample less, which is refused"""
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd.range_doppler_processing import ofdm_symbol_start
    sym = nfft + cp
    n = (nsym + 1) * sym + nfft
    body = O.white((nsym + 4) * nfft, nfft).reshape(nsym + 4, nfft)
    x = np.roll(np.concatenate([body[:, nfft - cp:], body], axis=1).reshape(-1), at)[:n]
    x = (x + 0.05 * O.white(n, 3)).astype(np.complex64)
    wm = O.timing_metric(x, nfft, cp, nsym)
    start, metric = ofdm_symbol_start(x, nfft, cp, nsym, return_metric=True)
    err = float(np.abs(metric - wm).max() / wm.max())
    print(f"timing ({nfft}, {cp}, {nsym}): metric {err:.3g} of its peak, start {start}")
    assert metric.shape == (sym,) and metric.dtype == np.float64 and err <= O.TIMING_BAR
    assert start == int(np.argmax(wm)) == at % sym
    assert ofdm_symbol_start(x, nfft, cp) == start                               # nsym None: the most the length allows, here nsym
    with pytest.raises(ValueError, match="samples are needed"):
        ofdm_symbol_start(x[:-1], nfft, cp, nsym)
    m = torch.zeros(sym, dtype=torch.float64, device="cuda")
    w = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="samples are needed"):
        engine.ofdm_timing(dev(x), n - 1, nfft, cp, nsym, m, w, _lib.torch_stream_ptr())
