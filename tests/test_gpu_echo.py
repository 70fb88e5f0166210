"""prc_echo_cancel / cancel_echoes / clean_xambg on the GPU (passiveradar_amd/csrc/echo.hip) against the float64 restatement of
the definition (tests/echo_oracle.py) on the same complex64 inputs.

Bars (include/prcore.h): max|out - oracle| <= 2e-6 max|srv| (the project's parity bar); amplitudes and
slopes within 2e-6 max|c|; refined Dopplers within 1e-6 Fs / n (a Doppler difference of d cells leaves (pi / sqrt 3) d of the
echo, so this is what the out bar needs).  They are stated for scenes whose oracle cond(G) < 100, which every case asserts.
Every case prints its measured figures before it asserts."""
import functools

import numpy as np
import pytest

import echo_oracle as EO

pytestmark = pytest.mark.gpu

OUT_BAR, COEF_BAR, DOPPLER_BAR = 2e-6, 2e-6, 1e-6


def _white(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def _frame(seed, n, fs, echoes, wrap, noise=1e-3):
    """white complex64 reference; srv = the echoes (lag, Doppler Hz, amplitude) + noise"""
    rng = np.random.default_rng(seed)
    ref = _white(rng, n)
    srv = noise * _white(rng, n).astype(np.complex128)
    for lag, f, amp in echoes:
        srv = srv + EO.echo(ref, lag, f, fs, amp, wrap)
    return ref, srv.astype(np.complex64)


def run(ref, srv, fs, lags, dops, *, wrap=False, ramp=True, refine=2, reg=0.0, max_atoms=None, stride=None, out_stride=None,
        counts=None, junk=None, fill=None):
    """prc_echo_cancel on a stack ref / srv [nframes, n] with per-frame lists.  Returns out [nframes, n], fit
    [nframes, max_atoms], info [nframes] and the atom list's bytes before and after."""
    import torch
    from passiveradar_amd import _lib, engine
    nf, n = ref.shape
    M = max([len(l) for l in lags] + [1]) if max_atoms is None else max_atoms
    stride = n if stride is None else stride
    out_stride = n if out_stride is None else out_stride
    rec = np.zeros((nf, M), _lib.ECHO_ATOM_DTYPE)
    if junk is not None:                                   # what the slots beyond a frame's count hold
        rec["lag"], rec["doppler"] = junk
    cnt = np.zeros(nf, np.int32)
    for b in range(nf):
        k = len(lags[b])
        rec["lag"][b, :k], rec["doppler"][b, :k], cnt[b] = lags[b], dops[b], k
    if counts is not None:
        cnt = np.asarray(counts, np.int32)
    d = engine.echo_desc(n, fs, M, nf, wrap, ramp, refine, reg, stride, out_stride)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = torch.zeros(nf * stride, dtype=torch.complex64, device="cuda")
    s = torch.zeros(nf * stride, dtype=torch.complex64, device="cuda")
    r.as_strided((nf, n), (stride, 1)).copy_(dev(ref))
    s.as_strided((nf, n), (stride, 1)).copy_(dev(srv))
    o = torch.full((nf * out_stride,), complex(7.0, -7.0), dtype=torch.complex64, device="cuda")
    atoms = dev(rec.view(np.uint8).reshape(-1))
    fit = torch.full((nf * M * _lib.ECHO_FIT_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    info = torch.full((nf,), -9, dtype=torch.int32, device="cuda")
    ws = torch.zeros(engine.echo_workspace_bytes(d), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    engine.echo_execute(d, r, s, atoms, dev(cnt), o, fit, info, ws, _lib.torch_stream_ptr())
    torch.cuda.synchronize()
    out = o.as_strided((nf, n), (out_stride, 1)).cpu().numpy()
    if out_stride > n:                                     # nothing between the frames was written
        gaps = o[:(nf - 1) * out_stride].view(nf - 1, out_stride)[:, n:]
        assert bool((gaps == complex(7.0, -7.0)).all())
    return (out, fit.cpu().numpy().view(_lib.ECHO_FIT_DTYPE).reshape(nf, M), info.cpu().numpy(),
            rec.view(np.uint8).reshape(-1).copy(), atoms.cpu().numpy())


def hold(tag, out, fit, info, ref, srv, fs, lags, dops, need_cond=True, **kw):
    """one frame of a device result against the oracle, at the bars of the module docstring"""
    n = ref.shape[0]
    want, wfit, winfo, cond = EO.cancel(ref, srv, fs, lags, dops, return_cond=True, **kw)
    k = len(lags)
    e_out = np.abs(out.astype(np.complex128) - want).max() / np.abs(srv).max()
    cmax = max(np.abs(wfit["amp"]).max(initial=0), np.abs(wfit["slope"]).max(initial=0), 1e-300)
    e_c = max(np.abs(fit["amp"][:k] - wfit["amp"]).max(initial=0), np.abs(fit["slope"][:k] - wfit["slope"]).max(initial=0)) / cmax
    e_f = np.abs(fit["doppler"][:k] - wfit["doppler"]).max(initial=0) * n / abs(fs)
    print(f"{tag}: out {e_out:.3g} (bar {OUT_BAR:g}), coefficients {e_c:.3g} (bar {COEF_BAR:g}), Dopplers {e_f:.3g} cells "
          f"(bar {DOPPLER_BAR:g}), cond(G) {cond:.3g}, info {info}")
    assert info == winfo
    assert not need_cond or cond < 100, cond
    assert np.array_equal(fit["flags"][:k], wfit["flags"]), (fit["flags"][:k], wfit["flags"])
    assert e_out <= OUT_BAR and e_c <= COEF_BAR and e_f <= DOPPLER_BAR
    assert not fit[k:].view(np.uint8).any()                # records from the count on are zero
    return e_out, e_c, e_f


def _design():
    ref, srv, fs = EO.design_scene()
    return dict(ref=ref, srv=srv, fs=fs, lags=[7, 12], dops=[3.0, -3.0], wrap=True)


def _case(seed, n, echoes, offs, wrap=False, fs=None, **kw):
    fs = float(n) if fs is None else fs
    ref, srv = _frame(seed, n, fs, echoes, wrap)
    return dict(ref=ref, srv=srv, fs=fs, lags=[e[0] for e in echoes], dops=[e[1] + o for e, o in zip(echoes, offs)], wrap=wrap, **kw)


def _many(n, k):
    """k echoes at lags 3 j + 1, Dopplers spread over +-40 cells, amplitudes 1 .. 0.1"""
    return [(3 * j + 1, ((17 * j) % 81 - 40) + 0.37, 1.0 / (1 + 0.3 * j)) for j in range(k)]


CASES = {
    # n = 6001: no tile divides it; the design scene from whole cells
    "design_6001": _design,
    # n = 4096: whole tiles; lag 0
    "tiles_4096_lag0": lambda: _case(11, 4096, [(0, 2.2, 1.0), (5, -7.4, 0.6)], [0.2, -0.3]),
    # n = 61: below one tile
    "short_61": lambda: _case(12, 61, [(0, 1.3, 1.0), (3, -2.1, 0.7)], [0.1, 0.2]),
    # |f| near Fs / 2 at n = 65553: a float32 ramp over i is off by whole radians there
    "nyquist_65553": lambda: _case(13, 65553, [(3, 32770.3, 1.0), (40, -32771.6, 0.5)], [0.2, -0.25]),
    "lag_n_minus_1_wrap": lambda: _case(14, 4096, [(4095, 3.3, 1.0), (2, -1.2, 0.8)], [0.3, 0.1], wrap=True),
    "negative_lag_wrap": lambda: _case(15, 4096, [(-5, 0.7, 1.0), (6, 9.1, 0.4)], [-0.2, 0.3], wrap=True),
    "lag_n_minus_1_plain": lambda: _case(16, 4096, [(4095, 1.0, 1.0)], [0.0], ramp=False, refine=0),
    "one_atom": lambda: _case(17, 3000, [(9, -4.6, 1.0)], [0.3]),
    # 32 atoms with ramp: 64 columns, the limit (the 9-pairs-per-thread Gram form)
    "atoms_32": lambda: _case(18, 4096, _many(4096, 32), [0.2 * (-1) ** j for j in range(32)]),
    # 12 atoms with ramp: 25 columns, the 3-pairs-per-thread Gram form
    "atoms_12": lambda: _case(19, 2500, _many(2500, 12), [0.15] * 12),
    "plain_ramp0": lambda: _case(20, 3000, [(4, 2.0, 1.0), (11, -3.0, 0.5)], [0.0, 0.0], ramp=False, refine=0),
    "plain_ramp0_wrap": lambda: _case(21, 3000, [(4, 2.0, 1.0), (11, -3.0, 0.5)], [0.004, 0.0], ramp=False, refine=0, wrap=True),
    "refine0": lambda: _case(22, 3000, [(4, 2.2, 1.0), (11, -3.4, 0.5)], [0.2, -0.1], refine=0),
    "refine4": lambda: _case(23, 3000, [(4, 2.2, 1.0), (11, -3.4, 0.5)], [0.4, -0.4], refine=4),
    "reg": lambda: _case(24, 3000, [(4, 2.2, 1.0), (11, -3.4, 0.5)], [0.2, -0.1], reg=150.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(gpu_ready, name):
    c = dict(CASES[name]())
    ref, srv, fs, lags, dops = (c.pop(k) for k in ("ref", "srv", "fs", "lags", "dops"))
    out, fit, info, before, after = run(ref[None], srv[None], fs, [lags], [dops], **c)
    hold(name, out[0], fit[0], info[0], ref, srv, fs, lags, dops, **c)
    assert np.array_equal(before, after)


def test_design_scene_is_cleaned(gpu_ready):
    """the device result on the design scene does what the feature is for: residual <= -45 dB from the whole cells"""
    c = _design()
    out, fit, info, _, _ = run(c["ref"][None], c["srv"][None], c["fs"], [c["lags"]], [c["dops"]], wrap=True)
    p = lambda x: np.sum(np.abs(x.astype(np.complex128)) ** 2)
    db = 10 * np.log10(p(out[0]) / p(c["srv"]))
    print(f"residual {db:.2f} dB, Dopplers {fit[0]['doppler']}")
    assert info[0] == 0 and db <= -45.0 and np.abs(fit[0]["doppler"] - [3.3, -2.7]).max() < 1e-3


@functools.lru_cache(maxsize=1)
def _stack():
    n, fs = 1500, 1500.0
    e0 = [(3, 1.7, 1.0), (20, -6.2, 0.5)]
    e2 = [(1, 0.4, 1.0), (8, 5.5, 0.8), (15, -9.3, 0.6), (22, 12.8, 0.4), (40, -2.6, 0.3)]
    frames = [_frame(31, n, fs, e0, False), _frame(32, n, fs, [(5, 1.0, 1.0)], False), _frame(33, n, fs, e2, False)]
    ref = np.stack([f[0] for f in frames])
    srv = np.stack([f[1] for f in frames])
    lags = [[e[0] for e in e0], [], [e[0] for e in e2]]
    dops = [[e[1] + 0.2 for e in e0], [], [e[1] - 0.15 for e in e2]]
    return n, fs, ref, srv, lags, dops


def test_stack_with_an_empty_frame_and_strides(gpu_ready):
    """three frames with counts (2, 0, 5) and strides above n: every frame matches its own oracle run, the frame without atoms
    comes back bit for bit, the slots beyond a frame's count are never read (they hold lags beyond n and NaN Dopplers) and the
    caller's list is unchanged"""
    n, fs, ref, srv, lags, dops = _stack()
    junk = (np.full((3, 5), 2 ** 31 - 1, np.int32), np.full((3, 5), np.nan))
    out, fit, info, before, after = run(ref, srv, fs, lags, dops, stride=n + 37, out_stride=n + 11, junk=junk)
    for b in range(3):
        hold(f"frame {b}", out[b], fit[b], info[b], ref[b], srv[b], fs, lags[b], dops[b])
    assert np.array_equal(out[1].view(np.uint32), srv[1].view(np.uint32))
    assert np.array_equal(before, after)
    # 200 frames: fewer chunks per frame, the same numbers
    big = run(np.tile(ref, (67, 1))[:200], np.tile(srv, (67, 1))[:200], fs, (lags * 67)[:200], (dops * 67)[:200])
    for b in (0, 1, 2, 198, 199):
        hold(f"frame {b} of 200", big[0][b], big[1][b], big[2][b], ref[b % 3], srv[b % 3], fs, lags[b % 3], dops[b % 3])


def test_counts_are_clipped(gpu_ready):
    """a count above max_atoms reads max_atoms records, a negative one none"""
    n, fs, ref, srv, lags, dops = _stack()
    out, fit, info, _, _ = run(ref[[2, 0]], srv[[2, 0]], fs, [lags[2], lags[0]], [dops[2], dops[0]], counts=[12, -3])
    hold("count 12 of 5", out[0], fit[0], info[0], ref[2], srv[2], fs, lags[2], dops[2])
    assert info[1] == 0 and np.array_equal(out[1].view(np.uint32), srv[0].view(np.uint32)) and not fit[1].view(np.uint8).any()


def test_bad_atoms_are_skipped_and_flagged(gpu_ready):
    """atoms with |lag| >= n or a Doppler that is not finite, mixed among good ones: flagged (bit 0), and the good ones come out
    as the oracle run without the bad ones has them"""
    n, fs, ref, srv, lags, dops = _stack()
    L = [n, lags[0][0], -n, 2 ** 31 - 1, lags[0][1], 7, -2 ** 31]
    D = [0.0, dops[0][0], 1.0, 2.0, dops[0][1], np.nan, np.inf]
    out, fit, info, _, _ = run(ref[:1], srv[:1], fs, [L], [D])
    hold("bad among good", out[0], fit[0], info[0], ref[0], srv[0], fs, L, D)
    # the list without the bad ones, at the same capacity (the order of the Gram sums goes with max_atoms): the same bytes
    good, gfit, _, _, _ = run(ref[:1], srv[:1], fs, [lags[0]], [dops[0]], max_atoms=len(L))
    assert np.array_equal(out.view(np.uint32), good.view(np.uint32))
    assert fit[0]["flags"].tolist() == [1, 0, 1, 1, 0, 1, 1] and np.array_equal(fit[0][[1, 4]], gfit[0][:2])
    # only bad ones: nothing to fit
    out, fit, info, _, _ = run(ref[:1], srv[:1], fs, [[n, 3]], [[1.0, np.nan]])
    assert info[0] == 0 and np.array_equal(out.view(np.uint32), srv[:1].view(np.uint32)) and fit[0]["flags"].tolist() == [1, 1]


@pytest.mark.parametrize("how", ["duplicate", "silent_reference"])
def test_breakdown(gpu_ready, how):
    """duplicate atoms, or a zero reference, with reg = 0: info = 1, out = srv bit for bit, zero fits with bit 2, no NaN anywhere;
    the other frame of the stack is not disturbed; reg > 0 repairs it"""
    n, fs, ref, srv, lags, dops = _stack()
    r = ref[[0, 0]].copy()
    if how == "silent_reference":
        r[0] = 0
    L = [[3, 3], lags[0]] if how == "duplicate" else [lags[0], lags[0]]
    D = [[1.9, 1.9], dops[0]] if how == "duplicate" else [dops[0], dops[0]]
    out, fit, info, _, _ = run(r, srv[[0, 0]], fs, L, D)
    assert info.tolist() == [1, 0]
    assert np.array_equal(out[0].view(np.uint32), srv[0].view(np.uint32))
    assert fit[0]["flags"].tolist() == [4, 4] and not fit[0]["amp"].any() and not fit[0]["slope"].any() and not fit[0]["doppler"].any()
    assert np.isfinite(out.view(np.float32)).all()
    assert all(np.isfinite(fit[k]).all() for k in ("doppler", "amp", "slope"))
    hold("the frame beside it", out[1], fit[1], info[1], ref[0], srv[0], fs, lags[0], dops[0])
    # (the split between two duplicates is as ill-determined as ever -- only their sum, and so out, is held to the oracle)
    out, fit, info, _, _ = run(r, srv[[0, 0]], fs, L, D, reg=1.0, refine=0)
    want = EO.cancel(r[0], srv[0], fs, L[0], D[0], reg=1.0, refine=0)[0]
    e = np.abs(out[0].astype(np.complex128) - want).max() / np.abs(srv[0]).max()
    print(f"with reg = 1: out {e:.3g}")
    assert info.tolist() == [0, 0] and np.isfinite(out.view(np.float32)).all() and e <= OUT_BAR


def test_dead_air(gpu_ready):
    """srv = 0: out = 0, c = 0, and the refinement is skipped (the Dopplers stay)"""
    n, fs, ref, srv, lags, dops = _stack()
    out, fit, info, _, _ = run(ref[:1], np.zeros_like(srv[:1]), fs, [lags[0]], [dops[0]])
    assert info[0] == 0 and not out.view(np.uint32).any()
    assert not fit[0]["amp"].any() and not fit[0]["slope"].any() and fit[0]["doppler"].tolist() == dops[0] and not fit[0]["flags"].any()


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scale(gpu_ready, scale):
    """inputs x 1e-3 and x 1e3 with reg = 0: the outputs scale within the bar, and each holds its own oracle's bars"""
    n, fs, ref, srv, lags, dops = _stack()
    one = run(ref[2:], srv[2:], fs, [lags[2]], [dops[2]])
    rs, ss = (ref[2:] * np.float32(scale)).astype(np.complex64), (srv[2:] * np.float32(scale)).astype(np.complex64)
    out, fit, info, _, _ = run(rs, ss, fs, [lags[2]], [dops[2]])
    hold(f"x {scale:g}", out[0], fit[0], info[0], rs[0], ss[0], fs, lags[2], dops[2])
    e = np.abs(out[0].astype(np.complex128) / scale - one[0][0]).max() / np.abs(srv[2]).max()
    print(f"scaled back: {e:.3g}")
    assert e <= OUT_BAR


def test_properties(gpu_ready):
    """the residual is no longer than srv; the same bytes whatever the workspace held"""
    n, fs, ref, srv, lags, dops = _stack()
    a = run(ref, srv, fs, lags, dops)
    nrm = lambda x: np.sqrt(np.sum(np.abs(x.astype(np.complex128)) ** 2, axis=-1))
    assert np.all(nrm(a[0]) <= nrm(srv) * (1 + 1e-6))
    b = run(ref, srv, fs, lags, dops, fill=0xFF)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8)) and np.array_equal(a[2], b[2])
    big = _case(18, 4096, _many(4096, 32), [0.2 * (-1) ** j for j in range(32)])
    a = run(big["ref"][None], big["srv"][None], big["fs"], [big["lags"]], [big["dops"]])
    b = run(big["ref"][None], big["srv"][None], big["fs"], [big["lags"]], [big["dops"]], fill=0xFF)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))
    assert nrm(a[0])[0] <= nrm(big["srv"]) * (1 + 1e-6)


def test_graph_capture_and_replay(gpu_ready):
    """the call enqueues a fixed set of launches and reads nothing back: captured on a side stream and replayed twice == eager"""
    import torch
    from passiveradar_amd import _lib, engine
    n, fs, ref, srv, lags, dops = _stack()
    eager = run(ref, srv, fs, lags, dops)
    M = 5
    rec = np.zeros((3, M), _lib.ECHO_ATOM_DTYPE)
    cnt = np.zeros(3, np.int32)
    for b in range(3):
        k = len(lags[b])
        rec["lag"][b, :k], rec["doppler"][b, :k], cnt[b] = lags[b], dops[b], k
    d = engine.echo_desc(n, fs, M, 3)
    r, s = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()
    atoms, counts = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(cnt).cuda()
    out = torch.zeros((3, n), dtype=torch.complex64, device="cuda")
    fit = torch.zeros(3 * M * 48, dtype=torch.uint8, device="cuda")
    info = torch.zeros(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(engine.echo_workspace_bytes(d), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.echo_execute(d, r, s, atoms, counts, out, fit, info, ws, _lib.torch_stream_ptr())
    side.synchronize()
    for k in range(2):
        out.zero_()
        fit.zero_()
        info.fill_(-1)
        ws.fill_(0xFF if k else 0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), eager[0].view(np.uint32))
        assert np.array_equal(fit.cpu().numpy(), eager[1].view(np.uint8).reshape(-1)) and np.array_equal(info.cpu().numpy(), eager[2])


def test_wrapper_numpy_and_tensors(gpu_ready):
    """cancel_echoes from NumPy and from device tensors gives the same bytes, 1-D and stacked; the fit comes back in the caller's
    order; a breakdown raises PrcoreError with ECA_Filter's advice"""
    import torch
    from passiveradar_amd import _lib
    from passiveradar_amd.clutter_removal import cancel_echoes
    n, fs, ref, srv, lags, dops = _stack()
    out, f, amp, slope, flags = cancel_echoes(ref[0], srv[0], fs, lags[0], dops[0], return_fit=True)
    raw = run(ref[:1], srv[:1], fs, [lags[0]], [dops[0]])
    assert out.dtype == np.complex64 and out.shape == (n,) and np.array_equal(out.view(np.uint32), raw[0][0].view(np.uint32))
    assert np.array_equal(f, raw[1][0]["doppler"]) and np.array_equal(amp, raw[1][0]["amp"]) and amp.dtype == np.complex128
    assert np.array_equal(slope, raw[1][0]["slope"]) and not flags.any()
    t = cancel_echoes(torch.from_numpy(ref[0]).cuda(), torch.from_numpy(srv[0]).cuda(), fs, lags[0], dops[0])
    assert t.is_cuda and t.dtype == torch.complex64 and np.array_equal(t.cpu().numpy().view(np.uint32), out.view(np.uint32))
    stack, fs_, amps, _, _ = cancel_echoes(ref, srv, fs, lags, dops, return_fit=True)
    tstack = cancel_echoes(torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda(), fs, lags, dops)
    want = run(ref, srv, fs, lags, dops)
    assert stack.shape == (3, n) and np.array_equal(stack.view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(tstack.cpu().numpy().view(np.uint32), stack.view(np.uint32))
    assert [len(a) for a in amps] == [2, 0, 5] and np.array_equal(fs_[2], want[1][2]["doppler"])
    with pytest.raises(_lib.PrcoreError, match="reg > 0"):
        cancel_echoes(ref[0], srv[0], fs, [3, 3], [1.0, 1.0])
    assert np.isfinite(cancel_echoes(ref[0], srv[0], fs, [3, 3], [1.0, 1.0], reg=1.0).view(np.float32)).all()


@pytest.mark.parametrize("tensors", [False, True])
def test_clean_xambg_uncovers_the_weak_echo(gpu_ready, tensors):
    """the feature: on the design scene the raw fast_xambg surface peaks on the unit echo; clean_xambg with npeaks = 2 and the
    guard off zero Doppler returns a surface whose argmax is the weak echo's cell, and the removed-echo records are
    (7, 3.3 Hz) and (12, -2.7 Hz) within 0.005 Hz"""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.range_doppler_processing import clean_xambg, fast_xambg
    ref, srv, fs = EO.design_scene()
    n, R, F = ref.shape[0], 31, 353                       # 6001 = 17 x 353: one Doppler row is 1 Hz
    cell = lambda lag, f: scene.expected_peak_cell(lag, f, n, fs, R, F)
    raw = np.abs(fast_xambg(ref, srv, R, F)[:, :, 0])
    assert np.unravel_index(raw.argmax(), raw.shape) == cell(7, 3.3)
    weak = raw[cell(9, -5.6)] / np.median(raw)
    a, b = (torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()) if tensors else (ref, srv)
    X, rec = clean_xambg(a, b, fs, R, F, npeaks=2, doppler_guard=-1, wrap=True)
    X = X.cpu().numpy() if tensors else X
    assert X.shape == (F, R + 1, 1) and X.dtype == np.complex64
    S = np.abs(X[:, :, 0])
    print(f"raw: weak cell / median {weak:.2f}; cleaned: peak / median {S.max() / np.median(S):.1f}; records {rec}")
    assert np.unravel_index(S.argmax(), S.shape) == cell(9, -5.6)
    assert rec["lag"].tolist() == [7, 12]
    assert np.abs(rec["doppler"] - [3.3, -2.7]).max() < 0.005
    assert np.abs(np.abs(rec["amplitude"]) - [1.0, 0.5]).max() < 0.01
    # lag_span = 1: three atoms per echo, the same surface peak
    X3, rec3 = clean_xambg(a, b, fs, R, F, npeaks=2, doppler_guard=-1, lag_span=1, wrap=True)
    S3 = np.abs((X3.cpu().numpy() if tensors else X3)[:, :, 0])
    assert rec3["lag"].tolist() == [6, 7, 8, 11, 12, 13] and np.unravel_index(S3.argmax(), S3.shape) == cell(9, -5.6)
