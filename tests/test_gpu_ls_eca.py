"""ECA_Filter on the GPU (passiveradar_amd/csrc/eca.hip) against its float64 restatement (tests/eca_oracle.py): the scene the
canceller exists for, the shapes at which the kernels can go wrong, batches and determinism, guard bands, breakdown, graph capture
and the HipBackend mode.  Errors are peak-normalised (conftest.rel_err).  Bars: out 1e-4 (the project's parity bar); suppression
within 0.5 dB of the restatement's and at least 15 dB beyond the chain's; complex128 taps TAPS128_BAR and solve_bar (below).

The file sorts after test_gpu_lifetime.py on purpose: that test holds the device's free memory to 1 MiB
in the suite's one process, and the plans and staging buffers the drop-ins here leave cached moved it by one 2 MiB granule."""
import functools

import numpy as np
import pytest

import eca_oracle as E
from conftest import rel_err

pytestmark = pytest.mark.gpu

# device complex128 taps against the restatement's dense solve on the scenes with cond(G) <= 1e5, measured on MI355X: white
# scene (cond 5.1e2) 1.23e-9, AR(1) scene (cond 8.0e4) 2.14e-9, amplitude 1e3 1.30e-9, amplitude 1e-3 1.15e-9.  Ten times the
# largest is 2.1e-8; anything looser than 1e-8 is not allowed, so the bar is 1e-8.  What is measured
# here is not the float64 solve: with one bin of 0 Hz (no ramp) the distance is 2e-16.  It is the last bit of the float32 sine
# and cosine of the ramp, where the device's sincosf and NumPy differ, carried into the taps by cond(G): on the eight bins of
# B8_T16 below (cond 9.7e4 from the bins themselves, half a resolution cell apart) it reaches 4.2e-7.
TAPS128_BAR = 1e-8


def solve_bar(cond):
    """The solve alone: both sides on the SAME regressors (the restatement takes the device's frequency_shift, which runs the
    arithmetic the kernels rotate with).  What is left is the rounding of the float64 sums behind G and y (n terms in chunks:
    some tens of ulps of R_0 at most) and of the two solves, carried into the taps by cond(G): 64 ulps times cond(G)."""
    return 64.0 * 2.0 ** -52 * cond


def _device_shift(x, fc, fs):
    from passiveradar_amd.signal_utils import frequency_shift
    return frequency_shift(x, fc, fs)

T_SCENE = E.SCENE_L + E.SCENE_PEEK


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    yield


def _call(refs, srvs, n, L, peek, fs, bins, reg=0.0, stride=None, ostride=None):
    """blocks [nb, stride] through one engine.eca_execute: out [nb, n] c64, taps [nb, B, T] c128, info [nb]"""
    import torch
    from passiveradar_amd import engine
    nb, B, T = refs.shape[0], len(bins), L + peek
    stride = refs.shape[1] if stride is None else stride
    ostride = n if ostride is None else ostride
    r, s = torch.from_numpy(np.ascontiguousarray(refs)).cuda(), torch.from_numpy(np.ascontiguousarray(srvs)).cuda()
    sentinel = complex(7.0, -3.0)
    out = torch.full((nb, ostride), sentinel, dtype=torch.complex64, device="cuda")
    taps = torch.full((nb, B, T), sentinel, dtype=torch.complex128, device="cuda")
    info = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(engine.eca_workspace_bytes(n, L, peek, B, nb), dtype=torch.uint8, device="cuda")
    engine.eca_execute(r, s, out, n, L, peek, fs, bins, reg, nb, stride, ostride, taps, info, ws)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == sentinel)
    return out[:, :n], taps.cpu().numpy(), info.cpu().numpy()


def _run(ref, srv, L, peek, fs, bins, reg=0.0):
    out, taps, info = _call(ref[None, :], srv[None, :], ref.shape[0], L, peek, fs, bins, reg)
    return out[0], taps[0], int(info[0])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _cwhite(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def _surveillance(rng, ref, fs, bins, amp=1.0):
    """echoes of ref at small delays, each a tenth of a resolution cell off its bin (on it at 0 Hz), a weak far target, noise"""
    n = ref.shape[0]
    t = np.arange(n, dtype=np.float64)
    cell = fs / n
    srv = 0.01 * np.roll(ref, 9) * np.exp(2j * np.pi * 40.0 * cell * t / fs) + 0.001 * _cwhite(rng, n)
    for d, (f, a) in enumerate(zip(bins, (1.0, 0.3, 0.2, 0.1, 0.1, 0.05, 0.05, 0.02))):
        srv = srv + a * np.roll(ref, d % 4) * np.exp(2j * np.pi * (f + 0.1 * cell * (f != 0)) * t / fs)
    return (amp * srv).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _scene(pole, amplitude=1.0):
    """the scene, the restatement on it and the device's result, once per session"""
    ref, srv, floor = E.scene(1, pole, amplitude=amplitude)
    eo, et, (G, _, _) = E.ECA_Filter(ref, srv, E.SCENE_L, E.SCENE_FS, E.SCENE_BINS, E.SCENE_PEEK, 0.0, True, True)
    out, taps, info = _run(ref, srv, E.SCENE_L, E.SCENE_PEEK, E.SCENE_FS, E.SCENE_BINS)
    return ref, srv, floor, eo, et, float(np.linalg.cond(G)), out, taps, info


@pytest.mark.parametrize("pole", [0.0, 0.9])
def test_scene_out_and_taps(pole):
    """white reference (cond 5e2) and AR(1) reference with pole 0.9 (cond 8e4)"""
    ref, srv, _, eo, et, cond, out, taps, info = _scene(pole)
    e_out, e_taps = rel_err(out, eo), rel_err(taps, et)
    _, ets = E.ECA_Filter(ref, srv, E.SCENE_L, E.SCENE_FS, E.SCENE_BINS, E.SCENE_PEEK, 0.0, True, shift=_device_shift)
    e_solve = rel_err(taps, ets)
    print(f"pole {pole}: cond {cond:.3g}, out {e_out:.2e}, taps {e_taps:.2e}, on the device's regressors {e_solve:.2e}")
    assert info == 0 and cond <= 1e5
    assert e_out <= 1e-4
    assert e_taps <= TAPS128_BAR
    assert e_solve <= solve_bar(cond)


@pytest.mark.parametrize("pole", [0.0, 0.9])
def test_scene_suppression(pole):
    """what is left of the clutter above the floor over [2T, n - 2T): within 0.5 dB of the restatement's, and at least 15 dB
    below what LS_Filter_Multiple's chain leaves on the device"""
    from passiveradar_amd.clutter_removal import LS_Filter_Multiple
    ref, srv, floor, eo, _, _, out, _, _ = _scene(pole)
    chain = LS_Filter_Multiple(ref, srv, E.SCENE_L, E.SCENE_FS, list(E.SCENE_BINS))
    dev, ora, ch = (E.clutter_db(x, floor, T_SCENE) for x in (out, eo, chain))
    print(f"pole {pole}: device {dev:.2f} dB, restatement {ora:.2f} dB, chain {ch:.2f} dB, gain {ch - dev:.2f} dB")
    assert abs(dev - ora) <= 0.5
    assert ch - dev >= 15.0


@pytest.mark.parametrize("amplitude", [1e3, 1e-3])
def test_scene_off_unit_amplitude(amplitude):
    _, _, _, eo, et, _, out, taps, info = _scene(0.0, amplitude)
    e_out, e_taps = rel_err(out, eo), rel_err(taps, et)
    print(f"amplitude {amplitude:g}: out {e_out:.2e}, taps {e_taps:.2e}")
    assert info == 0 and e_out <= 1e-4 and e_taps <= TAPS128_BAR


# (name, n, filterLen, peek, Fs, bins): one tap, one bin | T just past a wavefront, n a multiple of no tile, more than one
# chunk of the correlation | the most bins | no peek | bins in kHz, where the float32 phase of the ramp matters
SHAPES = [("T1_B1", 257, 1, 0, 1.0, (0.0,)),
          ("T65_B5", 12011, 55, 10, 2.0 * 12011, (0.0, 1.0, -1.0, 2.0, -2.0)),
          ("B8_T16", 4099, 6, 10, 2.0 * 4099, (0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0)),
          ("peek0", 4099, 16, 0, 2.0 * 4099, (0.0, 1.0, -1.0)),
          ("kHz", 12000, 16, 10, 1.0e5, (0.0, 1500.0, -1500.0))]


@pytest.mark.parametrize("name,n,L,peek,fs,bins", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(name, n, L, peek, fs, bins):
    rng = np.random.default_rng(8100 + n + L)
    ref = _cwhite(rng, n)
    srv = _surveillance(rng, ref, fs, bins)
    eo, et, (G, _, _) = E.ECA_Filter(ref, srv, L, fs, bins, peek, 0.0, True, True)
    _, ets = E.ECA_Filter(ref, srv, L, fs, bins, peek, 0.0, True, shift=_device_shift)
    out, taps, info = _run(ref, srv, L, peek, fs, bins)
    cond = float(np.linalg.cond(G))
    e_out, e_taps, e_solve = rel_err(out, eo), rel_err(taps, et), rel_err(taps, ets)
    print(f"{name}: cond {cond:.3g}, out {e_out:.2e}, taps {e_taps:.2e}, on the device's regressors {e_solve:.2e}")
    assert info == 0 and cond <= 1e5
    assert e_out <= 1e-4
    # the taps against the plain restatement carry the float32 ramp's last bit times cond(G) (TAPS128_BAR above: 4.2e-7 on
    # B8_T16, below 2e-9 elsewhere); the solve itself is held on equal regressors
    assert e_solve <= solve_bar(cond)


def _one_bin(f, fs):
    from oracle import np_oracle as O
    from passiveradar_amd.clutter_removal import ECA_Filter, LS_Filter_Multiple
    rng = np.random.default_rng(8200)
    n, L = 12000, 16
    ref = _cwhite(rng, n)
    srv = _surveillance(rng, ref, fs, (f,))
    out, taps = ECA_Filter(ref, srv, L, fs, [f], return_filter=True)
    assert out.dtype == np.complex128 and taps.dtype == np.complex128 and taps.shape == (1, L + 10)
    chain = LS_Filter_Multiple(ref, srv, L, fs, [f])
    exp = O.LS_Filter_Multiple(ref, srv, L, fs, [f])
    return rel_err(out, chain), rel_err(out, exp), rel_err(chain, exp)


@pytest.mark.parametrize("f,fs", [(0.0, 1.0), (50.0, 1.0e4)])
def test_one_bin_is_the_chain_with_one_bin(f, fs):
    """B = 1 against prc_ls_execute with nbins = 1 (LS_Filter_Multiple on the device), within 1e-4
    (measured on MI355X: 4.0e-7 at 0 Hz, 5.7e-5 at 50 Hz of 10 kHz)"""
    e_chain, e_oracle, chain_oracle = _one_bin(f, fs)
    print(f"bin {f:g} Hz: ECA_Filter against the device's one-bin chain {e_chain:.2e}, against the oracle's {e_oracle:.2e}; "
          f"the device's chain against the oracle's {chain_oracle:.2e}")
    assert e_chain <= 1e-4 and e_oracle <= 1e-4


def test_one_kHz_bin_is_the_oracles_chain_with_one_bin():
    """One bin of -1.5 kHz at 100 kHz, the whole clutter (amplitude 1) on it: ECA_Filter is held to the ORACLE's one-bin chain
    (LS_Filter_Toeplitz on the float32-phase shifted reference) within 1e-4; measured 1.9e-7 on MI355X.  Against the
    device's chain it measured 2.1e-4, and that is the chain's own distance to the oracle's chain on this input (2.1e-4):
    presumably its FFT kernels rotating by the ramp's effective slope, not by its float32 phases (about 6e-5 rad apart at a
    phase of 1100 rad), which shows when the dominant clutter sits on such a bin.  Both distances are printed; the chain is
    not this canceller's to change."""
    e_chain, e_oracle, chain_oracle = _one_bin(-1500.0, 1.0e5)
    print(f"bin -1500 Hz: ECA_Filter against the oracle's one-bin chain {e_oracle:.2e}, against the device's {e_chain:.2e}; "
          f"the device's chain against the oracle's {chain_oracle:.2e}")
    assert e_oracle <= 1e-4


def test_dead_air_surveillance():
    """a silent srv: exactly zero out and taps, no flag"""
    ref = _scene(0.0)[0]
    out, taps, info = _run(ref, np.zeros_like(ref), E.SCENE_L, E.SCENE_PEEK, E.SCENE_FS, E.SCENE_BINS)
    assert info == 0 and not out.any() and not taps.any()


def test_batch_equals_single_calls_and_repeats():
    """three blocks (the scene, a silent reference, another white block) in one call with stride > n and another out_stride ==
    three single calls, bit for bit; the same call twice gives the same bits"""
    n, L, peek, fs, bins = 4099, 6, 10, 2.0 * 4099, (0.0, 1.0, -1.0)
    stride, ostride = n + 37, n + 5
    rng = np.random.default_rng(8300)
    refs = np.zeros((3, stride), np.complex64)
    srvs = np.zeros((3, stride), np.complex64)
    refs[0, :n], refs[2, :n] = _cwhite(rng, n), _cwhite(rng, n)
    for b in range(3):
        srvs[b, :n] = _surveillance(rng, refs[b, :n], fs, bins) if b != 1 else _cwhite(rng, n)
    first = _call(refs, srvs, n, L, peek, fs, bins, 0.0, stride, ostride)
    again = _call(refs, srvs, n, L, peek, fs, bins, 0.0, stride, ostride)
    for x, y in zip(first, again):
        assert np.array_equal(_bits(x), _bits(y))
    assert tuple(first[2]) == (0, 1, 0)
    for b in range(3):
        out, taps, info = _run(refs[b, :n], srvs[b, :n], L, peek, fs, bins)
        assert np.array_equal(_bits(first[0][b]), _bits(out)), b
        assert np.array_equal(_bits(first[1][b]), _bits(taps)), b
        assert first[2][b] == info, b
    eo = E.ECA_Filter(refs[2, :n], srvs[2, :n], L, fs, bins, peek)
    assert rel_err(first[0][2], eo) <= 1e-4


@pytest.mark.parametrize("gap", [1, 4099])
def test_guard_bands(gap):
    """prc_eca_execute: inputs poisoned outside their blocks; out, taps_out, info_out and the workspace at its queried size
    guarded; two blocks"""
    import torch
    import guard
    from passiveradar_amd import engine
    NS, n, L, peek, fs, bins = 2, 1021, 27, 10, 2.0 * 1021, (0.0, 1.0, -1.0)
    T, B = L + peek, len(bins)
    rng = np.random.default_rng(8400)
    ref = np.stack([_cwhite(rng, n) for _ in range(NS)])
    srv = np.stack([_surveillance(rng, ref[b], fs, bins) for b in range(NS)])
    wsb = engine.eca_workspace_bytes(n, L, peek, B, NS)
    assert wsb % 16 == 0
    dev = lambda a: torch.from_numpy(a).cuda()
    ins = {"ref": guard.In(dev(ref), n + gap), "srv": guard.In(dev(srv), n + gap)}
    outs = {"out": guard.Out(NS, n, torch.complex64, n + gap + 5),
            "taps": guard.Out(1, NS * B * T, torch.complex128), "info": guard.Out(1, NS, torch.int32),
            # the workspace: 16-byte elements keep it aligned behind the guard's odd lead; nothing in it is promised
            "ws": guard.Out(1, wsb // 16, torch.complex128, promised=torch.zeros((1, wsb // 16), dtype=torch.bool), finite=False)}

    def run(a, s):
        engine.eca_execute(a["ref"], a["srv"], a["out"], n, L, peek, fs, bins, 0.0, NS, s["ref"], s["out"], a["taps"], a["info"],
                           a["ws"])
        torch.cuda.synchronize()
    got = guard.check(run, ins, outs)
    b = NS - 1
    eo, et = E.ECA_Filter(ref[b], srv[b], L, fs, bins, peek, 0.0, True)
    out = got.tight["out"].cpu().numpy()[b]
    taps = got.tight["taps"].cpu().numpy().reshape(NS, B, T)[b]
    assert rel_err(out, eo) <= 1e-4 and rel_err(taps, et) <= TAPS128_BAR
    assert not got.tight["info"].cpu().numpy().any()


def test_duplicate_bins_break_down_and_reg_repairs_them():
    """bins [0, 0] with reg = 0: the block is flagged, out is srv bit for bit, the taps are zero; with reg = 1e-3 R_0[0][0] the
    recursion runs and matches the restatement with the same reg"""
    from passiveradar_amd import _lib
    from passiveradar_amd.clutter_removal import ECA_Filter
    ref, srv = _scene(0.0)[:2]
    out, taps, info = _run(ref, srv, E.SCENE_L, E.SCENE_PEEK, E.SCENE_FS, (0.0, 0.0))
    assert info == 1 and np.array_equal(_bits(out), _bits(srv)) and not taps.any()
    with pytest.raises(_lib.PrcoreError):
        ECA_Filter(ref, srv, E.SCENE_L, E.SCENE_FS, [0.0, 0.0])
    reg = 1e-3 * float(np.sum(np.abs(ref.astype(np.complex128)) ** 2))
    out, taps, info = _run(ref, srv, E.SCENE_L, E.SCENE_PEEK, E.SCENE_FS, (0.0, 0.0), reg)
    eo, et = E.ECA_Filter(ref, srv, E.SCENE_L, E.SCENE_FS, (0.0, 0.0), E.SCENE_PEEK, reg, True)
    print(f"duplicate bins, reg 1e-3 R0: out {rel_err(out, eo):.2e}, taps {rel_err(taps, et):.2e}")
    assert info == 0 and rel_err(out, eo) <= 1e-4 and rel_err(taps, et) <= 1e-4


def test_silent_reference():
    """an all-zero reference with reg = 0: flagged, out is srv bit for bit, zero taps, nothing non-finite"""
    srv = _scene(0.0)[1]
    out, taps, info = _run(np.zeros_like(srv), srv, E.SCENE_L, E.SCENE_PEEK, E.SCENE_FS, E.SCENE_BINS)
    assert info == 1 and np.array_equal(_bits(out), _bits(srv)) and not taps.any()


def test_graph_capture_and_replay():
    """the call enqueues a fixed set of launches and reads nothing back: captured on one stream and replayed twice == eager"""
    import torch
    from passiveradar_amd import _lib, engine
    ref, srv, _, _, _, _, out_e, taps_e, _ = _scene(0.0)
    n, L, peek, B = ref.shape[0], E.SCENE_L, E.SCENE_PEEK, len(E.SCENE_BINS)
    r, s = torch.from_numpy(ref).cuda(), torch.from_numpy(srv).cuda()
    out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    taps = torch.zeros((B, L + peek), dtype=torch.complex128, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(engine.eca_workspace_bytes(n, L, peek, B, 1), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            engine.eca_execute(r, s, out, n, L, peek, E.SCENE_FS, E.SCENE_BINS, 0.0, 1, n, n, taps, info, ws, _lib.torch_stream_ptr())
    side.synchronize()
    for k in range(2):
        out.zero_()
        taps.zero_()
        info.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(out_e)), k
        assert np.array_equal(_bits(taps.cpu().numpy()), _bits(taps_e)), k
        assert int(info.cpu()[0]) == 0


def test_backend_equals_drop_in():
    """HipBackend(clutter='eca') on a short stream: chunk c of clean() == ECA_Filter on that chunk, bit for bit; the maps
    through StreamProcessor are finite"""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.clutter_removal import ECA_Filter
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    C, R, F, nch = 8192, 16, 64, 4
    fs = 2.0 * C
    ref, srv = scene.make_stream(nch, C, fs, R, 778)
    be = HipBackend(2 * C, R, F, fs, clutter="eca", batch=4, ls_reg=0.0)
    got = StreamProcessor(be).process(ref, srv).cpu().numpy()
    assert got.shape[1:] == (F, R + 1) and np.isfinite(got).all() and np.abs(got).max() > 0
    cl = be.clean(be.padded(ref), be.padded(srv), nch)
    torch.cuda.synchronize()
    cl = cl.cpu().numpy()
    for i in range(nch):
        want = ECA_Filter(ref[i * C:(i + 1) * C], srv[i * C:(i + 1) * C], R, fs, list(be.bins))
        assert np.array_equal(cl[C // 2 + i * C:C // 2 + (i + 1) * C].astype(np.complex128), want), i
    eo = E.ECA_Filter(ref[:C], srv[:C], R, fs, be.bins, 10)
    assert rel_err(cl[C // 2:C // 2 + C], eo) <= 1e-4


def test_drop_in_raises_on_a_length_mismatch():
    from passiveradar_amd.clutter_removal import ECA_Filter
    with pytest.raises(ValueError):
        ECA_Filter(np.zeros(4096, np.complex64), np.zeros(4095, np.complex64), 16, 1.0)


def test_entry_point_refuses_what_is_outside_its_limits():
    """prc_eca_execute: 1 <= T < n; 1 <= nbins <= 8; nbins T <= 4096; strides >= n; reg >= 0 -- PRC_EINVAL (ValueError)"""
    import torch
    from passiveradar_amd import engine
    n, L, peek = 8192, 16, 10
    x = torch.zeros(n + 64, dtype=torch.complex64, device="cuda")
    out = torch.zeros(n + 64, dtype=torch.complex64, device="cuda")
    ws = torch.empty(engine.eca_workspace_bytes(n, 502, 10, 8, 1), dtype=torch.uint8, device="cuda")

    def call(n=n, L=L, peek=peek, bins=(0.0, 1.0), reg=0.0, nblocks=1, stride=None, ostride=None, fs=2.0 * n, ws=ws):
        engine.eca_execute(x, x, out, n, L, peek, fs, bins, reg, nblocks, stride, ostride, None, None, ws)

    call()                                                   # the baseline is accepted
    torch.cuda.synchronize()
    bad = [dict(L=0, peek=0), dict(n=26), dict(n=10), dict(L=-1), dict(peek=-1), dict(bins=()), dict(bins=(0.0,) * 9),
           dict(L=503, bins=tuple(float(i) for i in range(8))), dict(L=4087, bins=(0.0,)), dict(stride=n - 1), dict(ostride=n - 1),
           dict(reg=-1.0), dict(reg=float("nan")), dict(nblocks=0), dict(fs=0.0), dict(ws=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
