"""Every signal-processing entry point off unit amplitude (part A) and on dead air (part B), on the MI355X.

A. Amplitude ladder (tests/signal_edges.py): ref * 2^a, srv * 2^b over LADDER.  An entry point without an absolute constant
must return its scale-0 result times the right power of two BIT FOR BIT; the scale-0 result is held to the oracle at the bar
of the entry point's own test file.  The entry points that carry the reference's absolute constants (GAL_JPE, CFAR_2D,
LS_Filter with reg, LS_Filter_SVD) are held to their oracle at every rung instead, one rung placed where the constant is
comparable to what it guards.

B. Dead air: silent streams, dropouts shorter and longer than the filter, constant recordings.  Where the oracle is finite
the existing bars hold; where it is not, the non-finite rule (``nonfinite_rule``) holds and what the device leaves in the
oracle's non-finite region is asserted as recorded in INTEGRATION.md, section "Degenerate input".

Bars (none is new): TOL / TIGHT of tests/test_gpu_parity.py, BAR / NORM_BAR of tests/test_gpu_preproc.py, REL_BAR / DB_BAR
of tests/test_gpu_psd.py, 5e-6 for decimate_iir and 2e-6 (absolute, unit input) for frequency_shift as in
tests/test_gpu_parity.py, out 1e-4 / k, h 2e-4 of tests/test_gpu_gal.py, out 1e-4 of tests/test_gpu_ls_svd.py.  The oracles
run once per shape at scale 0; tests/test_signal_edges_host.py proves that scaling them exactly is legitimate."""
import functools

import numpy as np
import pytest

import preproc_oracle as PO
import psd_oracle as P
import signal_edges as E
from conftest import rel_err
from gal_oracle import gal_jpe
from ls_svd_oracle import ls_filter_svd
from oracle import c_oracle
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL, TIGHT = 1e-4, 2e-5
BAR, NORM_BAR = 4e-6, 2e-6
REL_BAR, DB_BAR = 2e-6, 0.01
IIR_BAR, SHIFT_BAR = 5e-6, 2e-6
GAL_OUT, GAL_KH = 1e-4, 2e-4
SVD_OUT = 1e-4
FS = 2.4e6


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    yield


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()          # a copy: the shared inputs are read-only


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ladder(name, run, ref, srv, degrees, rungs=E.LADDER):
    """run(ref, srv) at scale 0 and at every rung; every returned array i, of degree degrees[i] in (ref, srv), must be the
    scale-0 array times 2^(da a + db b) in every bit.  Returns the scale-0 arrays (the caller holds them to the oracle)."""
    base = _tuple(run(ref, srv))
    assert len(base) == len(degrees)
    broke = []
    for a, b in rungs:
        got = _tuple(run(E.scaled(ref, a), E.scaled(srv, b)))
        for i, (da, db) in enumerate(degrees):
            r = E.diff_report(got[i], E.expected(base[i], da, db, a, b))
            if r:
                broke.append(f"{name} [{i}] at (2^{a}, 2^{b}): {r}")
    assert not broke, "not the scale-0 bits times a power of two:\n  " + "\n  ".join(broke)
    return base


def per_scale(name, run, oracle, ref, srv, bars, rungs):
    """for the entry points with an absolute constant: every rung against the oracle of the SAME scaled input (which must
    be finite there: a rung at which the reference's own recursion runs away is no rung)"""
    worst = {}
    for a, b in ((0, 0),) + tuple(rungs):
        r, s = E.scaled(ref, a), E.scaled(srv, b)
        got, want = _tuple(run(r, s)), _tuple(oracle(r, s))
        for i, bar in enumerate(bars):
            assert np.isfinite(want[i]).all(), (name, a, b, i)
            e = rel_err(got[i], want[i]) if np.any(want[i]) else float(np.abs(got[i]).max())
            worst[a, b, i] = e
            print(f"{name} [{i}] at (2^{a}, 2^{b}): {e:.3g} (bar {bar:g})")
    bad = {k: v for k, v in worst.items() if not v <= bars[k[2]]}
    assert not bad, (name, bad)


# =============================================================================================================================
# A. amplitude ladder
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def _caf_case(n, R, F, seed):
    ref, srv = E.pair(n, seed, min(R, 200), 1e5)
    w = np.kaiser(n, 5.0)
    exp = O.fast_xambg(ref, srv, R, F, n, w)
    exp.setflags(write=False)
    return ref, srv, w, exp


@pytest.mark.parametrize("doppler", [1, 2], ids=["rocfft_doppler", "column_doppler"])
@pytest.mark.parametrize("caf", [1, 2], ids=["direct", "fft1024"])
def test_ladder_caf(caf, doppler):
    from passiveradar_amd import range_doppler_processing as rdp
    n, R, F = E.CAF_N, E.CAF_R, E.CAF_F
    ref, srv, w, exp = _caf_case(n, R, F, 11)
    E.budget(exp, 1, 1)
    rdp.set_default_methods(caf=caf, doppler=doppler)
    try:
        assert (rdp.caf_plan_for(n, R, F).method, rdp.caf_plan_for(n, R, F).doppler) == (caf, doppler)
        (out,) = ladder("fast_xambg", lambda r, s: rdp.fast_xambg(r, s, R, F, n, w), ref, srv, [(1, 1)])
    finally:
        rdp.set_default_methods(caf=0, doppler=0)
    assert rel_err(out, exp) < TIGHT


@pytest.mark.parametrize("team8", [0, 1], ids=["four_waves", "eight_waves"])
def test_ladder_caf_team(team8):
    """the 4096-point segment kernel on the two-piece row, both team forms"""
    from passiveradar_amd import _lib, range_doppler_processing as rdp
    n, R, F = E.CAF_TEAM
    ref, srv, w, exp = _caf_case(n, R, F, 12)
    E.budget(exp, 1, 1)
    rdp.set_default_methods(caf=3)
    old = _lib.set_option(_lib.OPT_CAF_TEAM8, team8)
    try:
        (out,) = ladder("fast_xambg", lambda r, s: rdp.fast_xambg(r, s, R, F, n, w), ref, srv, [(1, 1)])
    finally:
        _lib.set_option(_lib.OPT_CAF_TEAM8, old)
        rdp.set_default_methods(caf=0)
    assert rel_err(out, exp) < TIGHT


@pytest.mark.parametrize("mode", ["turns", "shared", "pairs"])
def test_ladder_caf_multi(mode):
    """two illuminators at DIFFERENT exponents (a, a - 3) against one surveillance channel at b"""
    from passiveradar_amd import range_doppler_processing as rdp
    n, R, F = E.CAF_MULTI
    ref0, srv, w, exp0 = _caf_case(n, R, F, 13)
    ref1 = E.pair(n, 14, 200, 1e5)[0]
    exp1 = _caf_multi_second(n, R, F)
    rdp.set_default_methods(caf=3)
    try:
        base = rdp.fast_xambg_multi([ref0, ref1], srv, R, F, n, w, mode=mode)
        broke = []
        for a, b in E.LADDER:
            got = rdp.fast_xambg_multi([E.scaled(ref0, a), E.scaled(ref1, a - 3)], E.scaled(srv, b), R, F, n, w, mode=mode)
            for i, e in enumerate((a + b, a - 3 + b)):
                r = E.diff_report(got[i], E.scaled(base[i], e))
                if r:
                    broke.append(f"illuminator {i} at (2^{a}, 2^{b}): {r}")
        assert not broke, "\n  ".join(broke)
    finally:
        rdp.set_default_methods(caf=0)
    assert rel_err(base[0], exp0) < TIGHT and rel_err(base[1], exp1) < TIGHT


@functools.lru_cache(maxsize=None)
def _caf_multi_second(n, R, F):
    _, srv, w, _ = _caf_case(n, R, F, 13)
    return O.fast_xambg(E.pair(n, 14, 200, 1e5)[0], srv, R, F, n, w)


def test_ladder_xcorr():
    from passiveradar_amd.signal_utils import xcorr
    ref, srv = E.pair(4096, 15)
    exp = O.xcorr(ref, srv, 7, 20)
    E.budget(exp, 1, 1)
    (z,) = ladder("xcorr", lambda r, s: xcorr(r, s, 7, 20), ref, srv, [(1, 1)])
    assert rel_err(z, exp) < TIGHT


@pytest.mark.parametrize("detrend", ["none", "mean"])
def test_ladder_welch(detrend):
    """psd is of degree 2 in its one input, csd of degree (1, 1)"""
    from passiveradar_amd.spectral import csd, psd
    kw = dict(NFFT=256, Fs=FS, detrend=detrend, noverlap=37)
    x = P.white(9 * 256 + 3, 11)
    y = (np.roll(x, 5) * (0.5 - 0.2j) + 0.1 * P.white(x.shape[0], 31)).astype(np.complex64)
    ep, ec = P.psd(x, **kw), P.csd(x, y, **kw)
    E.budget(ep, 2, 0)
    E.budget(ec, 1, 1)
    p, c = ladder("psd, csd", lambda r, s: (psd(r, **kw)[0], csd(r, s, **kw)[0]), x, y, [(2, 0), (1, 1)])
    rel, db = float(np.abs(p - ep).max() / ep.max()), float(np.abs(10 * np.log10(p / ep)).max())
    assert rel <= REL_BAR and db <= DB_BAR, (rel, db)
    assert float(np.abs(c - ec).max() / np.abs(ec).max()) <= REL_BAR


@functools.lru_cache(maxsize=None)
def _ls_case(n, L, seed):
    ref, srv = E.pair(n, seed, 20, E.LS_FS)
    out, taps = O.LS_Filter_Toeplitz(ref, srv, L, 10, True)
    chain = O.LS_Filter_Multiple(ref, srv, L, E.LS_FS, list(E.LS_BINS))
    for a in (out, taps, chain):
        a.setflags(write=False)
    return ref, srv, out, taps, chain


def _with_ls_method(method, fn):
    from passiveradar_amd import clutter_removal as cr
    cr.set_default_ls_method(method)
    try:
        return fn(cr)
    finally:
        cr.set_default_ls_method(0)


def _ls_ladder(method, n, L, seed):
    ref, srv, eout, etaps, echain = _ls_case(n, L, seed)
    E.budget(eout, 0, 1)
    E.budget(etaps, -1, 1)
    out, taps = _with_ls_method(method, lambda cr: ladder(
        "LS_Filter_Toeplitz", lambda r, s: cr.LS_Filter_Toeplitz(r, s, L, 10, True), ref, srv, [(0, 1), (-1, 1)]))
    assert rel_err(taps, etaps) < TIGHT and rel_err(out, eout) < TIGHT
    (chain,) = _with_ls_method(method, lambda cr: ladder(
        "LS_Filter_Multiple", lambda r, s: cr.LS_Filter_Multiple(r, s, L, E.LS_FS, list(E.LS_BINS)), ref, srv, [(0, 1)]))
    assert rel_err(chain, echain) < TOL


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4], ids=["auto", "direct", "fft", "fft_cached", "fft4096_cached"])
def test_ladder_ls(method):
    _ls_ladder(method, E.LS_N, E.LS_L, 16)


def test_ladder_ls_team_kernels():
    """T = 800 > 769: beyond the 1024-point kernels"""
    _ls_ladder(0, E.LS_TEAM_N, E.LS_TEAM_L, 17)


def _ls_plan_call(plan, refs, srvs, bins=(0.0,), fs=1.0, reg=0.0):
    """one prc_ls_execute on [nblocks, n] host arrays: (out [nblocks, n] complex64, taps [nblocks, T] complex128)"""
    import torch
    from passiveradar_amd import _lib
    nb, n = refs.shape
    a, s = dev(refs), dev(srvs)
    out = torch.empty_like(s)
    taps = torch.empty((nb, plan.ntaps), dtype=torch.complex128, device="cuda")
    plan.execute(a, s, out, nb, n, n, fs, bins, reg, taps, _lib.torch_stream_ptr())
    return host(out), host(taps)


def test_ladder_ls_two_block_plan_call():
    """two blocks in one prc_ls_execute, each at its own pair of exponents: block 0 at (a, b), block 1 at (b, a)"""
    from passiveradar_amd import engine
    n, L = E.LS_N, E.LS_L
    r0, s0, eout0, etaps0, echain0 = _ls_case(n, L, 16)
    r1, s1, eout1, etaps1, echain1 = _ls_case(n, L, 18)
    plan = engine.LsPlan(n, L, 10, False, 2, 0)
    try:
        for bins, fs, degs in (((0.0,), 1.0, True), (E.LS_BINS, E.LS_FS, False)):
            out, taps = _ls_plan_call(plan, np.stack([r0, r1]), np.stack([s0, s1]), bins, fs)
            broke = []
            for a, b in E.LADDER:
                got, gt = _ls_plan_call(plan, np.stack([E.scaled(r0, a), E.scaled(r1, b)]),
                                        np.stack([E.scaled(s0, b), E.scaled(s1, a)]), bins, fs)
                for blk, (ea, eb) in enumerate(((a, b), (b, a))):
                    r = E.diff_report(got[blk], E.scaled(out[blk], eb)) or (degs and E.diff_report(gt[blk], E.scaled(taps[blk], eb - ea)))
                    if r:
                        broke.append(f"block {blk}, bins {bins} at (2^{ea}, 2^{eb}): {r}")
            assert not broke, "\n  ".join(broke)
            if degs:
                assert rel_err(out[0], eout0) < TIGHT and rel_err(out[1], eout1) < TIGHT
                assert rel_err(taps[0], etaps0) < TIGHT and rel_err(taps[1], etaps1) < TIGHT
            else:
                assert rel_err(out[0], echain0) < TOL and rel_err(out[1], echain1) < TOL
    finally:
        plan.close()


@functools.lru_cache(maxsize=None)
def _nlms_case(n, L, seed):
    ref, srv = E.pair(n, seed, 50)
    out, taps = c_oracle.nlms(ref, srv, L, E.NLMS_MU, 10)
    out.setflags(write=False)
    taps.setflags(write=False)
    return ref, srv, out, taps


@pytest.mark.parametrize("L,n", [(E.NLMS_L, E.NLMS_N), (E.NLMS_LONG_L, E.NLMS_LONG_N)], ids=["one_wavefront", "two_wavefronts"])
def test_ladder_nlms(L, n):
    """cold start, then a warm start from the first run's taps scaled by 2^(b - a) (what a caller who rescaled its
    recording would hand over): out of degree (0, 1), taps of degree (-1, 1)"""
    from passiveradar_amd.clutter_removal import NLMS_filter
    ref, srv, eout, etaps = _nlms_case(n, L, 19)
    E.budget(eout, 0, 1)
    E.budget(etaps, -1, 1)
    out, taps = ladder("NLMS_filter", lambda r, s: NLMS_filter(r, s, L, E.NLMS_MU, 10, None, True), ref, srv, [(0, 1), (-1, 1)])
    assert rel_err(out, eout) < TOL and rel_err(taps, etaps) < TOL
    wout, wtaps = NLMS_filter(ref, srv, L, 0.02, 10, taps, True)
    eo, et = c_oracle.nlms(ref, srv, L, 0.02, 10, taps)
    assert rel_err(wout, eo) < TOL and rel_err(wtaps, et) < TOL
    for a, b in E.LADDER:
        got, gt = NLMS_filter(E.scaled(ref, a), E.scaled(srv, b), L, 0.02, 10, E.scaled(taps, b - a), True)
        assert not E.diff_report(got, E.scaled(wout, b)) and not E.diff_report(gt, E.scaled(wtaps, b - a)), (a, b)


def _nlms_streams(refs, srvs, n, L, mu=E.NLMS_MU, taps_in=None):
    """prc_nlms_execute on [nstreams, stride] host arrays: (out [nstreams, stride], taps [nstreams, T])"""
    import torch
    from passiveradar_amd import engine
    ns, stride = refs.shape
    out = torch.zeros((ns, stride), dtype=torch.complex64, device="cuda")
    tout = torch.empty((ns, L + 10), dtype=torch.complex64, device="cuda")
    engine.nlms_execute(dev(refs), dev(srvs), out, n, L, mu, 10, None if taps_in is None else dev(taps_in), tout, ns, stride, stride)
    return host(out), host(tout)


@functools.lru_cache(maxsize=None)
def _stream_block(ns=E.NLMS_STREAMS, n=E.NLMS_STREAM_N, stride=E.NLMS_STRIDE, seed=20):
    base_ref, base_srv = E.pair(ns * 7 + n, seed, 50)
    ref = np.zeros((ns, stride), np.complex64)
    srv = np.zeros((ns, stride), np.complex64)
    for s in range(ns):
        ref[s, :n] = base_ref[7 * s:7 * s + n]
        srv[s, :n] = base_srv[7 * s:7 * s + n]
    ref.setflags(write=False)
    srv.setflags(write=False)
    return ref, srv


def test_ladder_nlms_streams():
    """several streams in one launch, stream i at exponents (a - i, b + i)"""
    ns, n, L = E.NLMS_STREAMS, E.NLMS_STREAM_N, E.NLMS_L
    ref, srv = _stream_block()
    out, taps = _nlms_streams(ref, srv, n, L)
    for s in range(ns):
        eo, et = c_oracle.nlms(ref[s, :n], srv[s, :n], L, E.NLMS_MU, 10)
        assert rel_err(out[s, :n], eo) < TOL and rel_err(taps[s], et) < TOL, s
    for a, b in E.LADDER:
        r = np.stack([E.scaled(ref[s], a - s) for s in range(ns)])
        v = np.stack([E.scaled(srv[s], b + s) for s in range(ns)])
        got, gt = _nlms_streams(r, v, n, L)
        for s in range(ns):
            assert not E.diff_report(got[s], E.scaled(out[s], b + s)), (a, b, s)
            assert not E.diff_report(gt[s], E.scaled(taps[s], b - a + 2 * s)), (a, b, s)


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("method", [1, 2], ids=["one_output_per_thread", "group"])
def test_ladder_front_end(method, fold):
    """float32 recordings through the fused front end (both kernel forms, folded tap rows on and off) and resample"""
    from passiveradar_amd import _lib
    from passiveradar_amd.signal_utils import front_end, resample
    up, dn, n_in, nblk = 3, 7, 700, 3
    raw = E.raw_float32(2 * n_in * nblk, 21)
    x = E.white(5000, 22)
    args = (2 * n_in, 100_000, 2_400_000, up, dn)
    exp, exr = O.front_end(raw, *args), O.resample(x, up, dn)
    E.budget(exp, 1, 0)
    old = _lib.get_option(_lib.OPT_FE_METHOD), _lib.get_option(_lib.OPT_FE_FOLD)
    _lib.set_option(_lib.OPT_FE_METHOD, method)
    _lib.set_option(_lib.OPT_FE_FOLD, fold)
    try:
        (y,) = ladder("front_end", lambda r, s: front_end(r, *args, max_blocks=2), raw, raw, [(1, 0)])
        (z,) = ladder("resample", lambda r, s: resample(r, up, dn), x, x, [(1, 0)])
    finally:
        _lib.set_option(_lib.OPT_FE_METHOD, old[0])
        _lib.set_option(_lib.OPT_FE_FOLD, old[1])
    assert rel_err(y, exp) < TIGHT and rel_err(z, exr) < TIGHT


def test_ladder_frequency_shift_and_decimators():
    from passiveradar_amd.signal_utils import channel_preprocessing, decimate, decimate_iir, frequency_shift
    x = E.pair(5000, 23)[0]
    raw = E.raw_float32(2 * 2001, 24)
    ef = O.frequency_shift(x, 37.5, 1e4, 0.3)
    (y,) = ladder("frequency_shift", lambda r, s: frequency_shift(r, 37.5, 1e4, 0.3), x, x, [(1, 0)])
    assert np.abs(y - ef).max() < SHIFT_BAR
    ei = O.decimate_iir(x, 4)
    E.budget(ei, 1, 0)
    (y,) = ladder("decimate_iir", lambda r, s: decimate_iir(r, 4), x, x, [(1, 0)])
    assert rel_err(y, ei) < IIR_BAR
    for q in (4, 97):                                            # the tile form and the direct form
        (y,) = ladder(f"decimate q={q}", lambda r, s: decimate(r, q), x, x, [(1, 0)])
        assert rel_err(y, PO.decimate(x, q)) <= BAR, q
    (y,) = ladder("channel_preprocessing", lambda r, s: channel_preprocessing(r, 10, 1e5, FS), raw, raw, [(1, 0)])
    assert rel_err(y, PO.channel_preprocessing(raw, 10, 1e5, FS)) <= BAR


def test_ladder_normalize():
    """degree 0: the same bits at every amplitude"""
    from passiveradar_amd.signal_utils import normalize
    x = E.pair(5000, 25)[0]
    (y,) = ladder("normalize", lambda r, s: normalize(r), x, x, [(0, 0)])
    assert rel_err(y, PO.normalize(x)) <= NORM_BAR


# ---- the entry points that carry the reference's absolute constants: every rung against its own oracle ---------------------
def _gal_scene():
    from passiveradar_amd import scene
    ref, srv = scene.make_ar2_scene(E.GAL_N, 262144.0, 64, 9100)
    return ref[:E.GAL_N], srv[:E.GAL_N]


# the surveillance exponents of the ladder stop at 2^5 here: mu1 <- 0.999 mu1 + 1e-8 e^2 is of degree 2 in srv with an
# absolute constant, and from |srv| ~ 1e2 on the reference's own recursion (the float64 restatement too) leaves the finite
# range within a few hundred samples, from int16 level on within ten (test_gal_at_int16_level)
GAL_RUNGS = ((15, -7), (24, -15), (-24, 10), (-10, 5), (E.GAL_EDGE, -12))


def test_per_scale_gal():
    """P + 1e-10 and b^H b + 1e-10 (and mu1's 1e-8 e^2, P's start at 1e-8): one rung at 2^-17, where b^H b ~ 1e-10"""
    from passiveradar_amd.clutter_removal import GAL_JPE
    L, D = E.GAL_L, E.GAL_D
    ref, srv = _gal_scene()
    per_scale("GAL_JPE", lambda r, s: GAL_JPE(r, s, L, D, E.GAL_MU1, E.GAL_MU2, return_filter=True),
              lambda r, s: gal_jpe(r, s, L, D, E.GAL_MU1, E.GAL_MU2, 10, np.complex64, True), ref, srv,
              (GAL_OUT, GAL_KH, GAL_KH), GAL_RUNGS)


def test_gal_at_int16_level():
    """srv * 2^15: e^2 ~ 1e9 makes mu1 = 1e-8 e^2 of order 10 and of either sign, the reflection coefficients run away and
    the reference's recursion overflows float32 within ten samples (the float64 restatement lasts three samples longer).
    The device does the same: the call returns, twice with the same bits, out is not finite from the same sample on (as
    recorded), and the samples before the run-away takes off (within 8 times the input's peak) meet the bar; in the
    run-away itself every rounding error grows with it (2.7e-5 of the peak over the six samples up to 9e9)."""
    from passiveradar_amd.clutter_removal import GAL_JPE
    L, D = E.GAL_L, E.GAL_D
    ref, srv = _gal_scene()
    s15 = E.scaled(srv, 15)
    with np.errstate(all="ignore"):
        want = gal_jpe(ref, s15, L, D, E.GAL_MU1, E.GAL_MU2, 10, np.complex64, True)
    k = E.first_nonfinite(want[0])
    assert k is not None and k < 12
    got = GAL_JPE(ref, s15, L, D, E.GAL_MU1, E.GAL_MU2, return_filter=True)
    again = GAL_JPE(ref, s15, L, D, E.GAL_MU1, E.GAL_MU2, return_filter=True)
    print(f"GAL at 2^15: oracle out[:{k + 1}] {want[0][:k + 1]}\n             device out[:{k + 1}] {got[0][:k + 1]}")
    for g, a in zip(got, again):
        assert not E.diff_report(g, a)
    quiet = np.abs(want[0][:k]) < 8 * np.abs(s15).max()                      # before the run-away takes off
    calm = k if quiet.all() else int(np.argmin(quiet))
    e = rel_err(got[0][:calm], want[0][:calm])
    print(f"GAL at 2^15: the {calm} samples before the run-away: {e:.3g}; device first non-finite {E.first_nonfinite(got[0])}, oracle {k}")
    assert calm >= 3 and e <= GAL_OUT
    for i, name in enumerate(("out", "k", "h")):
        _recorded(("gal_int16", name), got[i])
    healthy = GAL_JPE(ref, srv, L, D, E.GAL_MU1, E.GAL_MU2, return_filter=True)
    want0 = gal_jpe(ref, srv, L, D, E.GAL_MU1, E.GAL_MU2, 10, np.complex64, True)
    assert rel_err(healthy[0], want0[0]) <= GAL_OUT                                   # the next call is not affected


@pytest.mark.parametrize("method", [0, 1], ids=["separable", "every_tap"])
def test_per_scale_cfar(method):
    """box + 1e-10: one rung at 2^-33, where the box mean is ~ 1e-10"""
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import CFAR_2D, CFAR_2D_abs
    rng = np.random.default_rng(33064)
    H, W, fw, gw = E.CFAR_H, E.CFAR_W, E.CFAR_FW, E.CFAR_GW
    X = (rng.standard_normal((H, W)) + 1j * rng.standard_normal((H, W))).astype(np.complex64)
    rungs = tuple((a, a) for a, _ in E.LADDER) + ((E.CFAR_EDGE, E.CFAR_EDGE),)
    old = _lib.set_option(_lib.OPT_CFAR_METHOD, method)
    try:
        per_scale("CFAR_2D", lambda r, s: CFAR_2D(np.abs(r), fw, gw), lambda r, s: O.CFAR_2D(np.abs(r), fw, gw), X, X, (TIGHT,), rungs)
        per_scale("CFAR_2D_abs", lambda r, s: CFAR_2D_abs(r, fw, gw), lambda r, s: O.CFAR_2D(np.abs(r), fw, gw), X, X, (TIGHT,), rungs)
    finally:
        _lib.set_option(_lib.OPT_CFAR_METHOD, old)


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4], ids=["auto", "direct", "fft", "fft_cached", "fft4096_cached"])
def test_per_scale_ls_filter_reg(method):
    """reg = 1 on the Gram diagonal: one rung at 2^-7, where n |ref|^2 = 1"""
    ref, srv = E.pair(E.LS_N, 16, 20, E.LS_FS)
    L = E.LS_L
    _with_ls_method(method, lambda cr: per_scale(
        "LS_Filter", lambda r, s: cr.LS_Filter(r, s, L, 1.0, 10, True), lambda r, s: O.LS_Filter(r, s, L, 1.0, 10, True),
        ref, srv, (TOL, 5e-5), E.LADDER + ((E.LS_REG_EDGE, 3),)))


@pytest.mark.parametrize("rcond", [0.0, None], ids=["reference_cut", "default_cut"])
def test_per_scale_ls_svd(rcond):
    """max(1e-10, rcond sigma_max): one rung where every singular value is a few times the absolute cut, one below it
    (nothing is cancelled: out is srv)"""
    from passiveradar_amd.clutter_removal import LS_Filter_SVD
    n, L, peek = E.SVD_N, E.SVD_L, E.SVD_PEEK
    ref, srv = E.pair(n, 26)
    per_scale("LS_Filter_SVD", lambda r, s: LS_Filter_SVD(r, s, L, peek, rcond=rcond),
              lambda r, s: ls_filter_svd(r, s, L, peek, rcond)[0], ref, srv, (SVD_OUT,),
              E.LADDER + ((E.SVD_ABOVE, -30), (E.SVD_BELOW, -30)))
    r, s = E.scaled(ref, E.SVD_BELOW), E.scaled(srv, -30)
    out, taps = LS_Filter_SVD(r, s, L, peek, True, rcond=rcond)
    assert E.same_bits(out, s) and not taps.any()


# =============================================================================================================================
# B. dead air
# =============================================================================================================================
def describe(x):
    """what a region holds: counts of NaN, infinite and finite components and the first element that is not finite"""
    v = np.ascontiguousarray(x).reshape(-1)
    v = v.view(v.real.dtype)
    return {"nan": int(np.isnan(v).sum()), "inf": int(np.isinf(v).sum()), "finite": int(np.isfinite(v).sum()),
            "first": E.first_nonfinite(x)}


def nonfinite_rule(name, run, healthy, degenerate, item, oracle_item, bar, run_fresh=None):
    """The non-finite rule.  ``run(inputs)`` -> tuple of arrays [items, ...] (it raises when the call does not return
    success); ``degenerate`` is ``healthy`` with item ``item`` replaced by the degenerate input; ``oracle_item``: the oracle's
    first array for that item; ``run_fresh``: the same call on a fresh plan (None: the call path has no plan).
      1. the call returns success                          2. before the oracle's first non-finite sample the bar holds
      3. every other item has the bits of the launch without the degenerate item
      4. a second identical call returns the same bits     5. the same path, next on healthy input, returns a fresh one's bits
    Returns the degenerate item's arrays of the first call."""
    before = _tuple((run_fresh or run)(healthy))
    first = _tuple(run(degenerate))                                                            # 1
    again = _tuple(run(degenerate))
    after = _tuple(run(healthy))
    k = E.first_nonfinite(oracle_item)
    assert k is not None, "the oracle is finite here: not a case for this rule"
    if k > 0:                                                                                  # 2
        got, want = first[0][item].reshape(-1)[:k], np.asarray(oracle_item).reshape(-1)[:k]
        assert np.isfinite(got).all()
        e = rel_err(got, want) if np.any(want) else float(np.abs(got).max())
        print(f"{name}: the {k} samples before the oracle's first non-finite one: {e:.3g} (bar {bar:g})")
        assert e < bar, e
    others = [i for i in range(first[0].shape[0]) if i != item]
    for a, b in zip(first, before):                                                            # 3
        assert not E.diff_report(a[others], b[others]), name
    for a, b in zip(first, again):                                                             # 4
        assert not E.diff_report(a, b), name
    for a, b in zip(after, before):                                                            # 5
        assert not E.diff_report(a, b), name
    for i, a in enumerate(first):
        print(f"{name}: array {i} of the degenerate item from the oracle's first non-finite sample on: "
              f"{describe(a[item].reshape(-1)[k if i == 0 else 0:])}")
    return tuple(a[item] for a in first)


# ---- silent channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2, 3, 4], ids=["auto", "direct", "fft", "fft_cached", "fft4096_cached"])
def test_silent_srv_ls(method):
    """exactly zero out and exactly zero taps: Toeplitz and circular form, the three-bin chain, two blocks in a launch"""
    from passiveradar_amd import engine
    n, L = E.LS_N, E.LS_L
    ref, srv = E.pair(n, 16, 20, E.LS_FS)
    z = E.silent(n)

    def go(cr):
        out, taps = cr.LS_Filter_Toeplitz(ref, z, L, 10, True)
        assert not out.any() and not taps.any()
        assert not cr.LS_Filter_Multiple(ref, z, L, E.LS_FS, list(E.LS_BINS)).any()
        out, taps = cr.LS_Filter(ref, z, L, 1.0, 10, True)
        assert not out.any() and not taps.any()
    _with_ls_method(method, go)
    plan = engine.LsPlan(n, L, 10, False, 2, method)
    try:
        for bins, fs in (((0.0,), 1.0), (E.LS_BINS, E.LS_FS)):
            both, tb = _ls_plan_call(plan, np.stack([ref, ref]), np.stack([srv, srv]), bins, fs)
            out, taps = _ls_plan_call(plan, np.stack([ref, ref]), np.stack([z, srv]), bins, fs)
            assert not out[0].any() and not taps[0].any()
            assert E.same_bits(out[1], both[1]) and E.same_bits(taps[1], tb[1])       # the healthy block is not touched
    finally:
        plan.close()


def test_silent_srv_ls_team_kernels():
    from passiveradar_amd.clutter_removal import LS_Filter_Multiple, LS_Filter_Toeplitz
    ref, _ = E.pair(E.LS_TEAM_N, 17, 20, E.LS_FS)
    z = E.silent(E.LS_TEAM_N)
    out, taps = LS_Filter_Toeplitz(ref, z, E.LS_TEAM_L, 10, True)
    assert not out.any() and not taps.any()
    assert not LS_Filter_Multiple(ref, z, E.LS_TEAM_L, E.LS_FS, list(E.LS_BINS)).any()


def test_silent_srv_nlms_and_gal():
    import torch
    from passiveradar_amd import engine
    from passiveradar_amd.clutter_removal import GAL_JPE, NLMS_filter
    for L, n in ((E.NLMS_L, E.NLMS_N), (E.NLMS_LONG_L, E.NLMS_LONG_N)):
        ref = E.pair(n, 19, 50)[0]
        out, taps = NLMS_filter(ref, E.silent(n), L, E.NLMS_MU, 10, None, True)
        assert not out.any() and not taps.any(), L
    # one silent stream among healthy ones
    ns, n, L = E.NLMS_STREAMS, E.NLMS_STREAM_N, E.NLMS_L
    ref, srv = _stream_block()
    both, tb = _nlms_streams(ref, srv, n, L)
    quiet = np.array(srv)
    quiet[2] = 0
    out, taps = _nlms_streams(ref, quiet, n, L)
    assert not out[2].any() and not taps[2].any()
    others = [0, 1, 3, 4]
    assert E.same_bits(out[others], both[others]) and E.same_bits(taps[others], tb[others])
    # GAL: nothing is cancelled (out, h); the lattice still adapts to the reference (k) exactly as with a live srv ... one
    # stream, then one silent stream among three
    gref = E.pair(E.GAL_N, 27, 50)[0]
    gsrv = E.pair(E.GAL_N, 27, 50)[1]
    out, k, h = GAL_JPE(gref, E.silent(E.GAL_N), E.GAL_L, E.GAL_D, E.GAL_MU1, E.GAL_MU2, return_filter=True)
    assert not out.any() and not h.any() and k.any()
    n, D = E.GAL_N, E.GAL_D
    r3 = dev(np.stack([gref, gref, gref]))
    res = []
    for srv3 in (np.stack([gsrv, gsrv, gsrv]), np.stack([gsrv, E.silent(n), gsrv])):
        o = torch.zeros((3, n), dtype=torch.complex64, device="cuda")
        kb = torch.zeros((3, D), dtype=torch.complex64, device="cuda")
        hb = torch.zeros((3, D), dtype=torch.complex64, device="cuda")
        engine.gal_execute(r3, dev(srv3), o, n, E.GAL_L, D, E.GAL_MU1, E.GAL_MU2, 10, kb, hb, 3)
        res.append((host(o), host(kb), host(hb)))
    (o0, k0, h0), (o1, k1, h1) = res
    assert not o1[1].any() and not h1[1].any()
    for i in (0, 2):
        assert E.same_bits(o1[i], o0[i]) and E.same_bits(k1[i], k0[i]) and E.same_bits(h1[i], h0[i]), i


def test_silent_srv_ls_svd():
    from passiveradar_amd.clutter_removal import LS_Filter_SVD
    ref = E.pair(E.SVD_N, 26)[0]
    for rcond in (0.0, None):
        out, taps = LS_Filter_SVD(ref, E.silent(E.SVD_N), E.SVD_L, E.SVD_PEEK, True, rcond=rcond)
        assert not out.any() and not taps.any(), rcond


@pytest.mark.parametrize("caf,shape,seed", [(1, "small", 11), (2, "small", 11), (3, "multi", 13)], ids=["direct", "fft1024", "fft4096"])
def test_silent_channels_caf(caf, shape, seed):
    """silent srv, silent ref: an exactly zero map from every segment kernel, and from the multi call"""
    from passiveradar_amd import range_doppler_processing as rdp
    n, R, F = (E.CAF_N, E.CAF_R, E.CAF_F) if shape == "small" else E.CAF_MULTI
    ref, srv, w, _ = _caf_case(n, R, F, seed)
    z = E.silent(n)
    rdp.set_default_methods(caf=caf)
    try:
        assert not rdp.fast_xambg(ref, z, R, F, n, w).any()
        assert not rdp.fast_xambg(z, srv, R, F, n, w).any()
        if caf == 3:
            for mode in ("turns", "shared", "pairs"):
                healthy = rdp.fast_xambg_multi([ref, ref], srv, R, F, n, w, mode=mode)
                a, b = rdp.fast_xambg_multi([ref, z], srv, R, F, n, w, mode=mode)
                assert not b.any() and E.same_bits(a, healthy[0]), mode
                assert not any(m.any() for m in rdp.fast_xambg_multi([ref, ref], z, R, F, n, w, mode=mode)), mode
    finally:
        rdp.set_default_methods(caf=0)


def test_silent_ref_ls_filter_returns_srv():
    """reg = 1 is alone on the Gram diagonal: zero taps, out is srv bit for bit"""
    ref, srv = E.pair(E.LS_N, 16, 20, E.LS_FS)
    for method in (0, 1, 2, 3, 4):
        out, taps = _with_ls_method(method, lambda cr: cr.LS_Filter(E.silent(E.LS_N), srv, E.LS_L, 1.0, 10, True))
        assert E.same_bits(out, srv) and not taps.any(), method


# What the device leaves where the oracle is not finite ("Degenerate input"), as found on the MI355X: counts
# of NaN / infinite / finite float components of the region and its first element that is not finite.
def _all_nan(components):
    return {"nan": components, "inf": 0, "finite": 0, "first": 0}


def _all_finite(components):
    return {"nan": 0, "inf": 0, "finite": components, "first": None}


_T = E.NLMS_L + 10
RECORDED = {
    ("nlms_silent_ref_out",): _all_nan(2 * (E.NLMS_N - 10 - (E.NLMS_L + 1))),       # NaN like the oracle
    ("nlms_silent_ref_taps",): _all_nan(2 * _T),
    # a reference dropout longer than T (test_nlms_reference_dropout_longer_than_the_filter): finite while the slid u^H u is a
    # rounding residue, NaN from the step at which it is exactly 0
    ("nlms_dropout_out", 200, 14): _all_finite(2 * (E.NLMS_N - 10 - (E.NLMS_L + 200))),
    ("nlms_dropout_taps", 200, 14): _all_finite(2 * _T),
    ("nlms_dropout_out", 200, 30): {"nan": 2514, "inf": 0, "finite": 18, "first": 9},         # the update of step 208
    ("nlms_dropout_taps", 200, 30): _all_nan(2 * _T),
    ("nlms_dropout_out", 1010, 30): {"nan": 882, "inf": 0, "finite": 30, "first": 15},        # the update of step 1024
    ("nlms_dropout_taps", 1010, 30): _all_nan(2 * _T),
}
for _m in range(5):
    for _chain in (False, True):
        RECORDED["ls_silent_ref_out", _m, _chain] = _all_nan(2 * E.LS_N)            # an all-NaN block like the oracle
        RECORDED["ls_silent_ref_taps", _m, _chain] = _all_nan(2 * (E.LS_L + 10))    # complex128
RECORDED["gal_int16", "out"] = {"nan": 1364, "inf": 0, "finite": 36, "first": 7}    # NaN from out[7] on, like the restatement
RECORDED["gal_int16", "k"] = _all_nan(2 * E.GAL_D)
RECORDED["gal_int16", "h"] = _all_nan(2 * E.GAL_D)
for _m in range(2):
    for _abs in (False, True):
        RECORDED["cfar_zero_frame", _m, _abs] = _all_nan(E.CFAR_H * E.CFAR_W)       # 0 / 0 like the oracle


def _recorded(key, region):
    got = describe(region)
    print(f"recorded[{key}] = {got}")
    if key in RECORDED:
        assert got == RECORDED[key], (key, got, RECORDED[key])


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4], ids=["auto", "direct", "fft", "fft_cached", "fft4096_cached"])
@pytest.mark.parametrize("chain", [False, True], ids=["toeplitz", "three_bins"])
def test_silent_ref_ls_toeplitz(method, chain):
    """the oracle's Levinson recursion starts with 1 / c[0] = 1 / 0: an all-NaN block.  Block 0 of a two-block launch."""
    from passiveradar_amd import engine
    n, L = E.LS_N, E.LS_L
    r0, s0 = E.pair(n, 16, 20, E.LS_FS)
    r1, s1 = E.pair(n, 18, 20, E.LS_FS)
    bins, fs = (E.LS_BINS, E.LS_FS) if chain else ((0.0,), 1.0)
    with np.errstate(all="ignore"):
        exp = O.LS_Filter_Multiple(E.silent(n), s0, L, fs, list(bins))
    plan = engine.LsPlan(n, L, 10, False, 2, method)
    fresh = engine.LsPlan(n, L, 10, False, 2, method)
    try:
        out, taps = nonfinite_rule(
            f"LS silent ref, method {method}, bins {bins}", lambda x: _ls_plan_call(plan, x[0], x[1], bins, fs),
            (np.stack([r0, r1]), np.stack([s0, s1])), (np.stack([E.silent(n), r1]), np.stack([s0, s1])), 0, exp, TIGHT,
            lambda x: _ls_plan_call(fresh, x[0], x[1], bins, fs))
    finally:
        plan.close()
        fresh.close()
    _recorded(("ls_silent_ref_out", method, chain), out)
    _recorded(("ls_silent_ref_taps", method, chain), taps)


def _nlms_rule(name, ref_deg, L, n, stream_n=None):
    """stream 1 of a three-stream launch carries the degenerate reference"""
    ref, srv = E.pair(n, 19, 50)
    with np.errstate(all="ignore"):
        exp, _ = c_oracle.nlms(ref_deg, srv, L, E.NLMS_MU, 10)
    r1, s1 = E.pair(n, 28, 50)
    healthy = (np.stack([r1, ref, r1[::-1]]), np.stack([s1, srv, s1[::-1]]))
    degenerate = (np.stack([r1, ref_deg, r1[::-1]]), healthy[1])
    out, taps = nonfinite_rule(name, lambda x: _nlms_streams(np.ascontiguousarray(x[0]), np.ascontiguousarray(x[1]), n, L),
                               healthy, degenerate, 1, exp, TOL)
    return exp, out, taps


def test_silent_ref_nlms():
    """u^H u = 0 from the first step: the oracle's first output is srv[L] (zero taps), its update 0 / 0"""
    L, n = E.NLMS_L, E.NLMS_N
    exp, out, taps = _nlms_rule("NLMS silent ref", E.silent(n), L, n)
    assert E.first_nonfinite(exp) == L + 1
    _recorded(("nlms_silent_ref_out",), out[L + 1:n - 10])
    _recorded(("nlms_silent_ref_taps",), taps)


@pytest.mark.parametrize("start,extra", [(200, 14), (200, 30), (1010, 30)],
                         ids=["inside_a_window_residue", "inside_a_window_exact_zero", "across_a_window"])
def test_nlms_reference_dropout_longer_than_the_filter(start, extra):
    """ref[start:start + T + extra] = 0.  The oracle is finite through out[L + start - 1] and never again.  The device slides
    u^H u in double inside a staged window of 1024 steps, every lane from its own prefix of the window, and sums it afresh at
    the start of the next window.  Inside the run of zeros the slid sum is a rounding residue: while it is not 0 the step is
    finite, the update is that step times u = 0 and the taps wait (200, 14: finite to the end); where a lane's prefix cancels
    exactly (200, 30: step 208) or a window starts inside the run (1010, 30: step 1024, tap window ref[1025 .. 1058]) the
    sum is exactly 0, the step is infinite and the taps are NaN from there on, like the oracle's."""
    L, n = E.NLMS_L, E.NLMS_N
    ref = E.pair(n, 19, 50)[0]
    exp, out, taps = _nlms_rule(f"NLMS dropout at {start}", E.hole(ref, start, L + 10 + extra), L, n)
    first = E.nlms_first_nonfinite(L, start)
    assert E.first_nonfinite(exp) == first and np.isfinite(out[:first]).all()
    _recorded(("nlms_dropout_out", start, extra), out[first:n - 10])
    _recorded(("nlms_dropout_taps", start, extra), taps)


@pytest.mark.parametrize("L,n,short,at", [(E.NLMS_L, E.NLMS_N, E.NLMS_L + 4, 1020), (E.NLMS_LONG_L, E.NLMS_LONG_N, 100, 2300)],
                         ids=["one_wavefront", "two_wavefronts"])
def test_nlms_short_dropouts_and_srv_dropouts(L, n, short, at):
    """a dropout shorter than T in ref (at L = 24 across the staged-window boundary at step 1024, where u^H u is summed
    afresh), in srv, in both, and at L = 24 a dropout of srv longer than T: the oracle is finite, the bar holds"""
    from passiveradar_amd.clutter_removal import NLMS_filter
    ref, srv = E.pair(n, 19, 50)
    T = L + 10
    cases = [("ref", E.hole(ref, at, short), srv), ("srv", ref, E.hole(srv, at, short)),
             ("both", E.hole(ref, at, short), E.hole(srv, at, short))]
    if T + 50 < n // 4:
        cases.append(("srv, longer than T", ref, E.hole(srv, 1000, T + 50)))
    for name, r, s in cases:
        eo, et = c_oracle.nlms(r, s, L, E.NLMS_MU, 10)
        assert np.isfinite(eo).all() and np.isfinite(et).all()
        out, taps = NLMS_filter(r, s, L, E.NLMS_MU, 10, None, True)
        e_out, e_taps = rel_err(out, eo), rel_err(taps, et)
        print(f"NLMS L {L} dropout in {name}: out {e_out:.3g} taps {e_taps:.3g}")
        assert e_out < TOL and e_taps < TOL, (name, e_out, e_taps)


def test_gal_dropouts():
    """dropouts shorter (30) and longer (100) than the delay line of 64 in ref, in srv, in both: with the delay line empty
    b^H b + 1e-10 is the constant alone.  The restatement is finite; the bars of tests/test_gpu_gal.py hold."""
    from passiveradar_amd.clutter_removal import GAL_JPE
    L, D = E.GAL_L, E.GAL_D
    ref, srv = _gal_scene()
    for m in (30, 100):
        for name, r, s in (("ref", E.hole(ref, 300, m), srv), ("srv", ref, E.hole(srv, 300, m)),
                           ("both", E.hole(ref, 300, m), E.hole(srv, 300, m))):
            want = gal_jpe(r, s, L, D, E.GAL_MU1, E.GAL_MU2, 10, np.complex64, True)
            assert all(np.isfinite(w).all() for w in want)
            got = GAL_JPE(r, s, L, D, E.GAL_MU1, E.GAL_MU2, return_filter=True)
            errs = [rel_err(g, w) for g, w in zip(got, want)]
            print(f"GAL dropout of {m} in {name}: out {errs[0]:.3g} k {errs[1]:.3g} h {errs[2]:.3g}")
            assert errs[0] <= GAL_OUT and errs[1] <= GAL_KH and errs[2] <= GAL_KH, (m, name, errs)


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4], ids=["auto", "direct", "fft", "fft_cached", "fft4096_cached"])
def test_ls_dropouts(method):
    """dropouts of 20 (< T = 42) and 200 samples across the piece boundaries of the overlap-save kernels (983 k of the
    1024-point chain at 3932, 4055 of the 4096-point chain), in ref, in srv, in both: the oracle is finite, the bars hold"""
    n, L = E.LS_N, E.LS_L
    ref, srv = E.pair(n, 16, 20, E.LS_FS)

    def go(cr):
        for m, at in ((20, 4045), (200, 3900)):
            for name, r, s in (("ref", E.hole(ref, at, m), srv), ("srv", ref, E.hole(srv, at, m)),
                               ("both", E.hole(ref, at, m), E.hole(srv, at, m))):
                eo, et = O.LS_Filter_Toeplitz(r, s, L, 10, True)
                out, taps = cr.LS_Filter_Toeplitz(r, s, L, 10, True)
                e1, e2 = rel_err(out, eo), rel_err(taps, et)
                e3 = rel_err(cr.LS_Filter_Multiple(r, s, L, E.LS_FS, list(E.LS_BINS)), O.LS_Filter_Multiple(r, s, L, E.LS_FS, list(E.LS_BINS)))
                print(f"LS method {method} dropout of {m} in {name}: out {e1:.3g} taps {e2:.3g} chain {e3:.3g}")
                assert e1 < TIGHT and e2 < TIGHT and e3 < TOL, (m, name, e1, e2, e3)
    _with_ls_method(method, go)


@pytest.mark.parametrize("caf", [1, 2, 3], ids=["direct", "fft1024", "fft4096"])
def test_caf_dropouts(caf):
    """dropouts of 40 and 600 samples across the first piece boundary (3796) and the segment boundary (4096) of the
    4096-point kernel, in ref, in srv, in both; the same inputs through the other segment kernels"""
    from passiveradar_amd import range_doppler_processing as rdp
    n, R, F = E.CAF_MULTI
    ref, srv, w, _ = _caf_case(n, R, F, 13)
    rdp.set_default_methods(caf=caf)
    try:
        for m, at in ((40, 3780), (600, 3700)):
            for name, r, s in (("ref", E.hole(ref, at, m), srv), ("srv", ref, E.hole(srv, at, m)),
                               ("both", E.hole(ref, at, m), E.hole(srv, at + 7, m))):
                e = rel_err(rdp.fast_xambg(r, s, R, F, n, w), _caf_dropout_oracle(m, at, name))
                print(f"CAF method {caf} dropout of {m} in {name}: {e:.3g}")
                assert e < TIGHT, (m, name, e)
    finally:
        rdp.set_default_methods(caf=0)


@functools.lru_cache(maxsize=None)
def _caf_dropout_oracle(m, at, name):
    n, R, F = E.CAF_MULTI
    ref, srv, w, _ = _caf_case(n, R, F, 13)
    r = E.hole(ref, at, m) if name in ("ref", "both") else ref
    s = E.hole(srv, at + (7 if name == "both" else 0), m) if name in ("srv", "both") else srv
    return O.fast_xambg(r, s, R, F, n, w)


# ---- constant recordings ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int8", "int16", "uint8", "float32"])
def test_constant_recordings(dtype):
    """a recording stuck at one (I, Q) pair, full scale for the integer types: front end (both kernel forms), the FIR
    decimator behind channel_preprocessing, and the spectra with and without detrending.  A detrended constant has a
    spectrum of rounding errors, so its error is stated against the power of the input (the peak of the spectrum that is
    not detrended), at the same bar.  Without detrending the same holds for the far bins: a float32 transform leaves about
    1e-14 of the peak power in every bin, which moves a bin of 1e-7 of the peak by 2 sqrt(1e-7 1e-14) / 1e-7 = 6e-4, a
    quarter of the 0.01 dB bar; the dB bar is held on the bins above 1e-7 of the peak, the peak-normalised bar on all."""
    from passiveradar_amd import _lib
    from passiveradar_amd.signal_utils import channel_preprocessing, front_end
    from passiveradar_amd.spectral import psd
    up, dn, n_in, nblk = 3, 7, 700, 3
    i, q = E.full_scale(dtype)
    raw = E.constant_raw(dtype, 2 * n_in * nblk, i, q)
    args = (2 * n_in, 100_000, 2_400_000, up, dn)
    exp = O.front_end(raw, *args)
    old = _lib.get_option(_lib.OPT_FE_METHOD)
    try:
        for method in (1, 2):
            _lib.set_option(_lib.OPT_FE_METHOD, method)
            e = rel_err(front_end(raw, *args, max_blocks=2), exp)
            print(f"front_end {dtype} constant, method {method}: {e:.3g}")
            assert e < TIGHT, (method, e)
    finally:
        _lib.set_option(_lib.OPT_FE_METHOD, old)
    e = rel_err(channel_preprocessing(raw, 10, 1e5, FS), PO.channel_preprocessing(raw, 10, 1e5, FS))
    assert e <= BAR, e
    z = PO.deinterleave(raw)
    kw = dict(NFFT=256, Fs=FS, noverlap=37)
    plain = P.psd(z, detrend="none", **kw)
    got, _ = psd(raw, detrend="none", raw=True, **kw)
    held = plain > 1e-7 * plain.max()
    rel, db = float(np.abs(got - plain).max() / plain.max()), float(np.abs(10 * np.log10(got[held] / plain[held])).max())
    print(f"psd {dtype} constant: rel {rel:.3g} dB {db:.3g}")
    assert rel <= REL_BAR and db <= DB_BAR, (rel, db)
    got, _ = psd(raw, detrend="mean", raw=True, **kw)
    rel = float(np.abs(got - P.psd(z, detrend="mean", **kw)).max() / plain.max())
    print(f"psd {dtype} constant, detrended: {rel:.3g} of the input's peak")
    assert np.isfinite(got).all() and rel <= REL_BAR, rel


def test_constant_streams_through_resample_and_the_decimators():
    from passiveradar_amd.signal_utils import decimate, decimate_iir, resample
    from passiveradar_amd.spectral import csd
    for c in (32767 - 32768j, 1e-5 + 3e-5j):                     # int16 full scale as complex64; a float recording's level
        x = np.full(5000, c, np.complex64)
        assert rel_err(resample(x, 3, 7), O.resample(x, 3, 7)) < TIGHT, c
        assert rel_err(decimate_iir(x, 4), O.decimate_iir(x, 4)) < IIR_BAR, c
        for q in (4, 97):
            assert rel_err(decimate(x, q), PO.decimate(x, q)) <= BAR, (c, q)
        y = np.full(5000, c * (0.5 - 0.2j), np.complex64)
        kw = dict(NFFT=256, Fs=FS, noverlap=37)
        plain = P.csd(x, y, detrend="none", **kw)
        got, _ = csd(x, y, detrend="none", **kw)
        assert float(np.abs(got - plain).max() / np.abs(plain).max()) <= REL_BAR, c
        got, _ = csd(x, y, detrend="mean", **kw)
        assert float(np.abs(got - P.csd(x, y, detrend="mean", **kw)).max() / np.abs(plain).max()) <= REL_BAR, c


# ---- CFAR -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absolute", [False, True], ids=["CFAR_2D", "CFAR_2D_abs"])
@pytest.mark.parametrize("method", [0, 1], ids=["separable", "every_tap"])
def test_cfar_zero_frame_and_zero_patch(method, absolute):
    """frame 1 of a stack of three is all zero (the oracle: 0 / 0 everywhere); frame 2 has a zero patch larger than the box
    (inside it the box sum is exactly 0 and the ratio 0 / 1e-10 = 0)"""
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import CFAR_2D, CFAR_2D_abs
    H, W, fw, gw = E.CFAR_H, E.CFAR_W, E.CFAR_FW, E.CFAR_GW
    rng = np.random.default_rng(33064 + method)
    X = (rng.standard_normal((3, H, W)) + 1j * rng.standard_normal((3, H, W))).astype(np.complex64)
    X[2, 5:25, 10:40] = 0
    Z = np.array(X)
    Z[1] = 0

    def run(stack):
        return (host(CFAR_2D_abs(dev(stack), fw, gw)),) if absolute else (host(CFAR_2D(dev(np.abs(stack)), fw, gw)),)

    old = _lib.set_option(_lib.OPT_CFAR_METHOD, method)
    try:
        with np.errstate(all="ignore"):
            exp = O.CFAR_2D(np.abs(Z[1]), fw, gw)
        (frame,) = nonfinite_rule(f"CFAR zero frame, method {method}", run, X, Z, 1, exp, TIGHT)
        got = run(Z)[0]
    finally:
        _lib.set_option(_lib.OPT_CFAR_METHOD, old)
    _recorded(("cfar_zero_frame", method, absolute), frame)
    want = O.CFAR_2D(np.abs(Z[2]), fw, gw)
    assert rel_err(got[2], want) < TIGHT and not got[2][5 + fw:25 - fw, 10 + fw:40 - fw].any()
    assert rel_err(got[0], O.CFAR_2D(np.abs(Z[0]), fw, gw)) < TIGHT


def test_channel_offset_of_two_silent_inputs():
    """an argmax over exact ties: the first index, as NumPy's"""
    from passiveradar_amd.signal_utils import find_channel_offset
    z = np.zeros(4000, np.complex64)
    for nd, nl in ((1, 10), (4, 25)):
        off, xc = find_channel_offset(z, z, nd, nl, return_xc=True)
        assert not xc.any() and off == -nl * nd == O.find_channel_offset(z, z, nd, nl), (nd, nl, off)
