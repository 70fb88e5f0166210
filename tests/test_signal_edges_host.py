"""What the oracles say off unit amplitude and on dead air (tests/signal_edges.py): the expectations that
tests/test_gpu_signal_edges.py holds the kernels to are themselves under test here, on the CPU.

Every oracle of an entry point without an absolute constant is power-of-two equivariant BIT FOR BIT (so one oracle run at
scale 0, scaled exactly, serves every rung of the ladder); zero results are exact zeros; the first sample that is not finite
after a reference dropout longer than the filter is out[filterLen + start]; an argmax over exact ties returns the first
index.  Small shapes: the properties do not depend on the size."""
import numpy as np
import pytest

import preproc_oracle as PO
import psd_oracle as P
import signal_edges as E
from gal_oracle import gal_jpe
from ls_svd_oracle import ls_filter_svd
from oracle import c_oracle
from oracle import np_oracle as O

N = 4096
W = np.kaiser(N, 5.0)
FS = 2.4e6

# name -> (oracle of (ref, srv), (degree in ref, degree in srv) per returned array)
EQUIVARIANT = {
    "fast_xambg": (lambda r, s: O.fast_xambg(r, s, 20, 64, N, W), [(1, 1)]),
    "fast_xambg_c_twin": (lambda r, s: c_oracle.fast_xambg(r, s, 20, 64, W), [(1, 1)]),
    "xcorr": (lambda r, s: O.xcorr(r, s, 7, 20), [(1, 1)]),
    "psd": (lambda r, s: P.psd(r, NFFT=256, Fs=FS, detrend="none", noverlap=37), [(2, 0)]),
    "psd_detrended": (lambda r, s: P.psd(r, NFFT=256, Fs=FS, detrend="mean", noverlap=37), [(2, 0)]),
    "csd": (lambda r, s: P.csd(r, s, NFFT=256, Fs=FS, detrend="mean", noverlap=37), [(1, 1)]),
    "LS_Filter_Toeplitz": (lambda r, s: O.LS_Filter_Toeplitz(r, s, 32, 10, True), [(0, 1), (-1, 1)]),
    "LS_Filter_Multiple": (lambda r, s: O.LS_Filter_Multiple(r, s, 32, 1e4, [0, 1, -1]), [(0, 1)]),
    "NLMS_c_twin": (lambda r, s: c_oracle.nlms(r[:1500], s[:1500], 24, 0.05, 10), [(0, 1), (-1, 1)]),
    "NLMS_numpy": (lambda r, s: O.NLMS_filter(r[:300], s[:300], 24, 0.05, 10, None, True), [(0, 1), (-1, 1)]),
    "frequency_shift": (lambda r, s: O.frequency_shift(r, 37.5, 1e4, 0.3), [(1, 0)]),
    "resample": (lambda r, s: O.resample(r, 3, 7), [(1, 0)]),
    "decimate_iir": (lambda r, s: O.decimate_iir(r, 4), [(1, 0)]),
    "fir_decimate": (lambda r, s: PO.decimate(r, 4), [(1, 0)]),
    "normalize": (lambda r, s: PO.normalize(r), [(0, 0)]),
}


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


@pytest.mark.parametrize("name", list(EQUIVARIANT))
def test_oracle_is_power_of_two_equivariant(name):
    fn, degrees = EQUIVARIANT[name]
    ref, srv = E.pair(N, 1)
    base = _tuple(fn(ref, srv))
    assert len(base) == len(degrees)
    for (da, db), out in zip(degrees, base):
        E.budget(out, da, db)
    for a, b in E.LADDER:
        got = _tuple(fn(E.scaled(ref, a), E.scaled(srv, b)))
        for i, ((da, db), out) in enumerate(zip(degrees, base)):
            assert not E.diff_report(got[i], E.expected(out, da, db, a, b)), (name, a, b, i)


def test_the_issue_example_of_the_caf():
    ref, srv = E.pair(N, 1)
    assert E.same_bits(O.fast_xambg(E.scaled(ref, 10), E.scaled(srv, -7), 20, 64), E.scaled(O.fast_xambg(ref, srv, 20, 64), 3))


def test_warm_started_nlms_scales_its_taps_by_srv_over_ref():
    ref, srv = E.pair(N, 1)
    ref, srv = ref[:1500], srv[:1500]
    _, taps = c_oracle.nlms(ref, srv, 24, 0.05, 10)
    out0, t0 = c_oracle.nlms(ref, srv, 24, 0.02, 10, taps)
    for a, b in E.LADDER:
        out, t = c_oracle.nlms(E.scaled(ref, a), E.scaled(srv, b), 24, 0.02, 10, E.scaled(taps, b - a))
        assert E.same_bits(out, E.scaled(out0, b)) and E.same_bits(t, E.scaled(t0, b - a)), (a, b)


def test_raw_front_ends_are_equivariant_on_float32_recordings():
    raw = E.raw_float32(2 * 700 * 3, 5)
    fe = O.front_end(raw, 1400, 100000, 2400000, 3, 7)
    cp = PO.channel_preprocessing(raw, 10, 1e5, FS)
    E.budget(fe, 1, 0)
    for a, _ in E.LADDER:
        assert E.same_bits(O.front_end(E.scaled(raw, a), 1400, 100000, 2400000, 3, 7), E.scaled(fe, a)), a
        assert E.same_bits(PO.channel_preprocessing(E.scaled(raw, a), 10, 1e5, FS), E.scaled(cp, a)), a


def test_helpers_notice_what_they_are_for():
    x = E.white(64, 2)
    assert E.same_bits(E.scaled(x, -24), x * np.float32(2.0 ** -24)) and not E.same_bits(x, x + np.float32(1e-7) * x)
    assert not E.same_bits(np.zeros(3, np.float32), -np.zeros(3, np.float32))          # bits, not values
    assert E.diff_report(x, x) == "" and "1 of 64" in E.diff_report(E.hole(x, 5, 1), x)
    with pytest.raises(AssertionError):
        E.scaled(x, -140)                                                                # subnormal: not exact
    with pytest.raises(AssertionError):
        E.budget(np.ones(4), 2, 2, ladder=((30, 30),))
    assert E.first_nonfinite(np.array([0.0, 1.0, np.nan, 2.0, np.inf])) == 2 and E.first_nonfinite(x) is None
    h = E.hole(x, 10, 7)
    assert not h[10:17].any() and h[:10].all() and h[17:].all() and x[10:17].all()
    for dt in ("int8", "int16", "uint8", "float32"):
        i, q = E.full_scale(dt)
        raw = E.constant_raw(dt, 10, i, q)
        assert raw.dtype == np.dtype(dt) and (raw[0::2] == i).all() and (raw[1::2] == q).all()


# ---- dead air ---------------------------------------------------------------------------------------------------------------
def test_silent_surveillance_gives_exact_zeros():
    ref, _ = E.pair(2000, 3)
    z = E.silent(2000)
    out, taps = O.LS_Filter_Toeplitz(ref, z, 32, 10, True)
    assert not out.any() and not taps.any()
    assert not O.LS_Filter_Multiple(ref, z, 32, 1e4, [0, 1, -1]).any()
    out, taps = O.LS_Filter(ref, z, 32, 1.0, 10, True)
    assert not out.any() and not taps.any()
    for out, taps in (c_oracle.nlms(ref, z, 24, 0.05, 10), O.NLMS_filter(ref[:300], z[:300], 24, 0.05, 10, None, True)):
        assert not out.any() and not taps.any()
    out, k, h = gal_jpe(ref[:700], z[:700], 8, 64, 2e-3, 2e-2, 10, np.complex64, True)
    assert not out.any() and not h.any() and k.any()          # the lattice still adapts to the reference; nothing is cancelled
    out, taps = ls_filter_svd(ref[:1021], z[:1021], 17, 10, 0.0)
    assert not out.any() and not taps.any()
    assert not O.fast_xambg(ref, z, 20, 50).any() and not O.xcorr(ref, z, 3, 9).any()


def test_silent_reference():
    _, srv = E.pair(2000, 3)
    z = E.silent(2000)
    assert not O.fast_xambg(z, srv, 20, 50).any()
    assert E.same_bits(O.LS_Filter(z, srv, 32, 1.0), srv)                       # reg = 1 alone on the diagonal: taps 0
    with np.errstate(all="ignore"):
        out, taps = O.LS_Filter_Toeplitz(z, srv, 32, 10, True)                   # 1 / c[0] = 1 / 0
        assert np.isnan(out).all() and np.isnan(taps).all()
        assert np.isnan(O.LS_Filter_Multiple(z, srv, 32, 1e4, [0, 1, -1])).all()
        for out, taps in (c_oracle.nlms(z, srv, 24, 0.05, 10), O.NLMS_filter(z[:300], srv[:300], 24, 0.05, 10, None, True)):
            # the first step's error still uses the zero taps; its update is 0 / 0
            assert E.first_nonfinite(out) == 24 + 1 and out[24] == srv[24] and not np.isfinite(taps).any()
    # the guarded divisions: GAL and the SVD cut keep everything finite and cancel nothing
    out, k, h = gal_jpe(z[:700], srv[:700], 8, 64, 2e-3, 2e-2, 10, np.complex64, True)
    assert E.same_bits(out[:700 - 11], srv[:700 - 11]) and not out[700 - 11:].any() and not k.any() and not h.any()
    out, taps = ls_filter_svd(z[:1021], srv[:1021], 17, 10, 0.0)
    assert E.same_bits(out.astype(np.complex64), srv[:1021]) and not taps.any()


@pytest.mark.parametrize("L,start", [(16, 200), (24, 700)])
def test_nlms_dropout_longer_than_the_filter(L, start):
    """ref[start:start + m] = 0: finite everywhere with m < T; with m > T finite through out[L + start - 1], not from
    out[L + start] on, and never again (NaN taps stay NaN) -- NumPy oracle and C twin alike"""
    ref, srv = E.pair(1500, 4)
    T = L + 10
    short = E.hole(ref, start, T - 6)
    long = E.hole(ref, start, T + 14)
    with np.errstate(all="ignore"):
        for run in (lambda r: c_oracle.nlms(r, srv, L, 0.05, 10), lambda r: O.NLMS_filter(r, srv, L, 0.05, 10, None, True)):
            out, taps = run(short)
            assert np.isfinite(out).all() and np.isfinite(taps).all()
            out, taps = run(long)
            first = E.nlms_first_nonfinite(L, start)
            assert E.first_nonfinite(out) == first and np.isfinite(out[:first]).all()
            assert not np.isfinite(out[first:1500 - 10]).any() and not out[1500 - 10:].any() and not np.isfinite(taps).any()
    # a dropout of srv, of any length, is an ordinary input
    out, taps = c_oracle.nlms(ref, E.hole(srv, start, T + 14), L, 0.05, 10)
    assert np.isfinite(out).all() and np.isfinite(taps).all()


def test_ls_and_caf_ride_through_dropouts():
    ref, srv = E.pair(2000, 3)
    for m in (20, 60):                           # T = 42: shorter and longer
        for r, s in ((E.hole(ref, 500, m), srv), (ref, E.hole(srv, 500, m)), (E.hole(ref, 500, m), E.hole(srv, 500, m))):
            out, taps = O.LS_Filter_Toeplitz(r, s, 32, 10, True)
            assert np.isfinite(out).all() and np.isfinite(taps).all()
            assert np.isfinite(O.fast_xambg(r, s, 20, 50)).all()


def test_cfar_of_zeros_and_of_a_zero_patch():
    with np.errstate(all="ignore"):
        assert np.isnan(O.CFAR_2D(np.zeros((E.CFAR_H, E.CFAR_W), np.float32), E.CFAR_FW, E.CFAR_GW)).all()     # 0 / 0
    rng = np.random.default_rng(8)
    X = np.abs(rng.standard_normal((E.CFAR_H, E.CFAR_W))).astype(np.float32)
    X[5:25, 10:40] = 0                           # larger than the 7 x 7 box: inside, the box sum is exactly 0
    cr = O.CFAR_2D(X, E.CFAR_FW, E.CFAR_GW)
    assert np.isfinite(cr).all() and not cr[5:25, 10:40].any() and cr[0, 0] > 0


def test_argmax_over_exact_ties_is_the_first_index():
    z = np.zeros(4000, np.complex64)
    for nd, nl in ((1, 10), (4, 25)):
        off, xc = O.find_channel_offset(z, z, nd, nl, return_xc=True)
        assert not xc.any() and off == -nl * nd
    assert O.find_channel_offset(z, z, 1, 10) == -10
