"""signal_utils.channelize and prc_channelize on the MI355X against the float64 definition of tests/channelize_oracle.py.

Accuracy bar: 2e-6 of the peak.  A NumPy float32 emulation of the two kernels' own summation orders (channelize_oracle.
emulate_tile / emulate_direct, run on the CPU before any GPU run, tests/test_channelize_host.py) differs from the definition by at
most 4.4e-7 (tile order, (4100, 100, 50)) and 1.4e-7 (direct order, (600, 8, 74)); 4 x 4.4e-7 = 1.8e-6 (fused multiply-adds, the
rounding of the twiddle table), rounded up to one digit.  The same bar holds at start = 2^40 + 12345.
Measured on the MI355X: tile form at most 4.6e-7 on the zero-mean types (complex64, (4100, 100, 50)) and
1.4e-6 on uint8 at (600, 8, 73) -- uint8 carries a mean of 127.5 that every tap phase's partial sum holds until the DFT over the
phases cancels it; the emulation on that input gives 1.6e-6; the bar was set from the zero-mean inputs and holds --, direct form
at most 1.6e-7, start = 2^40 + 12345 1.5e-7 (tile) and 9.9e-8 (direct).

Against the existing front end, row i is held to channel_preprocessing(raw, D, -k_i Fs / M, Fs) within
4 * 2^-24 * 2 pi |k_i| n / M + bar (k_i folded to [-M/2, M/2]): four float32 roundings of the reference's phase ramp, which
channelize does not have.  The shapes are the smallest at which each thing can go wrong."""
import contextlib

import numpy as np
import pytest

import channelize_oracle as O

pytestmark = pytest.mark.gpu

BAR = O.GPU_BAR
FS = 2.4e6
_want = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_resident(gpu_ready):
    before = O.device_tables()
    yield
    O.release_device_leftovers(before)


def want(label, n, M, D, ch, taps, dtype, start=0):
    """the float64 definition of a case, computed once"""
    key = (label, dtype, start)
    if key not in _want:
        _want[key] = O.channelize(O.case_input(n, M, D, dtype), M, D, ch, taps, start)
        _want[key].setflags(write=False)
    return _want[key]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


class direct_form:
    """PRC_OPT_CHANNELIZE_FORM = 1 for the block: every call runs the direct form"""

    def __enter__(self):
        from passiveradar_amd import _lib
        self.old = _lib.set_option(_lib.OPT_CHANNELIZE_FORM, 1)

    def __exit__(self, *exc):
        from passiveradar_amd import _lib
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, self.old)


@pytest.mark.parametrize("case", O.all_cases(), ids=lambda c: c[0])
def test_accuracy_every_case_and_dtype(gpu_ready, case):
    """the form the library chooses (tile wherever the tile fits), NumPy and device-tensor paths, every raw dtype"""
    from passiveradar_amd.signal_utils import channelize
    label, n, M, D, ch, taps = case
    form = "tile" if O.is_tile(D, 20 * D + 1 if taps is None else len(taps)) else "direct"
    for dtype in O.DTYPES:
        x = O.case_input(n, M, D, dtype)
        w = want(label, n, M, D, ch, taps, dtype)
        got = channelize(x, M, D, ch, taps=taps)
        assert got.shape == w.shape and got.dtype == np.complex64
        err = O.rel_err(got, w)
        print(f"channelize {label} {dtype} ({form}): {err:.3g}")
        assert err <= BAR, (label, dtype, err)
        gd = channelize(dev(x), M, D, ch, taps=taps)
        assert gd.is_cuda and same_bits(gd, got), (label, dtype)


def test_accuracy_direct_form_every_case(gpu_ready):
    from passiveradar_amd.signal_utils import channelize
    worst = 0.0
    with direct_form():
        for label, n, M, D, ch, taps in O.all_cases():
            for dtype in ("int8", "complex64"):
                got = channelize(O.case_input(n, M, D, dtype), M, D, ch, taps=taps)
                err = O.rel_err(got, want(label, n, M, D, ch, taps, dtype))
                worst = max(worst, err)
                assert err <= BAR, (label, dtype, err)
    print(f"direct form, every case: worst {worst:.3g}")


def test_exact_phase_far_into_a_stream(gpu_ready):
    from passiveradar_amd.signal_utils import channelize
    label, (n, M, D, ch) = "2000_12_12", O.CASES[0]
    for dtype in ("int8", "complex64"):
        x = O.case_input(n, M, D, dtype)
        w = want(label, n, M, D, ch, None, dtype, O.FAR_START)
        near = want(label, n, M, D, ch, None, dtype)
        assert O.rel_err(w[1], near[1]) > 0.1                         # another phase than start = 0: the test can fail
        got = channelize(x, M, D, ch, start=O.FAR_START)
        with direct_form():
            got_direct = channelize(x, M, D, ch, start=O.FAR_START)
        print(f"start = 2^40 + 12345, {dtype}: tile {O.rel_err(got, w):.3g}, direct {O.rel_err(got_direct, w):.3g}")
        assert O.rel_err(got, w) <= BAR and O.rel_err(got_direct, w) <= BAR
    # a later block continues the stream: its outputs away from the edges are the whole stream's, bit for bit
    raw = O.case_input(4800, M, D)
    whole = channelize(raw, M, D, ch)
    block = channelize(raw[2 * 1200:], M, D, ch, start=1200)
    assert same_bits(block[:, 11:-11], whole[:, 111:-11])


@pytest.mark.parametrize("case", O.CASES, ids=lambda c: "_".join(map(str, c[:3])))
def test_tie_to_the_existing_front_end(gpu_ready, case):
    from passiveradar_amd.signal_utils import channel_preprocessing, channelize, decimate, deinterleave_IQ
    n, M, D, ch = case
    raw = O.case_input(n, M, D)
    got = channelize(raw, M, D, ch)
    for i, k in enumerate(ch):
        kf = k % M - (M if 2 * (k % M) > M else 0)                    # the same channel, folded to [-M/2, M/2]
        if kf == 0:
            ref, allow = decimate(deinterleave_IQ(raw), D), BAR
        else:
            ref = channel_preprocessing(raw, D, -kf * FS / M, FS)
            allow = 4 * 2.0 ** -24 * 2 * np.pi * abs(kf) * n / M + BAR
        err = O.rel_err(got[i], ref)
        print(f"({n}, {M}, {D}) channel {k}: {err:.3g} of the front end's row, allowance {allow:.3g}")
        assert err <= allow, (case, k, err, allow)


def test_bits_do_not_depend_on_the_request(gpu_ready):
    """two calls; a channel alone, inside any list, in another order, duplicated, as k - M, in every group size of the tile
    kernel (1, 2, 4, 8, a ragged last group) and past the wrapper's 64-row split -- in both forms"""
    from passiveradar_amd.signal_utils import channelize
    n, M, D = 2000, 12, 12
    raw = O.case_input(n, M, D)
    rows = {}
    for form, ctx in (("tile", contextlib.nullcontext()), ("direct", direct_form())):
        with ctx:
            alone = rows[form] = {k: channelize(raw, M, D, [k])[0] for k in range(M)}
            assert same_bits(channelize(raw, M, D, [5])[0], alone[5])
            for req in ([5, 5], [7, 2], [2, 7, 5], [0, 1, -1, 5, 6], [11, 10, 9, 8, 7, 6, 5, 4], list(range(M)), None,
                        [5] * 9, (list(range(M)) * 6)[:70]):
                y = channelize(raw, M, D, req)
                ks = range(M) if req is None else req
                assert y.shape[0] == len(ks)
                for i, k in enumerate(ks):
                    assert same_bits(y[i], alone[k % M]), (form, req, i)
    # the two forms differ in the order of their sums, not in what they compute
    assert O.rel_err(rows["tile"][5], rows["direct"][5]) <= 2 * BAR


def test_device_tensor_is_read_in_place_on_the_current_stream(gpu_ready):
    import torch
    from passiveradar_amd.signal_utils import channelize
    n, M, D, ch = 40000, 12, 10, [1, -3, 6]
    raw = dev(O.case_input(n, M, D))
    w = channelize(raw, M, D, ch)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rs = torch.zeros_like(raw)
        for _ in range(20):                                          # work the launch must wait behind
            rs = rs // 2 + raw // 2
        rs = rs * 0 + raw
        got = channelize(rs, M, D, ch)
    side.synchronize()
    assert got.device == raw.device and tuple(got.shape) == (3, 4000) and same_bits(got, w)
    # a strided view is made contiguous, not over-read; an odd trailing scalar is ignored
    wide = torch.full((2 * n, 2), 127, dtype=torch.int8, device="cuda")
    wide[:, 0] = raw
    assert same_bits(channelize(wide[:, 0], M, D, ch), w)
    assert same_bits(channelize(torch.cat([raw, raw[:1]]), M, D, ch), w)


def _band_noise(rng, n, fs, bw):
    """complex noise of length n at rate fs, flat inside |f| < bw / 2, unit power"""
    spec = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    spec[np.abs(np.fft.fftfreq(n, 1.0 / fs)) > bw / 2] = 0
    z = np.fft.ifft(spec)
    return z / np.sqrt(np.mean(np.abs(z) ** 2))


def test_two_stations_end_to_end(gpu_ready):
    """two band-limited noise stations in channels 2 and -5 of 12, each with an echo delayed by whole output samples and its own
    Doppler over weaker direct signals: channelize both int8 captures once, fast_xambg per station, at the smallest frame of the
    CAF parity tests (2401 samples, 3 range bins, 16 Doppler bins)"""
    from passiveradar_amd import scene
    from passiveradar_amd.range_doppler_processing import fast_xambg
    from passiveradar_amd.signal_utils import channelize
    M = D = 12
    n, R, F = 2401, 3, 16
    fs_out = FS / D
    cpi = n / fs_out
    stations = [(2, 1, 3 / cpi), (-5, 3, -5 / cpi)]                   # (channel, delay in output samples, Doppler in Hz)
    rng = np.random.default_rng(2512)
    m = np.arange(n * D)
    ref = np.zeros(n * D, np.complex128)
    srv = np.zeros(n * D, np.complex128)
    for k, d, f in stations:
        s = _band_noise(rng, n * D, FS, 120e3) * np.exp(2j * np.pi * k * m / M)
        ref += s
        srv += 0.3 * s + np.roll(s, d * D) * np.exp(2j * np.pi * f * m / FS)

    def capture(z):
        z = z * (100.0 / np.abs(np.concatenate([z.real, z.imag])).max())
        return np.round(np.stack([z.real, z.imag], axis=1)).astype(np.int8).reshape(-1)

    chans = [k for k, _, _ in stations]
    yr, ys = channelize(capture(ref), M, D, chans), channelize(capture(srv), M, D, chans)
    cells = [scene.expected_peak_cell(d, f, n, fs_out, R, F) for _, d, f in stations]
    assert cells[0] != cells[1]
    for i, (k, d, f) in enumerate(stations):
        X = np.abs(fast_xambg(yr[i], ys[i], R, F, n)[:, :, 0])
        peak = np.unravel_index(np.argmax(X), X.shape)
        print(f"station in channel {k}: peak at {peak}, expected {cells[i]}, the other station's cell {cells[1 - i]}")
        assert tuple(int(v) for v in peak) == cells[i], (k, peak, cells)
        assert X[cells[1 - i]] < 0.5 * X[cells[i]]
