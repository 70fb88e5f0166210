"""Whole-recording lengths: the entry points of include/prcore.h that are meant for a recording in one call, on streams of
N64 = 2^29 + 4099 complex64 samples (byte 2^31 falls at sample 2^28, byte 2^32 at sample 2^29) and N8 = 2^31 + 4099 int8 I/Q
samples (byte 2^31 at sample 2^30, byte 2^32 at sample 2^31).  DESIGN.md, "64-bit sizes", has the audit these cases follow and
their measured times and memory.

The inputs are built on the device and never exist on the host: x[i] = base[i mod P], P = 1 000 003, base a seeded host array.
The oracle then produces any window, and any exact whole-stream sum, from base alone in float64.  Outputs of local support
are compared with the entry point's own oracle, evaluated on absolute sample indices with the history it needs, at the entry
point's existing bar, over windows of 4096 outputs: the first one, those centred on every input and output index at which a
byte offset of an argument crosses 2^31 or 2^32, and the last one with the final ragged output.  An addressing error is
structured -- zeros, shifted data, a break at a power of two -- and lands in one of these windows.  Exact operations
(prc_deinterleave, prc_shift, prc_persistence, prc_display_rgba) are compared in full, on the device, with torch.

Every case says what it allocates before it does, skips below that plus 8 GiB of free device memory (none skips on an idle
MI355X) and leaves the device memory as it found it."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import preproc_oracle as PO
from passiveradar_amd import _lib

pytestmark = pytest.mark.gpu

GiB = 1 << 30
P = 1_000_003
N64 = 2 ** 29 + 4099
N8 = 2 ** 31 + 4099
WIN = 4096


@pytest.fixture(autouse=True)
def _clean(gpu_ready, request):
    """a HIP fault is sticky: if an earlier case left one, nothing more is started on the device (tests/test_gpu_bounds.py)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports a fault from an earlier case, stopping: {e}", returncode=3)
    torch.cuda.reset_peak_memory_stats()
    try:
        yield
    finally:
        print(f"\n[{request.node.name}: peak {torch.cuda.max_memory_allocated() / GiB:.1f} GiB of tensors]")
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def need(gib):
    """skip unless ``gib`` GiB (what the case allocates at its peak) plus 8 GiB are free"""
    assert gib <= 40
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < (gib + 8) * GiB:
        pytest.skip(f"needs {gib} GiB + 8 GiB of device memory, {free / GiB:.1f} GiB are free")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def base_c64(seed):
    """complex white noise scaled to a peak magnitude of 1: an absolute bar set at unit scale holds as it stands"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    return (z / np.abs(z).max()).astype(np.complex64)


def base_i8(seed):
    """P int8 I/Q pairs, [P, 2]"""
    return np.random.default_rng(seed).integers(-128, 128, (P, 2), dtype=np.int8)


def periodic(base, n):
    """device x[i] = base[i mod P], i < n (rows of base for a 2-D base); at most P elements more than n are allocated"""
    b = dev(base)
    reps = -(-n // P)
    return b.repeat((reps,) + (1,) * (b.dim() - 1))[:n]


def at(base, lo, hi):
    """host x[lo:hi] of the periodic stream"""
    return base[np.arange(lo, hi) % P]


def windows(n, crossings):
    """[lo, hi) runs of WIN indices below n: the first, one centred on every crossing inside the stream, the last"""
    out = [(0, min(WIN, n))]
    for c in crossings:
        if 0 < c < n:
            lo = max(0, min(c - WIN // 2, n - WIN))
            out.append((lo, min(lo + WIN, n)))
    out.append((max(0, n - WIN), n))
    return sorted(set(out))


def peak_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- frequency_shift: the float32 ramp of the reference is part of the oracle -----------------------------------------------
FS, FC = 2.4e5, 37500.5


def ramp32(lo, hi):
    """ph[i] = fl32(fl32(fl32(2 pi fc) fl32(i)) fl32(1 / fl32(fs))) on absolute indices: fl32(i) is not i up there"""
    i = np.arange(lo, hi).astype(np.float32)
    return (np.float32(2 * np.pi * FC) * i) * (np.float32(1.0) / np.float32(FS))


@pytest.mark.parametrize("form", ["shift", "block", "phases64", "phases32"])
def test_frequency_shift(form):
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    wide = form in ("block", "phases64")
    need(4 + (8 if wide else 4) + {"phases64": 4, "phases32": 2}.get(form, 0) + 1)
    base = base_c64(101)
    x = periodic(base, N64)
    y = torch.full((N64,), float("nan"), dtype=torch.complex128 if wide else torch.complex64, device="cuda")
    pbase = np.random.default_rng(102).uniform(-3, 3, P)
    if form == "shift":
        _lib.check(lib.prc_frequency_shift(x.data_ptr(), y.data_ptr(), N64, FC, FS, 0.3, st))
    elif form == "block":
        _lib.check(lib.prc_frequency_shift_block(x.data_ptr(), y.data_ptr(), N64, FC, FS, 0.3, st))
    else:
        pbase = pbase.astype(np.float32) if form == "phases32" else pbase
        ph = periodic(pbase, N64)
        _lib.check(lib.prc_frequency_shift_phases(x.data_ptr(), y.data_ptr(), N64, FC, FS, ph.data_ptr(), int(form == "phases32"), st))
    torch.cuda.synchronize()
    worst = 0.0
    # byte 2^31 / 2^32 of x and float64 phases (8 per sample): 2^28 / 2^29; of a complex128 y (16): 2^27 / 2^28; of float32
    # phases (4): 2^29 / beyond the end
    for lo, hi in windows(N64, [2 ** 27, 2 ** 28, 2 ** 29]):
        xs = at(base, lo, hi).astype(np.complex128)
        ph = ramp32(lo, hi)
        if form == "shift":
            ph = (ph + np.float32(0.3)).astype(np.float64)
        elif form == "block":
            ph = ph.astype(np.float64) + 0.3
        elif form == "phases64":
            ph = ph.astype(np.float64) + at(pbase, lo, hi)
        else:
            ph = (ph + at(pbase, lo, hi)).astype(np.float64)
        want = xs * np.exp(1j * ph)
        worst = max(worst, float(np.abs(y[lo:hi].cpu().numpy() - want).max()))
    print(f"prc_frequency_shift {form}: worst absolute error on the windows {worst:.3g}")
    assert worst < 2e-6                                               # tests/test_gpu_bounds.py, test_frequency_shift


# ---- deinterleave and shift: exact, compared in full on the device ---------------------------------------------------------
def test_deinterleave_int8():
    need(4.1 + 16.1 + 2)          # raw, out, and one 2^26-sample piece of the comparison
    base = base_i8(103)
    raw = periodic(base, N8)
    out = torch.full((N8,), float("nan"), dtype=torch.complex64, device="cuda")
    _lib.check(_lib.lib().prc_deinterleave(raw.data_ptr(), _lib.RAW_DTYPES["int8"], N8, out.data_ptr(), _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    got = torch.view_as_real(out)
    step = 2 ** 26
    for lo in range(0, N8, step):
        assert torch.equal(got[lo:lo + step], raw[lo:lo + step].to(torch.float32)), lo


def test_deinterleave_float32():
    need(3 * N64 * 8 / GiB + 1)      # raw, out, and the repeat that raw is cut from
    base = np.random.default_rng(104).standard_normal((P, 2)).astype(np.float32)
    raw = periodic(base, N64)
    out = torch.full((N64,), float("nan"), dtype=torch.complex64, device="cuda")
    _lib.check(_lib.lib().prc_deinterleave(raw.data_ptr(), _lib.RAW_DTYPES["float32"], N64, out.data_ptr(), _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(out), raw)


@pytest.mark.parametrize("k", [5, -5])
def test_shift(k):
    rows, width = 2 ** 20 + 3, 4099
    need(3 * rows * width / GiB + 1)      # x, y, and the masks of the comparison
    x = periodic(np.random.default_rng(105).integers(0, 256, P, dtype=np.uint8), rows * width).view(rows, width)
    y = torch.full((rows, width), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().prc_shift(x.data_ptr(), y.data_ptr(), rows, width, k, _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    if k > 0:
        assert torch.equal(y[k:], x[:rows - k]) and not bool(y[:k].any())
    else:
        assert torch.equal(y[:rows + k], x[-k:]) and not bool(y[rows + k:].any())


# ---- fir_decimate ----------------------------------------------------------------------------------------------------------
FD_FC, FD_FS = 1e5, 2.4e6


def firdec_oracle(xt_at, n, q, ntaps, taps, lo, hi):
    """outputs [lo, hi) of prc_fir_decimate in float64: y[j] = sum_k h[k] xt[j q + half - k], xt zero outside [0, n);
    ``xt_at(a, b)`` gives the converted (and tuned) samples [a, b) inside the stream"""
    half = (ntaps - 1) // 2
    a, b = lo * q + half - (ntaps - 1), (hi - 1) * q + half + 1
    xt = np.zeros(b - a, np.complex128)
    ia, ib = max(a, 0), min(b, n)
    xt[ia - a:ib - a] = xt_at(ia, ib)
    h = taps.astype(np.float64)
    y = np.zeros(hi - lo, np.complex128)
    for k in range(ntaps):
        # sample j q + half - k sits at index (j - lo) q + (ntaps - 1) - k of xt
        y += h[k] * xt[ntaps - 1 - k:ntaps - 1 - k + (hi - lo - 1) * q + 1:q]
    return y


def test_fir_decimate_int8_tile_and_out_step():
    """channel_preprocessing of a 2^31-sample int8 recording in one launch (q = 10, 201 taps, the tile form); then the same
    with out_step = 3, whose last output lies beyond 2^32 bytes: bit for bit the dense outputs, nothing between them"""
    q, ntaps = 10, 201
    m = PO.out_len(N8, q)
    need(4.1 + 1.7 + 4.9 + 2)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = base_i8(106)
    raw = periodic(base, N8)
    taps = PO.taps32(q)
    dtaps = dev(taps)
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix, d.fc, d.fs = q, ntaps, _lib.RAW_DTYPES["int8"], 1, FD_FC, FD_FS
    out = torch.full((m,), float("nan"), dtype=torch.complex64, device="cuda")
    _lib.check(lib.prc_fir_decimate(C.byref(d), dtaps.data_ptr(), raw.data_ptr(), N8, 1, 0, 1, out.data_ptr(), 1, 0, st))
    torch.cuda.synchronize()

    def tuned(a, b):
        z = at(base, a, b).astype(np.float32)
        return ((z[:, 0] + 1j * z[:, 1]).astype(np.complex64) * PO.rotation(b - a, FD_FC, FD_FS, a)).astype(np.complex64)
    worst = 0.0
    # input bytes: 2 per sample; output bytes: 8 per output (1.7 GB: no crossing), 24 per output at out_step = 3
    for lo, hi in windows(m, [2 ** 30 // q, 2 ** 31 // q, 2 ** 31 // 24, 2 ** 32 // 24]):
        worst = max(worst, peak_err(out[lo:hi].cpu().numpy(), firdec_oracle(tuned, N8, q, ntaps, taps, lo, hi)))
    print(f"prc_fir_decimate int8 N8 q = 10: worst window error {worst:.3g}")
    assert worst <= 4e-6                                              # tests/test_gpu_preproc.py: BAR
    assert 8 * 3 * (m - 1) > 2 ** 32
    wide = torch.zeros((m, 3), dtype=torch.complex64, device="cuda")
    _lib.check(lib.prc_fir_decimate(C.byref(d), dtaps.data_ptr(), raw.data_ptr(), N8, 1, 0, 1, wide.data_ptr(), 3, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(wide[:, 0]), torch.view_as_real(out))
    assert not bool(torch.view_as_real(wide[:, 1:]).any())


def test_fir_decimate_c64_direct():
    q = PO.TILE_MAX_Q + 1
    ntaps = 20 * q + 1
    m = PO.out_len(N64, q)
    need(4.1 + 1)
    base = base_c64(107)
    x = periodic(base, N64)
    taps = PO.taps32(q)
    dtaps = dev(taps)
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix = q, ntaps, _lib.RAW_DTYPES["complex64"], 0
    out = torch.full((m,), float("nan"), dtype=torch.complex64, device="cuda")
    _lib.check(_lib.lib().prc_fir_decimate(C.byref(d), dtaps.data_ptr(), x.data_ptr(), N64, 1, 0, 1, out.data_ptr(), 1, 0,
                                           _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    worst = 0.0
    for lo, hi in windows(m, [2 ** 28 // q, 2 ** 29 // q]):
        want = firdec_oracle(lambda a, b: at(base, a, b), N64, q, ntaps, taps, lo, hi)
        worst = max(worst, peak_err(out[lo:hi].cpu().numpy(), want))
    print(f"prc_fir_decimate complex64 N64 q = {q}: worst window error {worst:.3g}")
    assert worst <= 4e-6


# ---- channelize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tile", "direct"])
def test_channelize_int8(form):
    import channelize_oracle as O
    M, D, CH, start = 12, 10, [5, -1], 2 ** 40 + 7
    L = 20 * D + 1
    m = O.out_len(N8, D)
    need(4.1 + 3.3 + 1)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = base_i8(108)
    raw = periodic(base, N8)
    cs, sn = O.twiddles32(M)
    tw = dev((cs + 1j * sn).astype(np.complex64))
    taps, ch = dev(O.taps32(D)), dev(np.array(CH, np.int32))
    d = _lib.ChannelizeDesc()
    d.nchan, d.dec, d.ntaps, d.raw_dtype, d.nsel, d.start = M, D, L, _lib.RAW_DTYPES["int8"], len(CH), start
    out = torch.full((len(CH), m), float("nan"), dtype=torch.complex64, device="cuda")
    old = _lib.set_option(_lib.OPT_CHANNELIZE_FORM, int(form == "direct"))
    try:
        _lib.check(lib.prc_channelize(C.byref(d), taps.data_ptr(), tw.data_ptr(), ch.data_ptr(), raw.data_ptr(), N8, out.data_ptr(),
                                      m, st))
        torch.cuda.synchronize()
    finally:
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, old)
    edge = 11                                                         # c / D = 10 outputs either side see a block's edge
    worst = 0.0
    # input bytes: 2 per sample; out bytes: 8 per output, row 1 begins at byte 8 m = 1.7e9 and crosses 2^31 at output 2^28 - m
    for lo, hi in windows(m, [2 ** 30 // D, 2 ** 31 // D, 2 ** 28 - m]):
        j0, j1 = max(lo - edge, 0), min(hi + edge, m)
        s0, s1 = j0 * D, min(j1 * D, N8)
        blk = O.channelize(at(base, s0, s1).reshape(-1), M, D, CH, start=start + s0)       # outputs j0 .. of the stream
        a = edge if j0 else 0
        b = blk.shape[1] - (edge if s1 < N8 else 0)
        want = blk[:, a:b]
        got = out[:, j0 + a:j0 + b].cpu().numpy()
        worst = max(worst, O.rel_err(got, want))
        assert j0 + a <= lo and j0 + b >= hi
    print(f"prc_channelize int8 N8 ({form}): worst window error {worst:.3g}")
    assert worst <= O.GPU_BAR


# ---- welch as a specgram: every row has local support ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex64", "int8"])
def test_welch_specgram(dtype):
    import psd_oracle as W
    nfft, navg = 1024, 4
    step = 1 if dtype == "complex64" else 2
    # int8 at step 2: N8 pairs end 2050 channel samples past byte 2^32, less than one row of 4096: 8192 pairs more, so
    # that the last row lies wholly beyond it
    total = N64 if dtype == "complex64" else N8 + 8192
    n = -(-total // step)                                            # samples of the channel: element i * step
    per_row = nfft * navg
    rows = n // nfft // navg
    need(2 * total * (8 if dtype == "complex64" else 2) / GiB + rows * nfft * 8 / GiB + 2)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = base_c64(109) if dtype == "complex64" else base_i8(109)
    x = periodic(base, total)
    w = np.hanning(nfft)
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.step, d.scale = nfft, 0, navg, 1, step, W.scale(w, 2.4e6)
    d.in_dtype = _lib.RAW_DTYPES[dtype]
    got_seg, got_rows, ws = C.c_int64(0), C.c_int64(0), C.c_size_t(0)
    _lib.check(lib.prc_welch_rows(C.byref(d), n, C.byref(got_seg), C.byref(got_rows)))
    assert got_rows.value == rows
    _lib.check(lib.prc_welch_workspace_bytes(C.byref(d), n, 1, C.byref(ws)))
    work = torch.empty(ws.value, dtype=torch.uint8, device="cuda")
    win = dev(w.astype(np.float32))
    out = torch.full((rows, nfft), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.prc_welch(C.byref(d), x.data_ptr(), None, n, 0, 1, win.data_ptr(), out.data_ptr(), work.data_ptr(), st))
    torch.cuda.synchronize()
    bytes_per = 8 * step if dtype == "complex64" else 2 * step       # input bytes per sample of the channel
    crossings = [2 ** 31 // bytes_per // per_row, 2 ** 32 // bytes_per // per_row, 2 ** 31 // (8 * nfft), 2 ** 32 // (8 * nfft)]
    worst = 0.0
    # 4 rows of 1024 bins are 4096 outputs: the first four, four around every crossing, the last four
    for lo in sorted({0, rows - 4} | {max(0, min(c - 2, rows - 4)) for c in crossings if 0 < c < rows}):
        hi = lo + 4
        if lo == rows - 4:
            assert (hi * per_row - 1) * step * (bytes_per // step) >= 2 ** 32      # the last row is read beyond byte 2^32
        z = at(base, lo * per_row * step, (hi * per_row - 1) * step + 1)[::step]
        if dtype == "int8":
            z = (z[:, 0].astype(np.float32) + 1j * z[:, 1].astype(np.float32)).astype(np.complex64)
        want = W.welch(z, None, NFFT=nfft, Fs=2.4e6, detrend="mean", noverlap=0, navg=navg)
        worst = max(worst, peak_err(out[lo:hi].cpu().numpy(), want))
    print(f"prc_welch {dtype} specgram: worst window error {worst:.3g}")
    assert worst <= 2e-6                                              # tests/test_gpu_psd.py: REL_BAR


# ---- normalize and xcorr: whole-stream sums from the period sums in float64 -------------------------------------------------
def test_normalize():
    need(4.1 + 4.1)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = base_c64(110)
    x = periodic(base, N64)
    y = torch.full((N64,), float("nan"), dtype=torch.complex64, device="cuda")
    ws = C.c_size_t(0)
    _lib.check(lib.prc_normalize_workspace_bytes(N64, C.byref(ws)))
    work = torch.full((ws.value // 8,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.prc_normalize(x.data_ptr(), y.data_ptr(), N64, 1, work.data_ptr(), st))
    torch.cuda.synchronize()
    mag = np.hypot(base.real, base.imag).astype(np.float32).astype(np.float64)       # hypotf, then summed in float64
    q, r = divmod(N64, P)
    mean = np.float32((q * mag.sum() + mag[:r].sum()) / N64)
    worst = 0.0
    for lo, hi in windows(N64, [2 ** 28, 2 ** 29]):
        want = at(base, lo, hi).astype(np.complex128) / np.float64(mean)
        worst = max(worst, peak_err(y[lo:hi].cpu().numpy(), want))
    print(f"prc_normalize N64: mean {mean!r}, worst window error {worst:.3g}")
    assert worst <= 2e-6                                              # tests/test_gpu_preproc.py: NORM_BAR


def test_xcorr():
    nlead = nlag = 8
    need(4.1 + 4.1 + 1)
    b1, b2 = base_c64(111), base_c64(112)
    b2 = (0.5 * b1 + 0.5 * np.roll(b2, 3)).astype(np.complex64)        # correlated: the lags are not all noise
    s1, s2 = periodic(b1, N64), periodic(b2, N64)
    out = torch.full((nlead + nlag + 1,), float("nan"), dtype=torch.complex64, device="cuda")
    _lib.check(_lib.lib().prc_xcorr(s1.data_ptr(), s2.data_ptr(), N64, nlead, nlag, out.data_ptr(), _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    want = np.zeros(nlead + nlag + 1, np.complex128)
    z1, z2 = b1.astype(np.complex128), b2.astype(np.complex128)
    for i in range(nlead + nlag + 1):
        dlag = i - nlead                                             # z[i] = sum_n s1[n] conj(s2[n - dlag]), both inside [0, N64)
        prod = z1 * np.conj(np.roll(z2, dlag))                       # p[m] = b1[m] conj(b2[(m - dlag) mod P]), period P
        cum = np.concatenate([[0], np.cumsum(prod)])

        def upto(t):                                                 # sum of p[n mod P] for n < t
            qq, rr = divmod(t, P)
            return qq * cum[P] + cum[rr]
        want[i] = upto(min(N64, N64 + dlag)) - upto(max(0, dlag))
    err = peak_err(out.cpu().numpy(), want)
    print(f"prc_xcorr N64: {err:.3g}")
    assert err < 2e-5                                                 # tests/test_gpu_bounds.py: TIGHT


# ---- the zero-phase IIR decimator and the channel offset: two spectral passes over a 2^30-point transform ---------------------
IIR_Q = 3


def test_decimate_iir():
    """windows of prc_decimate_iir at N64 against sosfiltfilt of the same samples with padlen + settle samples of history on
    either side (the recursion's memory is below 1e-9 there), at the bar of the entry point's bounds test"""
    from oracle import np_oracle as O
    from passiveradar_amd import engine
    dec = engine.IirDecimator(IIR_Q)
    m = dec.out_len(N64)
    M = 2 ** 30                                                       # next_pow2(N64 + 2 padlen + 2 settle)
    assert N64 + 2 * dec.padlen + 2 * dec.settle <= M
    need((N64 * 8 + m * 8 + 2 * M * 8) / GiB + 1)                   # x, y, the transform in place and rocFFT's work buffer
    base = base_c64(115)
    x = periodic(base, N64)
    y = torch.full((m,), float("nan"), dtype=torch.complex64, device="cuda")
    dec.decimate(x, N64, y, _lib.torch_stream_ptr())
    torch.cuda.synchronize()
    hist = -(-(dec.padlen + dec.settle) // IIR_Q) * IIR_Q             # a multiple of q: the decimation phase is kept
    worst = 0.0
    # bytes of x: 8 per sample; the transform buffer holds sample i at element settle + padlen + i, 8 bytes each
    for lo, hi in windows(m, [2 ** 28 // IIR_Q, 2 ** 29 // IIR_Q]):
        a, b = max(lo * IIR_Q - hist, 0), min(hi * IIR_Q + hist, N64)
        want = O.decimate_iir(at(base, a, b), IIR_Q)[lo - a // IIR_Q:hi - a // IIR_Q]
        worst = max(worst, peak_err(y[lo:hi].cpu().numpy(), want))
    print(f"prc_decimate_iir N64 q = {IIR_Q}: worst window error {worst:.3g}")
    assert worst < 5e-6                                               # tests/test_gpu_bounds.py, test_decimate_and_channel_offset


def test_channel_offset():
    """s2 is s1 delayed by 333 samples (a multiple of q): the offset is -333 as in the bounds test, and the peak of xc is the
    energy of decimate(s1) up to the 111 outputs that leave the overlap, at the bounds test's bar for xc"""
    from passiveradar_amd import engine
    dec = engine.IirDecimator(IIR_Q)
    m, nl, delay = dec.out_len(N64), 200, 333
    M, Mc = 2 ** 30, 2 ** 28
    assert m + 2 * nl <= Mc
    need((2 * N64 * 8 + m * 8 + 2 * M * 8 + 3 * Mc * 8) / GiB + 1)   # s1, s2, y, the transform and its work, A, B and theirs
    base = base_c64(116)
    st = _lib.torch_stream_ptr()
    s1 = periodic(base, N64)
    y = torch.empty((m,), dtype=torch.complex64, device="cuda")
    dec.decimate(s1, N64, y, st)
    torch.cuda.synchronize()
    mag = y.abs().to(torch.float64) ** 2
    energy = float(mag.sum())
    edge = float(mag[:delay // IIR_Q + 64].sum() + mag[-(delay // IIR_Q + 64):].sum())       # what the delay moves out of the overlap
    del y, mag
    torch.cuda.empty_cache()
    s2 = periodic(np.roll(base, delay), N64)                          # s2[i] = s1[i - 333]
    n_xc = dec.n_lags(N64, N64, nl)
    xc = torch.full((n_xc,), float("nan"), dtype=torch.float32, device="cuda")
    am, k = dec.channel_offset(s1, N64, s2, N64, nl, xc, st)
    torch.cuda.synchronize()
    xc = xc.cpu().numpy().astype(np.float64)
    assert k == n_xc == 2 * nl + 1 and ((am - nl) * IIR_Q, int(np.argmax(xc))) == (-delay, am)
    err = abs(xc[am] - energy) / energy
    print(f"prc_channel_offset N64: offset {(am - nl) * IIR_Q}, peak {xc[am]:.6g} against the energy {energy:.6g}: {err:.3g} "
          f"(the edges hold {edge / energy:.3g} of it)")
    assert np.isfinite(xc).all() and np.sort(xc)[-2] < 0.9 * xc[am]
    assert err < 2e-5 + edge / energy                                 # tests/test_gpu_bounds.py: rel_err(xc) < 2e-5


# ---- one display frame and a two-frame persistence stack of 2^30 + 4099 cells ----------------------------------------------
CELLS = 2 ** 30 + 4099


def weighted_percentile(values, counts, p):
    """NumPy's linear percentile of the multiset (values[i] counts[i] times), as display_oracle.percentile computes it"""
    order = np.argsort(values, kind="stable")
    v, c = values[order].astype(np.float64), counts[order]
    cum = np.cumsum(c)
    n = int(cum[-1])
    vi = np.float64(n - 1) * (np.float64(p) / np.float64(100))
    k = int(np.floor(vi))
    t = vi - np.floor(vi)
    a = v[np.searchsorted(cum, k, side="right")]
    b = v[np.searchsorted(cum, min(k + 1, n - 1), side="right")]
    d = b - a
    return a + d * t if t < 0.5 else b - d * (np.float64(1.0) - t)


def test_display_limits_and_rgba():
    """the exact order statistics follow from base and the multiplicities q or q + 1 of its values; the pixels of the first
    H W cells with those limits are compared in full on the device"""
    import display_oracle as DO
    H, W = 32769, 32768                                            # H W = 2^30 + 2^15 cells: the last pixel lies beyond 2^32 bytes
    need(4.1 + 4.1 + 4)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = np.random.default_rng(113).exponential(1.0, P).astype(np.float32)
    x = periodic(base, H * W)                                        # the limits are those of its first CELLS cells
    lim = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.prc_display_limits(x.data_ptr(), _lib.REAL_F32, CELLS, 1, 35.0, 99.0, 1.5, lim.data_ptr(), st))
    torch.cuda.synchronize()
    q, r = divmod(CELLS, P)
    counts = np.full(P, q, np.int64)
    counts[:r] += 1
    want = np.array([weighted_percentile(base, counts, 35.0), np.float64(1.5) * weighted_percentile(base, counts, 99.0)])
    assert np.array_equal(lim.cpu().numpy(), want), (lim.cpu().numpy(), want)
    px = torch.zeros((H * W, 4), dtype=torch.uint8, device="cuda")
    _lib.check(lib.prc_display_rgba(x.data_ptr(), _lib.REAL_F32, H, W, 1, lim.data_ptr(), None, _lib.DISPLAY_STORED, px.data_ptr(), st))
    torch.cuda.synchronize()
    lut = dev(DO.gnuplot2_lut())
    vmin, vmax = float(want[0]), float(want[1])
    piece = 2 ** 26
    for lo in range(0, H * W, piece):
        v = x[lo:lo + piece].to(torch.float64)
        xa = ((v - vmin) / (vmax - vmin)) * 256.0
        idx = torch.where(xa < 0, torch.zeros_like(xa), torch.where(xa >= 256, torch.full_like(xa, 255.0), torch.trunc(xa))).to(torch.int64)
        assert torch.equal(px[lo:lo + piece], lut[idx]), lo


def test_persistence_two_long_frames():
    need(8.1 + 8.1 + 3)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()
    base = np.random.default_rng(114).exponential(1.0, P).astype(np.float32)
    x = periodic(base, 2 * CELLS).view(2, CELLS)
    out = torch.full((CELLS,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.prc_persistence(x.data_ptr(), _lib.REAL_F32, CELLS, 2, 1, 1, 2, 0.9, out.data_ptr(), _lib.REAL_F64, st))
    torch.cuda.synchronize()
    d1 = torch.tensor(np.float32(0.9 ** 1), dtype=torch.float32, device="cuda")
    piece = 2 ** 26
    for lo in range(0, CELLS, piece):
        # the sum starts at +0.0 and adds fl32(x[1] * 1) and fl32(x[0] * fl32(0.9)) widened, in that order
        want = (0.0 + x[1, lo:lo + piece].to(torch.float64)) + (x[0, lo:lo + piece] * d1).to(torch.float64)
        assert torch.equal(out[lo:lo + piece], want), lo
