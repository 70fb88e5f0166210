"""prc_batch_xambg / prc_ofdm_timing without a GPU: the ABI, the first refused value of every limit with its status and
message, the front doors' Python errors, and the properties of tests/batch_xambg_oracle.py that the GPU tests rely on -- the
direct-summation form against scalar loops bit for bit, the scipy form against it, the float32 emulation against the bar, and
the design scene's thresholds held by the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import batch_xambg_oracle as O


def _lib():
    from passiveradar_amd import _lib
    return _lib


def _desc(n=300000, L=1024, R=64, F=256, hop=1152, start=165, filt=1, floor=0.1):
    from passiveradar_amd import engine
    return engine.batch_xambg_desc(n, L, R, F, hop, start, filt, floor)


def _status(d, nframes=1):
    L = _lib()
    nb = C.c_size_t(12345)
    rc = L.lib().prc_batch_xambg_workspace_bytes(C.byref(d), nframes, C.byref(nb))
    return rc, L.lib().prc_last_error().decode(), nb.value


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_descriptor_symbols_argtypes():
    L = _lib()
    assert C.sizeof(L.BatchXambgDesc) == 56
    offs = {f[0]: getattr(L.BatchXambgDesc, f[0]).offset for f in L.BatchXambgDesc._fields_}
    assert offs == dict(struct_size=0, magic=4, n=8, start=16, hop=24, batch_len=32, range_bins=36, freq_bins=40, filter=44, floor=48,
                        reserved=52)
    types = dict((f[0], f[1]) for f in L.BatchXambgDesc._fields_)
    assert types["n"] is C.c_int64 and types["start"] is C.c_int64 and types["hop"] is C.c_int64 and types["floor"] is C.c_float
    for name in ("prc_batch_xambg_workspace_bytes", "prc_batch_xambg", "prc_ofdm_timing"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(L.lib(), name)
    sig = L._SIGNATURES["prc_batch_xambg"][1]
    assert len(sig) == 9 and sig[3] is C.c_int64 and sig[6] is C.c_int32
    sig = L._SIGNATURES["prc_ofdm_timing"][1]
    assert len(sig) == 8 and sig[1] is C.c_int64 and sig[2:5] == [C.c_int32] * 3
    assert (L.BATCH_MATCHED, L.BATCH_RECIPROCAL) == (0, 1) and L.BATCH_FILTERS == {"matched": 0, "reciprocal": 1}


def test_header_constants(tmp_path):
    import os
    import subprocess
    from conftest import REPO
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "include/prcore.h"\nint main(void) { printf("%u %lld %d %d %u\\n", '
                   "PRC_BATCH_XAMBG_DESC_SIZE_MIN, (long long)PRC_BATCH_XAMBG_MAX_BATCHES, PRC_BATCH_MATCHED, PRC_BATCH_RECIPROCAL, "
                   "(unsigned)sizeof(prc_batch_xambg_desc)); return 0; }\n")
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split()
    L = _lib()
    assert got == ["56", str(L.BATCH_XAMBG_MAX_BATCHES), "0", "1", "56"]
    assert os.path.exists(os.path.join(REPO, "passiveradar_amd", "csrc", "caf_batch.hip"))


def test_workspace_is_the_tile_major_slow_time_buffer():
    # tiles of 32 / 16 / 8 / 8 / 4 columns at 256 / 512 / 1024 / 2048 / 4096 batches
    for F, kt in ((256, 32), (512, 16), (1024, 8), (2048, 8), (4096, 4)):
        for R in (0, kt - 1, kt, 70):
            d = _desc(n=2 ** 27, F=F, R=R, hop=1024, start=0)
            rc, msg, nb = _status(d, 3)
            assert rc == 0, msg
            assert nb == 8 * 3 * F * (-(-(R + 1) // kt) * kt), (F, R, nb)


# ---- limits: the value at the limit passes, the first beyond it is refused --------------------------------------------------
def test_descriptor_header_is_checked():
    L = _lib()
    d = _desc()
    d.magic = 0
    assert _status(d)[0] == L.PRC_EINVAL and "magic" in _status(d)[1]
    d = _desc()
    d.struct_size = 52
    assert _status(d)[0] == L.PRC_EINVAL and "struct_size" in _status(d)[1]


LIMITS = [
    # (fields at the limit, fields one past it, status name, words of the message)
    (dict(L=1024), dict(L=2048), "PRC_EUNSUPPORTED", ("batch_len = 2048", "1024 or 4096")),
    (dict(L=4096, hop=1, start=0, n=5000), dict(L=4097, hop=1, start=0, n=5000), "PRC_EUNSUPPORTED", ("batch_len = 4097",)),
    (dict(F=4096, hop=1, start=0, n=6000), dict(F=8192, hop=1, start=0, n=20000), "PRC_EUNSUPPORTED", ("freq_bins = 8192", "256")),
    (dict(F=256), dict(F=128), "PRC_EUNSUPPORTED", ("freq_bins = 128",)),
    (dict(F=256), dict(F=300), "PRC_EUNSUPPORTED", ("freq_bins = 300",)),
    (dict(start=0), dict(start=-1), "PRC_ESHAPE", ("start = -1",)),
    (dict(hop=1), dict(hop=0), "PRC_ESHAPE", ("hop = 0",)),
    (dict(R=0), dict(R=-1), "PRC_ESHAPE", ("range_bins = -1",)),
    (dict(R=1023), dict(R=1024), "PRC_ESHAPE", ("range_bins = 1024", "1023")),
    (dict(L=4096, hop=4096, n=2 ** 21, R=4095), dict(L=4096, hop=4096, n=2 ** 21, R=4096), "PRC_ESHAPE", ("range_bins = 4096", "4095")),
    (dict(n=165 + 255 * 1152 + 1024), dict(n=165 + 255 * 1152 + 1023), "PRC_ESHAPE", ("last batch", "beyond n = 294948")),
    (dict(n=536805376), dict(n=536805377), "PRC_ESHAPE", ("n = 536805377", "536805376", "PRC_CAF_MAX_N")),
    (dict(filt=1), dict(filt=2), "PRC_EINVAL", ("filter = 2",)),
    (dict(filt=0), dict(filt=-1), "PRC_EINVAL", ("filter = -1",)),
    (dict(floor=0.0), dict(floor=-0.001), "PRC_EINVAL", ("floor",)),
    (dict(floor=1e30), dict(floor=float("inf")), "PRC_EINVAL", ("floor",)),
    (dict(floor=1.0), dict(floor=float("nan")), "PRC_EINVAL", ("floor",)),
]


@pytest.mark.parametrize("at_limit,refused,status,words", LIMITS, ids=[repr(c[1]) for c in LIMITS])
def test_limit(at_limit, refused, status, words):
    L = _lib()
    rc, msg, nb = _status(_desc(**at_limit))
    assert rc == L.PRC_OK and nb > 0, (at_limit, msg)
    rc, msg, nb = _status(_desc(**refused))
    assert rc == getattr(L, status) and nb == 0, (refused, rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    # the entry point itself refuses the same descriptor before it looks at a pointer
    rc = L.lib().prc_batch_xambg(C.byref(_desc(**refused)), None, None, 0, None, None, 1, None, None)
    assert rc == getattr(L, status) and all(w in L.lib().prc_last_error().decode() for w in words)


def test_frame_count_limit_and_null_arguments():
    L = _lib()
    d = _desc()
    most = (2 ** 31 - 1) // 256
    assert _status(d, most)[0] == L.PRC_OK
    rc, msg, _ = _status(d, most + 1)
    assert rc == L.PRC_ESHAPE and f"{(most + 1) * 256} batches" in msg and "PRC_BATCH_XAMBG_MAX_BATCHES" in msg
    assert _status(d, -1)[0] == L.PRC_EINVAL
    assert _status(d, 0)[0] == L.PRC_OK and _status(d, 0)[2] == 0
    assert L.lib().prc_batch_xambg(C.byref(d), None, None, 0, None, None, 0, None, None) == L.PRC_OK      # no frames: a no-op
    assert L.lib().prc_batch_xambg(C.byref(d), None, None, 0, None, None, 1, None, None) == L.PRC_EINVAL
    assert "null" in L.lib().prc_last_error().decode()
    assert L.lib().prc_batch_xambg(C.byref(d), 8, 8, 0, None, 8, 1, 12, None) == L.PRC_EINVAL            # workspace off by 4 bytes
    assert "alignment" in L.lib().prc_last_error().decode()


def test_timing_limits():
    L = _lib()
    fn = L.lib().prc_ofdm_timing
    need = (3 + 1) * (100 + 7) + 100
    assert fn(None, need - 1, 100, 7, 3, None, None, None) == L.PRC_ESHAPE
    msg = L.lib().prc_last_error().decode()
    assert f"= {need} samples are needed" in msg and f"n = {need - 1}" in msg
    assert fn(None, need, 100, 7, 3, None, None, None) == L.PRC_EINVAL and "null" in L.lib().prc_last_error().decode()
    for nfft, cp, nsym in ((1, 1, 1), (8, 0, 1), (8, 8, 1), (8, 3, 0)):
        assert fn(None, 10 ** 6, nfft, cp, nsym, None, None, None) == L.PRC_EINVAL, (nfft, cp, nsym)
    assert fn(None, 2 ** 40, 2 ** 31 - 1, 1, 1, None, None, None) == L.PRC_ESHAPE and "offsets" in L.lib().prc_last_error().decode()
    assert fn(None, 7, 2, 1, 1, None, None, None) == L.PRC_ESHAPE                  # the smallest sizes need 2 * 3 + 2 = 8 samples
    assert fn(None, 8, 2, 1, 1, None, None, None) == L.PRC_EINVAL                  # enough samples: only the pointers are missing


# ---- the front doors' Python errors: before the library, before a device --------------------------------------------------
def test_front_door_errors():
    from passiveradar_amd.range_doppler_processing import batch_xambg, ofdm_symbol_start
    x = np.zeros(300000, np.complex64)
    ok = dict(rangeBins=64, freqBins=256, batchLen=1024, hop=1152, start=165)

    def call(**kw):
        a = dict(ok, **kw)
        return batch_xambg(a.pop("ref", x), a.pop("srv", x), a.pop("rangeBins"), a.pop("freqBins"), a.pop("batchLen"), **a)

    with pytest.raises(ValueError, match="same length"):
        call(srv=x[:-1])
    with pytest.raises(ValueError, match="one-dimensional channels or"):
        call(ref=x.reshape(2, 2, -1), srv=x.reshape(2, 2, -1))
    with pytest.raises(ValueError, match="filter is"):
        call(filter="inverse")
    with pytest.raises(NotImplementedError, match="batchLen = 2048"):
        call(batchLen=2048)
    with pytest.raises(NotImplementedError, match="freqBins = 100"):
        call(freqBins=100)
    with pytest.raises(ValueError, match="start = -1"):
        call(start=-1)
    with pytest.raises(ValueError, match="hop = 0"):
        call(hop=0)
    with pytest.raises(ValueError, match="rangeBins = 1024"):
        call(rangeBins=1024)
    with pytest.raises(ValueError, match="last batch ends at"):
        call(start=300000 - 255 * 1152 - 1024 + 1)
    with pytest.raises(ValueError, match="last batch ends at"):
        call(hop=None, start=300000 - 256 * 1024 + 1)                            # hop defaults to batchLen
    with pytest.raises(ValueError, match="floor"):
        call(floor=-1.0)
    with pytest.raises(ValueError, match="broadcast"):
        call(window=np.ones(255, np.float32))
    with pytest.raises(ValueError, match="broadcast"):
        call(window=np.ones((256, 1), np.float32))
    with pytest.raises(ValueError, match="one-dimensional"):
        ofdm_symbol_start(x.reshape(2, -1), 1024, 128)
    with pytest.raises(ValueError, match="cp = 0"):
        ofdm_symbol_start(x, 1024, 0)
    with pytest.raises(ValueError, match="cp = 8"):
        ofdm_symbol_start(x, 8, 8)
    with pytest.raises(ValueError, match="samples are needed"):
        ofdm_symbol_start(x[:2 * 1152 + 1023], 1024, 128)
    with pytest.raises(ValueError, match="samples are needed"):
        ofdm_symbol_start(x, 1024, 128, nsym=(300000 - 1024) // 1152)


# ---- the oracle -----------------------------------------------------------------------------------------------------------
TINY = dict(L=16, F=4, R=5, hop=12, start=3)


@pytest.mark.parametrize("filt", [O.RECIPROCAL, O.MATCHED])
def test_direct_summation_equals_the_scalar_loops_bit_for_bit(filt):
    ref, srv = O.white(3 + 3 * 12 + 16 + 2, 11), O.white(3 + 3 * 12 + 16 + 2, 12)
    win = np.array([0.25, 1.0, 0.75, 0.5], np.float32)
    for floor, w in ((0.1, None), (0.4, win)):
        a = O.surface_direct(ref, srv, filt=filt, floor=floor, window=w, **TINY)
        b = O.surface_brute(ref, srv, filt=filt, floor=floor, window=w, **TINY)
        assert a.shape == (4, 6) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        # the scipy form, which the device is held to, is the same definition: it differs by roundings of float64 only
        assert O.rel_err(O.surface(ref, srv, filt=filt, floor=floor, window=w, **TINY), a) < 1e-13
    # the floor matters on this case (the test can tell 0.1 from 0.4) and a silent reference batch contributes nothing
    if filt == O.RECIPROCAL:
        assert O.rel_err(O.surface(ref, srv, floor=0.1, **TINY), O.surface(ref, srv, floor=0.4, **TINY)) > 1e-3
    dead = ref.copy()
    dead[3 + 12:3 + 12 + 16 + 12] = 0                                            # batches 1 and 2 (they overlap)
    c = O.profiles(dead, srv, 16, 12, 3, 4, 5, filt, 0.1)
    assert np.all(c[1] == 0) and np.isfinite(c).all() and np.abs(c[0]).max() > 0
    assert np.isfinite(O.surface_direct(dead, srv, filt=filt, **TINY)).all()


def test_scipy_form_against_direct_summation_at_a_transform_length():
    ref, srv = O.white(1024 + 3 * 700, 21), O.white(1024 + 3 * 700, 22)
    # (F = 4 is not a length the device takes: the oracle has no such limit)
    a = O.surface(ref, srv, 1024, 4, 9, hop=700, start=0, floor=0.3)
    b = O.surface_direct(ref, srv, 1024, 4, 9, hop=700, start=0, floor=0.3)
    assert O.rel_err(a, b) < 1e-12


def test_timing_metric_against_scalar_loops():
    ref = O.white(4 * 107 + 100, 31)
    m = O.timing_metric(ref, 100, 7, 3)
    z = ref.astype(np.complex128)
    for o in (0, 1, 50, 106):
        acc = 0j
        for s in range(3):
            for t in range(7):
                acc += z[o + s * 107 + t] * np.conj(z[o + s * 107 + t + 100])
        assert abs(abs(acc) - m[o]) <= 1e-13 * m.max()
    assert m.shape == (107,)


def test_design_scene_on_the_oracle():
    D = O.DESIGN
    ref, srv = O.design_scene()
    nsym = (D["n"] - D["L"]) // D["hop"] - 1
    assert O.symbol_start(ref, D["L"], D["cp"], nsym) == D["symbol_start"]
    Xr = O.surface(ref, srv, **O.design_args(O.RECIPROCAL))
    Xm = O.surface(ref, srv, **O.design_args(O.MATCHED))
    c = O.design_conditions(Xr, Xm)
    print(c)
    O.check_design(c)
    # misaligned batches: the reciprocal filter gains nothing (the documented limit)
    off = dict(O.design_args(O.RECIPROCAL), start=D["symbol_start"] + D["cp"] + 500)
    A = np.abs(O.surface(ref, srv, **off))
    assert A[c["weak"]] / np.median(A) < 5.0
    # float32 emulation: a quarter of the bar
    for filt, X in ((O.RECIPROCAL, Xr), (O.MATCHED, Xm)):
        e = O.rel_err(O.emulate32(ref, srv, **O.design_args(filt)), X)
        print(f"emulation, L = 1024, {filt}: {e:.3g}")
        assert e <= O.GPU_BAR / 4


def test_qpsk_makes_the_two_filters_coincide():
    ref, srv = O.design_scene(order=2)
    Xr = O.surface(ref, srv, **O.design_args(O.RECIPROCAL))
    Xm = O.surface(ref, srv, **O.design_args(O.MATCHED))
    e = O.rel_err(Xr / np.abs(Xr).max(), Xm / np.abs(Xm).max())
    print(f"QPSK: normalised surfaces differ by {e:.3g}")
    assert e <= 0.01


def test_emulation_at_4096_points():
    n = 549 + 255 * 4608 + 4096
    ref = O.white(n, 41)
    srv = (0.5 * np.roll(ref, 30) + 0.01 * O.white(n, 42)).astype(np.complex64)
    for filt in (O.RECIPROCAL, O.MATCHED):
        a = dict(L=4096, F=256, R=64, hop=4608, start=549, filt=filt, floor=0.1)
        e = O.rel_err(O.emulate32(ref, srv, **a), O.surface(ref, srv, **a))
        print(f"emulation, L = 4096, {filt}: {e:.3g}")
        assert e <= O.GPU_BAR / 4
