"""Welch spectra without a GPU: the NumPy restatement (tests/psd_oracle.py) against matplotlib.mlab, the argument checks of
passiveradar_amd/spectral.py (raised before any device call), the descriptor's layout and the size arithmetic of the C ABI."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import psd_oracle as P
from conftest import REPO

FS = 2.4e6


def peak_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("nfft", [64, 256, 2048, 8192])
def test_restatement_equals_mlab(nfft):
    mlab = pytest.importorskip("matplotlib.mlab")
    for noverlap in P.overlaps(nfft):
        for name, x in P.cases(nfft, noverlap).items():
            x = x.astype(np.complex128)      # mlab detrends in the input's own precision: give it the values in float64
            for detrend in ("none", "mean"):
                for sbf in (True, False):
                    want, f = mlab.psd(x, NFFT=nfft, Fs=FS, detrend=detrend, noverlap=noverlap, scale_by_freq=sbf)
                    got = P.psd(x, NFFT=nfft, Fs=FS, detrend=detrend, noverlap=noverlap, scale_by_freq=sbf)
                    assert peak_err(got, want) <= 1e-12, (nfft, noverlap, name, detrend, sbf)
                    assert np.array_equal(P.freqs(nfft, FS), f)
            y = np.roll(x, 3) * (0.5 - 0.2j) + 0.1 * P.white(x.shape[0], 99)
            want, _ = mlab.csd(x, y, NFFT=nfft, Fs=FS, detrend="mean", noverlap=noverlap)
            assert peak_err(P.csd(x, y, NFFT=nfft, Fs=FS, detrend="mean", noverlap=noverlap), want) <= 1e-12
            want, f, t = mlab.specgram(x, NFFT=nfft, Fs=FS, noverlap=noverlap)
            assert peak_err(P.specgram(x, NFFT=nfft, Fs=FS, noverlap=noverlap), want) <= 1e-12
            assert np.array_equal(P.times(x.shape[0], nfft, FS, noverlap), t)


def test_restatement_short_input_window_and_rows():
    mlab = pytest.importorskip("matplotlib.mlab")
    x = P.dc(256 - 5, 3).astype(np.complex128)
    for detrend in ("none", "mean"):
        want, _ = mlab.psd(x, NFFT=256, Fs=FS, detrend=detrend, noverlap=0)
        assert peak_err(P.psd(x, NFFT=256, Fs=FS, detrend=detrend), want) <= 1e-12
    w = np.kaiser(256, 5.0)
    x = P.white(7 * 256, 4).astype(np.complex128)
    want, _ = mlab.psd(x, NFFT=256, Fs=FS, window=w, noverlap=0)
    assert peak_err(P.psd(x, NFFT=256, Fs=FS, window=w), want) <= 1e-12
    per_seg, _, t = mlab.specgram(x, NFFT=256, Fs=FS, noverlap=0)
    for navg, rows in ((1, 7), (2, 3), (3, 2), (7, 1), (0, 1)):
        got = P.specgram(x, navg=navg, NFFT=256, Fs=FS, noverlap=0)
        k = 7 if navg == 0 else navg
        assert got.shape == (256, rows)
        for r in range(rows):
            assert peak_err(got[:, r], per_seg[:, r * k:(r + 1) * k].mean(axis=1)) <= 1e-12
        assert np.allclose(P.times(x.shape[0], 256, FS, 0, navg), [t[r * k:(r + 1) * k].mean() for r in range(rows)], rtol=1e-15)
    with pytest.raises(ValueError):
        P.specgram(x, navg=8, NFFT=256, Fs=FS, noverlap=0)
    # step: every second sample
    z = np.empty(2 * x.shape[0], np.complex128)
    z[0::2], z[1::2] = x, np.nan
    assert np.array_equal(P.psd(z, NFFT=256, Fs=FS, step=2), P.psd(x, NFFT=256, Fs=FS))


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from passiveradar_amd import _lib, spectral
    called = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: called.append("require_gpu"))
    monkeypatch.setattr(_lib, "DeviceBuffer", lambda *a, **k: called.append("DeviceBuffer"))
    x = P.white(7 * 256, 5)
    bad = [dict(detrend="linear"), dict(detrend=lambda v: v), dict(window=np.ones(255)), dict(window=np.hanning),
           dict(NFFT=100), dict(NFFT=32), dict(NFFT=16384), dict(noverlap=256), dict(noverlap=-1), dict(step=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            spectral.psd(x, **{"NFFT": 256, **kw})
    with pytest.raises(ValueError):
        spectral.csd(x, x[:-1], NFFT=256)
    with pytest.raises(ValueError):
        spectral.specgram(x, NFFT=256, noverlap=0, navg=8)          # 7 segments
    with pytest.raises(ValueError):
        spectral.specgram(x, NFFT=256, noverlap=0, navg=-1)
    with pytest.raises(ValueError):
        spectral.psd(x.astype(np.complex128).view(np.float64), NFFT=256, raw=True)     # float64 scalars are no raw type
    with pytest.raises(ValueError):
        spectral.psd(np.zeros((2, 2, 512), np.complex64), NFFT=256)
    with pytest.raises(ValueError):
        spectral.preview(dict(interleaved_input_channels=False, input_chunk_length=1000, input_sample_rate=FS,
                              input_center_freq=0.0), np.zeros(1000, np.int8))
    assert not called


def test_welch_desc_matches_the_header(tmp_path):
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "w.c"
    fields = ["struct_size", "magic", "nfft", "noverlap", "navg", "detrend", "in_dtype", "step", "scale"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_welch_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %u %u %d\\n", sizeof(prc_welch_desc), PRC_WELCH_DESC_SIZE_650, d.struct_size, PRC_VERSION);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(prc_welch_desc, {f}));\n' for f in fields) + '  return 0; }\n')
    exe = tmp_path / "w"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    size = C.sizeof(_lib.WelchDesc)
    assert [int(v) for v in lines[0].split()] == [size, size, size, _lib.MIN_LIB_VERSION]
    assert _lib.MIN_LIB_VERSION >= 650
    assert [int(v) for v in lines[1:]] == [getattr(_lib.WelchDesc, f).offset for f in fields]
    assert [f for f, _ in _lib.WelchDesc._fields_] == fields


def _desc(**kw):
    from passiveradar_amd import _lib
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.in_dtype, d.step, d.scale = 256, 0, 0, 0, 4, 1, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_rows_and_workspace_bytes_answer_without_a_gpu():
    from passiveradar_amd import _lib
    lib = _lib.lib()
    assert lib.prc_version() >= 650

    def rows(n, **kw):
        d, nseg, r = _desc(**kw), C.c_int64(-1), C.c_int64(-1)
        rc = lib.prc_welch_rows(C.byref(d), n, C.byref(nseg), C.byref(r))
        return rc, nseg.value, r.value

    assert rows(256) == (0, 1, 1) and rows(251) == (0, 1, 1) and rows(1) == (0, 1, 1)
    assert rows(7 * 256 + 255) == (0, 7, 1)
    assert rows(200, nfft=64, noverlap=63) == (0, 137, 1)
    assert rows(9 * 256 + 3, noverlap=37) == (0, (9 * 256 + 3 - 256) // 219 + 1, 1)
    for navg, want in ((1, 7), (2, 3), (3, 2), (7, 1), (0, 1)):
        assert rows(7 * 256, navg=navg) == (0, 7, want)
    assert rows(7 * 256, navg=8)[0] == _lib.PRC_ESHAPE and "navg" in lib.prc_last_error().decode()
    for bad in (dict(nfft=100), dict(nfft=32), dict(nfft=16384), dict(noverlap=256), dict(noverlap=-1), dict(navg=-1),
                dict(step=0), dict(in_dtype=5), dict(detrend=2), dict(magic=0), dict(struct_size=32)):
        assert rows(1000, **bad)[0] == _lib.PRC_EINVAL, bad
    assert rows(0)[0] == _lib.PRC_EINVAL
    assert lib.prc_welch_rows(C.byref(_desc()), 1000, None, None) == _lib.PRC_EINVAL

    def ws(n, nch, **kw):
        d, b = _desc(**kw), C.c_size_t(0)
        rc = lib.prc_welch_workspace_bytes(C.byref(d), n, nch, C.byref(b))
        return rc, b.value

    rc, one = ws(256, 1)
    assert rc == 0 and one == 8 * 256 + 16 * 256            # the twiddles and one workgroup's two components
    # the split of a row over workgroups is a function of the shape alone, and the bytes grow with channels and rows
    assert ws(100 * 256, 1) == ws(100 * 256, 1)
    assert ws(7 * 256, 3, navg=1)[1] == 8 * 256 + 16 * 256 * 3 * 7
    assert ws(100 * 256, 1)[1] > one and ws(100 * 256, 2)[1] > ws(100 * 256, 1)[1]
    assert ws(1000, 0)[0] == _lib.PRC_EINVAL and ws(7 * 256, 1, navg=8)[0] == _lib.PRC_ESHAPE
    # null pointers and a bad descriptor are refused before prc_welch touches a device
    d = _desc()
    assert lib.prc_welch(C.byref(d), None, None, 1000, 1000, 1, None, None, None, None) == _lib.PRC_EINVAL
    assert lib.prc_welch(C.byref(_desc(nfft=100)), None, None, 1000, 1000, 1, None, None, None, None) == _lib.PRC_EINVAL
