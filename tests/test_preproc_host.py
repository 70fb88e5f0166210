"""decimate, channel_preprocessing, shift, offset_compensation and normalize without a GPU: the NumPy restatement
(tests/preproc_oracle.py) against goldens written by the reference itself (tools/gen_golden_preproc.py), the argument
handling of passiveradar_amd/signal_utils.py that happens before any device call, and the descriptor of the C ABI.

The restatement (float32 taps, the reference's float32 rotation, float64 sums) is held to 2e-6 of the peak, the project's bar
for small goldens; it measured 8.9e-7 at worst (decimate, q = 97), the reference's own float32 arithmetic."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import preproc_oracle as O
from conftest import REPO, load_golden, rel_err

BAR = 2e-6


@pytest.fixture(scope="module")
def gold():
    return {k: load_golden("preproc_" + k) for k in ("decimate", "channel", "misc")}


def test_decimate_restatement_equals_the_reference(gold):
    g = gold["decimate"]
    for n, q in O.DECIMATE_CASES:
        y = O.decimate(O.decimate_input(n, q), q)
        want = g[f"y_{n}_{q}"]
        assert y.shape == want.shape == (O.out_len(n, q),) and y.dtype == want.dtype == np.complex64
        if np.abs(want).max() > 0:
            assert rel_err(y, want) <= BAR, (n, q, rel_err(y, want))
    y = O.decimate(O.decimate_input(300, 5, 3), 5)
    assert y.shape == (60, 3) and rel_err(y, g["cols"]) <= BAR
    for name in O.DECIMATE_DTYPES:
        y = O.decimate(O.dtype_input(name), 5)
        want = g["dt_" + name]
        assert y.dtype == want.dtype and rel_err(y, want) <= BAR, name
    assert g["dt_int16"].dtype == np.float64 and g["dt_float32"].dtype == np.float32


def test_channel_preprocessing_restatement_equals_the_reference(gold):
    g = gold["channel"]
    for name, (dtype, nscalars, dec, fc, Fs) in O.CHANNEL_CASES.items():
        y = O.channel_preprocessing(O.channel_input(name), dec, fc, Fs)
        want = g["y_" + name]
        assert y.shape == want.shape == (O.out_len(nscalars // 2, dec),) and want.dtype == np.complex64
        assert rel_err(y, want) <= BAR, (name, rel_err(y, want))


def test_long_recording_restatement_where_the_sample_index_rounds(gold):
    """2^24 + 70 000 samples: fl32(i) rounds from 2^24 on, and the closed form of the rotation still is the reference's"""
    g = gold["channel"]
    raw = O.long_input()
    assert np.array_equal(O.checksum(raw), g["long_raw"])
    m = O.out_len(O.LONG_SAMPLES, 10)
    lo = (m - O.LONG_KEEP) * 10 - 100
    z = (O.deinterleave(raw[2 * lo:]) * O.rotation(O.LONG_SAMPLES - lo, 1e5, 2.4e6, start=lo)).astype(np.complex64)
    tail = O.fir_decimate(z, 10)[10:]
    assert tail.shape == (O.LONG_KEEP,)
    assert float(np.abs(tail - g["long_tail"]).max() / g["long_peak"]) <= BAR


def test_shift_offsets_and_normalize_restatements(gold):
    g = gold["misc"]
    for name, x in O.shift_inputs().items():
        for k in O.SHIFTS:
            want = g[f"shift_{name}_{k}"]
            got = O.shift(x, k)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, k)
    x1 = O.offset_input()
    for d in O.OFFSETS:
        os_, same = int(g[f"off_{d}"][0]), int(g[f"off_{d}"][1])
        assert os_ == -d and same == (d == 0)
        out = O.shift(O.shift(x1, d), os_)
        assert np.array_equal(O.checksum(out.view(np.float32).view(np.int8)), g[f"off_{d}"][2:])
    for shape in O.NORMALIZE_SHAPES:
        for dtype in ("float32", "complex64"):
            y = O.normalize(O.normalize_input(shape, dtype))
            want = g[f"norm_{dtype}_" + "x".join(map(str, shape))]
            assert y.dtype == want.dtype == np.dtype(dtype)
            if y.size >= 1000:
                y = y.reshape(-1)[::O.NORMALIZE_STRIDE]
            assert y.shape == want.shape and rel_err(y, want) <= BAR, (shape, dtype)


def test_emulated_kernel_orders_sit_inside_the_gpu_bar(gold):
    """the float32 emulations of the two kernels' summation orders, whose worst error (8.9e-7) times 4 is the GPU bar"""
    g = gold["decimate"]
    for n, q in ((1003, 7), (700, 59), (700, 60), (3000, 97)):
        x = O.decimate_input(n, q)
        em = O.emulate_tile(x, q) if q <= O.TILE_MAX_Q else O.emulate_direct(x, q)
        assert rel_err(em, g[f"y_{n}_{q}"]) <= 1e-6, (n, q)


def _no_device(monkeypatch):
    from passiveradar_amd import _lib, signal_utils
    called = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: called.append("require_gpu"))
    monkeypatch.setattr(_lib, "DeviceBuffer", lambda *a, **k: called.append("DeviceBuffer"))
    monkeypatch.setattr(_lib, "lib", lambda: called.append("lib"))
    monkeypatch.setattr(signal_utils, "lib", lambda: called.append("lib"))
    return called


def test_argument_handling_comes_before_any_device_call(monkeypatch):
    from passiveradar_amd import signal_utils as S
    called = _no_device(monkeypatch)
    x = O.white(100, 1)
    raw = O.raw_int8(200, 2)
    with pytest.raises(ValueError):
        S.decimate(x, 1)                         # firwin: a cut-off at Nyquist
    with pytest.raises(ValueError):
        S.channel_preprocessing(raw, 1, 1e5, 2.4e6)
    with pytest.raises(TypeError):
        S.decimate(x, 4.0)                       # operator.index
    with pytest.raises(TypeError):
        S.channel_preprocessing(raw, 10.0, 1e5, 2.4e6)
    with pytest.raises(ValueError):
        S.decimate(x, 0)
    with pytest.raises(ValueError):
        S.decimate(np.complex64(1), 4)
    with pytest.raises(ValueError):
        S.channel_preprocessing(raw.reshape(2, 100), 10, 1e5, 2.4e6)
    # n = 0: the result's length, shape and dtype, no launch
    table = {"complex64": np.complex64, "complex128": np.complex128, "float32": np.float32, "float64": np.float64,
             "int16": np.float64, "int8": np.float64, "uint8": np.float64, "int64": np.float64}
    for name, want in table.items():
        y = S.decimate(np.zeros(0, name), 4)
        assert y.shape == (0,) and y.dtype == want, name
        y = S.normalize(np.zeros((0, 3), name))
        assert y.shape == (0, 3) and y.dtype == want, name
    assert S.decimate(np.zeros((0, 3), np.complex64), 4).shape == (0, 3)
    assert S.decimate(np.zeros((10, 0), np.complex64), 4).shape == (3, 0)          # ceil(10 / 4) rows of no channels
    for nscalars in (0, 1):
        y = S.channel_preprocessing(np.zeros(nscalars, np.int8), 10, 1e5, 2.4e6)
        assert y.shape == (0,) and y.dtype == np.complex64
    assert S.shift(x, 0) is x
    e = S.shift(np.zeros((0, 2), np.int8), 3)
    assert e.shape == (0, 2) and e.dtype == np.int8
    monkeypatch.setattr(S, "find_channel_offset", lambda s1, s2, nd, nl: 0)
    x2 = O.white(100, 3)
    assert S.offset_compensation(x, x2, 50, 4, 10) is x2
    assert not called


def test_output_lengths():
    for n, q in O.DECIMATE_CASES:
        assert O.out_len(n, q) == (n + q - 1) // q
    for name, (dtype, nscalars, dec, fc, Fs) in O.CHANNEL_CASES.items():
        assert O.out_len(nscalars // 2, dec) == -(-(nscalars // 2) // dec)


def test_the_five_names_are_exported():
    from passiveradar_amd import signal_utils as S
    for name in ("decimate", "channel_preprocessing", "shift", "offset_compensation", "normalize"):
        assert name in S.__all__ and callable(getattr(S, name))


def test_firdec_desc_matches_the_header(tmp_path):
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "f.c"
    fields = ["struct_size", "magic", "q", "ntaps", "raw_dtype", "mix", "fc", "fs", "phase_offset"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_firdec_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %u %u %d %d\\n", sizeof(prc_firdec_desc), PRC_FIRDEC_DESC_SIZE_660, d.struct_size, PRC_VERSION,\n'
                   '         PRC_FIRDEC_TILE_MAX_Q);\n'
                   + "".join(f'  printf("%zu\\n", offsetof(prc_firdec_desc, {f}));\n' for f in fields) + '  return 0; }\n')
    exe = tmp_path / "f"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    size = C.sizeof(_lib.FirdecDesc)
    assert [int(v) for v in lines[0].split()] == [size, size, size, _lib.MIN_LIB_VERSION, _lib.FIRDEC_TILE_MAX_Q]
    assert size == 48 and _lib.MIN_LIB_VERSION >= 660 and _lib.FIRDEC_TILE_MAX_Q == O.TILE_MAX_Q
    assert [int(v) for v in lines[1:]] == [getattr(_lib.FirdecDesc, f).offset for f in fields]
    assert [f for f, _ in _lib.FirdecDesc._fields_] == fields


def test_bad_arguments_are_refused_without_a_gpu():
    from passiveradar_amd import _lib
    lib = _lib.lib()
    assert lib.prc_version() >= 660

    def desc(**kw):
        d = _lib.FirdecDesc()
        d.q, d.ntaps, d.raw_dtype, d.mix, d.fc, d.fs = 4, 81, 4, 0, 0.0, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    p = C.c_void_p(4096)                  # never dereferenced: every call below fails its checks first

    def dec(d, taps=p, x=p, n=100, step=1, stride=100, nch=1, out=p, out_step=1, out_stride=25):
        return lib.prc_fir_decimate(C.byref(d), taps, x, n, step, stride, nch, out, out_step, out_stride, None)

    E = _lib.PRC_EINVAL
    for bad in (dict(q=0), dict(ntaps=80), dict(ntaps=0), dict(raw_dtype=5), dict(raw_dtype=-1), dict(mix=2),
                dict(mix=1, fs=0.0), dict(magic=0), dict(struct_size=40)):
        assert dec(desc(**bad)) == E, bad
    assert "prc_firdec_desc.struct_size = 40" in lib.prc_last_error().decode()
    assert dec(desc(ntaps=(1 << 24) + 1)) == _lib.PRC_ESHAPE
    for kw in (dict(taps=None), dict(x=None), dict(out=None), dict(n=-1), dict(step=0), dict(out_step=0), dict(nch=0),
               dict(nch=65536), dict(nch=2, stride=-1), dict(out=C.c_void_p(4100))):
        assert dec(desc(), **kw) == E, kw
    assert dec(desc(), n=0) == _lib.PRC_OK                      # nothing to do, nothing launched
    assert lib.prc_shift(None, p, 4, 8, 1, None) == E and lib.prc_shift(p, p, -1, 8, 1, None) == E
    assert lib.prc_shift(p, p, 4, 0, 1, None) == E and lib.prc_shift(p, p, 0, 8, 1, None) == _lib.PRC_OK
    b = C.c_size_t(0)
    assert lib.prc_normalize_workspace_bytes(0, C.byref(b)) == E and lib.prc_normalize_workspace_bytes(10, None) == E
    for n, want in ((1, 8), (8192, 8), (8193, 16), (10 ** 9, 8 * 256)):
        assert lib.prc_normalize_workspace_bytes(n, C.byref(b)) == _lib.PRC_OK and b.value == want, n
    assert lib.prc_normalize(None, p, 10, 0, p, None) == E and lib.prc_normalize(p, p, 0, 0, p, None) == E
    assert lib.prc_normalize(p, p, 10, 2, p, None) == E and lib.prc_normalize(p, p, 10, 0, C.c_void_p(4100), None) == E
