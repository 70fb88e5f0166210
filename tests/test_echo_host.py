"""cancel_echoes without a GPU: the scene the feature was designed on reproduced from the oracle alone (tests/echo_oracle.py),
the ABI layout of the three new structs, and every argument check (host arithmetic)."""
import ctypes
import functools

import numpy as np
import pytest

import echo_oracle as EO

LAGS = np.arange(64)
DOPS = np.arange(-32, 32).astype(np.float64)       # Hz: one cell is 1 Hz in the design scene


@functools.lru_cache(maxsize=1)
def _scene():
    ref, srv, fs = EO.design_scene()
    before = EO.surface(ref, srv, fs, LAGS, DOPS) / ref.shape[0]
    return ref, srv, fs, before


def _db(out, srv):
    return 10 * np.log10(np.sum(np.abs(out.astype(np.complex128)) ** 2) / np.sum(np.abs(srv.astype(np.complex128)) ** 2))


def test_the_strong_echoes_mask_the_weak_one():
    """before: the weak echo's cell (lag 9, -6 Hz) reads what the pedestal reads -- within 0.9 .. 1.1 of the surface median --
    and the surface's argmax is the unit echo"""
    _, _, _, S = _scene()
    weak = S[list(DOPS).index(-6.0), 9]
    med = np.median(S)
    print(f"weak cell {weak:.4g}, median {med:.4g}, ratio {weak / med:.3f}")
    assert 0.9 <= weak / med <= 1.1
    assert np.unravel_index(S.argmax(), S.shape) == (list(DOPS).index(3.0), 7)


@pytest.mark.parametrize("refine", [1, 2])
def test_slope_columns_and_gauss_newton_reach_the_floor_from_whole_cells(refine):
    """after, from the whole cells (7, 3 Hz) and (12, -3 Hz): the cleaned surface's argmax is the weak echo's cell, the
    residual power is <= -45 dB, the Dopplers come out within 1e-3 Hz of 3.3 and -2.7 and cond(G) < 100"""
    ref, srv, fs, _ = _scene()
    out, fit, info, cond = EO.cancel(ref, srv, fs, [7, 12], [3.0, -3.0], wrap=True, ramp=True, refine=refine, return_cond=True)
    S = EO.surface(ref, out, fs, LAGS, DOPS) / ref.shape[0]
    am = np.unravel_index(S.argmax(), S.shape)
    print(f"refine {refine}: residual {_db(out, srv):.2f} dB, Dopplers {fit['doppler']}, cond {cond:.2f}, peak {S.max():.3g}, "
          f"median {np.median(S):.3g}")
    assert info == 0 and (DOPS[am[0]], LAGS[am[1]]) == (-6.0, 9)
    assert _db(out, srv) <= -45.0
    assert cond < 100
    # the Dopplers the final fit arrives at (its own slope term included) and, from the second update on, the records themselves
    assert np.abs(EO.implied_dopplers(fit, fs, ref.shape[0]) - [3.3, -2.7]).max() < 1e-3
    if refine >= 2:
        assert np.abs(fit["doppler"] - [3.3, -2.7]).max() < 1e-3
    assert S.max() > 20 * np.median(S)


def test_plain_atoms_are_not_enough():
    """one plain atom per strong echo at its whole cell leaves the scene almost as it was, and a Doppler error of 0.01 cell alone
    leaves more than -36 dB of a lone unit echo: why the slope column and the refinement exist"""
    ref, srv, fs, _ = _scene()
    out, _, _ = EO.cancel(ref, srv, fs, [7, 12], [3.0, -3.0], wrap=True, ramp=False, refine=0)
    assert _db(out, srv) > -18.0
    out, _, _ = EO.cancel(ref, srv, fs, [7, 12], [3.0, -3.0], wrap=True, ramp=True, refine=0)
    assert -19.0 < _db(out, srv) < -17.0                       # the slope column alone, no update
    lone = EO.echo(ref, 7, 3.3, fs, 1.0, True).astype(np.complex64)
    out, _, _ = EO.cancel(ref, lone, fs, [7], [3.31], wrap=True, ramp=False, refine=0)
    print(f"0.01 Hz off: {_db(out, lone):.2f} dB")
    assert _db(out, lone) > -36.0


def test_oracle_rules():
    """skipped atoms, breakdown, dead air and the empty list, on the oracle"""
    ref, srv, fs, _ = _scene()
    n = ref.shape[0]
    good, _, _ = EO.cancel(ref, srv, fs, [7, 12], [3.0, -3.0], refine=1)
    out, fit, info = EO.cancel(ref, srv, fs, [n, 7, -n, 12, 3], [0.0, 3.0, 1.0, -3.0, np.nan], refine=1)
    assert info == 0 and np.array_equal(out, good) and fit["flags"].tolist() == [1, 0, 1, 0, 1]
    out, fit, info = EO.cancel(ref, srv, fs, [7, 7], [3.0, 3.0])
    assert info == 1 and np.array_equal(out, srv) and (fit["flags"] == EO.BROKE_DOWN).all() and not fit["amp"].any()
    out, fit, info = EO.cancel(np.zeros_like(ref), srv, fs, [7], [3.0])
    assert info == 1 and np.array_equal(out, srv)
    out, fit, info = EO.cancel(ref, np.zeros_like(srv), fs, [7, 12], [3.0, -3.0])
    assert info == 0 and not out.any() and not fit["amp"].any() and fit["doppler"].tolist() == [3.0, -3.0]
    out, fit, info = EO.cancel(ref, srv, fs, [], [])
    assert info == 0 and np.array_equal(out, srv) and fit.shape == (0,)
    # a Doppler half a cell and more away: the update is clamped and says so
    _, fit, _ = EO.cancel(ref, EO.echo(ref, 7, 3.3, fs, 1.0).astype(np.complex64), fs, [7], [2.4], refine=1)
    assert fit["flags"][0] & EO.CLAMPED and fit["doppler"][0] == 2.9


def test_structs_match_the_header(tmp_path):
    """sizeof / offsetof of prc_echo_desc, prc_echo_atom and prc_echo_fit as gcc lays them out == the ctypes mirrors and the
    NumPy views; the constants agree; both symbols are declared and exported"""
    import shutil
    import subprocess
    from conftest import REPO
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("prc_echo_desc", _lib.EchoDesc), ("prc_echo_atom", _lib.EchoAtom), ("prc_echo_fit", _lib.EchoFit))
    body = ""
    for cname, cls in structs:
        body += f'  printf("%zu\\n", sizeof({cname}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n, _ in cls._fields_)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_echo_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%u %u %d %d %d\\n", PRC_ECHO_DESC_SIZE_MIN, d.struct_size, PRC_ECHO_MAX_ATOMS, PRC_ECHO_MAX_REFINE,\n'
                   '         PRC_VERSION);\n' + body + '  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", REPO, str(src), "-o", str(exe)])
    lines = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert [int(v) for v in lines[0]] == [ctypes.sizeof(_lib.EchoDesc), ctypes.sizeof(_lib.EchoDesc), _lib.ECHO_MAX_ATOMS,
                                          _lib.ECHO_MAX_REFINE, _lib.MIN_LIB_VERSION]
    want = []
    for _, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    assert [int(ln[0]) for ln in lines[1:]] == want
    assert ctypes.sizeof(_lib.EchoAtom) == 16 == _lib.ECHO_ATOM_DTYPE.itemsize
    assert ctypes.sizeof(_lib.EchoFit) == 48 == _lib.ECHO_FIT_DTYPE.itemsize == EO.FIT_DTYPE.itemsize
    for name, cls, dt in (("lag", _lib.EchoAtom, _lib.ECHO_ATOM_DTYPE), ("doppler", _lib.EchoAtom, _lib.ECHO_ATOM_DTYPE),
                          ("doppler", _lib.EchoFit, _lib.ECHO_FIT_DTYPE), ("amp", _lib.EchoFit, _lib.ECHO_FIT_DTYPE),
                          ("slope", _lib.EchoFit, _lib.ECHO_FIT_DTYPE), ("flags", _lib.EchoFit, _lib.ECHO_FIT_DTYPE)):
        assert getattr(cls, name).offset == dt.fields[name][1]
    assert (_lib.ECHO_SKIPPED, _lib.ECHO_CLAMPED, _lib.ECHO_BROKE_DOWN) == (EO.SKIPPED, EO.CLAMPED, EO.BROKE_DOWN)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("prc_echo_cancel_workspace_bytes", "prc_echo_cancel"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(handle, sym)


def _desc(**kw):
    from passiveradar_amd import _lib
    d = _lib.EchoDesc()
    d.n, d.frame_stride, d.out_stride, d.nframes, d.max_atoms = 6001, 6001, 6001, 1, 4
    d.wrap, d.ramp, d.refine, d.sample_rate, d.reg = 0, 1, 2, 6001.0, 0.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD = (dict(n=0), dict(n=-5), dict(nframes=0), dict(nframes=-1), dict(nframes=2, frame_stride=6000),
       dict(nframes=2, out_stride=6000), dict(nframes=3, frame_stride=0), dict(max_atoms=0), dict(max_atoms=33), dict(max_atoms=-1),
       dict(wrap=2), dict(wrap=-1), dict(ramp=2), dict(ramp=-1), dict(refine=-1), dict(refine=9), dict(refine=1, ramp=0),
       dict(reg=-1e-9), dict(reg=float("nan")), dict(reg=float("inf")), dict(sample_rate=0.0), dict(sample_rate=float("nan")),
       dict(sample_rate=float("inf")), dict(magic=0), dict(struct_size=64), dict(struct_size=74))


def test_c_abi_argument_errors_need_no_device():
    """every PRC_EINVAL case of the header, from prc_echo_cancel_workspace_bytes and from prc_echo_cancel itself (which checks
    before it launches); PRC_ESHAPE for what the kernels' index arithmetic does not hold"""
    from passiveradar_amd import _lib
    lib = _lib.lib()
    nb = ctypes.c_size_t(0)
    one = ctypes.c_void_p(16)         # non-null, aligned, never dereferenced: every call below fails before a launch

    def ws(d):
        return lib.prc_echo_cancel_workspace_bytes(ctypes.byref(d), ctypes.byref(nb))

    def run(d, ref=one, srv=one, atoms=one, counts=one, out=one, fit=one, info=one, work=one):
        return lib.prc_echo_cancel(ctypes.byref(d), ref, srv, atoms, counts, out, fit, info, work, None)

    assert ws(_desc()) == _lib.PRC_OK and nb.value > 0 and nb.value % 16 == 0
    for kw in (dict(nframes=1, frame_stride=0, out_stride=0), dict(max_atoms=32, refine=8), dict(ramp=0, refine=0),
               dict(n=1), dict(sample_rate=-48000.0), dict(reg=1e3), dict(wrap=1), dict(nframes=65535)):
        assert ws(_desc(**kw)) == _lib.PRC_OK, kw
    for kw in BAD:
        assert ws(_desc(**kw)) == _lib.PRC_EINVAL, kw
        assert run(_desc(**kw)) == _lib.PRC_EINVAL, kw
    for kw in (dict(n=2 ** 31), dict(nframes=65536, frame_stride=2 ** 31)):
        assert ws(_desc(**kw)) == _lib.PRC_ESHAPE, kw
    assert lib.prc_echo_cancel_workspace_bytes(None, ctypes.byref(nb)) == _lib.PRC_EINVAL
    assert lib.prc_echo_cancel_workspace_bytes(ctypes.byref(_desc()), None) == _lib.PRC_EINVAL
    for missing in ("ref", "srv", "atoms", "counts", "out", "fit", "info", "work"):
        assert run(_desc(), **{missing: None}) == _lib.PRC_EINVAL, missing
    assert run(_desc(), work=ctypes.c_void_p(24)) == _lib.PRC_EINVAL and "aligned" in lib.prc_last_error().decode()
    # a larger stack or more atoms never needs less
    sizes = []
    for kw in (dict(), dict(max_atoms=32), dict(nframes=3), dict(ramp=0, refine=0)):
        assert ws(_desc(**kw)) == _lib.PRC_OK
        sizes.append(nb.value)
    assert sizes[1] > sizes[0] and sizes[2] > sizes[0] and sizes[3] < sizes[0]


def test_python_argument_errors_need_no_device():
    """ValueError from the host, before a device is touched: engine.echo_desc, cancel_echoes and clean_xambg"""
    from passiveradar_amd import engine
    from passiveradar_amd.clutter_removal import cancel_echoes
    from passiveradar_amd.range_doppler_processing import clean_xambg
    for kw in (dict(max_atoms=0), dict(max_atoms=33), dict(refine=9), dict(refine=-1), dict(ramp=False), dict(reg=-1.0),
               dict(reg=float("nan")), dict(nframes=2, frame_stride=10), dict(nframes=0), dict(n=0), dict(sample_rate=0.0)):
        args = dict(n=100, sample_rate=1.0, max_atoms=2)
        args.update(kw)
        with pytest.raises(ValueError):
            engine.echo_desc(**args)
    x = np.ones(100, np.complex64)
    bad = [((x, x[:50], 1.0, [1], [0.0]), {}), ((x, x, 1.0, [1, 2], [0.0]), {}), ((x, x, 1.0, [1.5], [0.0]), {}),
           ((x, x, 1.0, [100], [0.0]), {}), ((x, x, 1.0, [-100], [0.0]), {}), ((x, x, 1.0, [1], [np.nan]), {}),
           ((x, x, 1.0, [1], [np.inf]), {}), ((x, x, 1.0, list(range(33)), [0.0] * 33), {}),
           ((x, x, 1.0, [1], [0.0]), dict(ramp=False)), ((x, x, 1.0, [1], [0.0]), dict(refine=9)),
           ((x, x, 1.0, [1], [0.0]), dict(reg=-1.0)), ((x, x, 0.0, [1], [0.0]), {}),
           ((np.ones((2, 100), np.complex64),) * 2 + (1.0, [1], [0.0]), {}),
           ((np.ones((2, 2, 50), np.complex64),) * 2 + (1.0, [1], [0.0]), {})]
    for args, kw in bad:
        with pytest.raises(ValueError):
            cancel_echoes(*args, **kw)
    assert cancel_echoes(x, x, 1.0, [], []) is x                      # an empty list returns srvChannel
    s = np.ones((2, 100), np.complex64)
    assert cancel_echoes(s, s, 1.0, [[], []], [[], []]) is s
    for kw in (dict(npeaks=-1), dict(lag_span=-1), dict(oversample=0), dict(patch=(2, 16)), dict(npeaks=11, lag_span=1)):
        with pytest.raises(ValueError):
            clean_xambg(x, x, 1.0, 8, 10, **kw)
    with pytest.raises(ValueError):
        clean_xambg(s, s, 1.0, 8, 10)
