"""Exact ambiguity patches, the part that needs no GPU: the float64 oracle (tests/xambg_patch_oracle.py) against the
reference-made direct_xambg golden and a closed form, the cell -> origin mapping, the droop of fast_xambg's boxcar
decimator that the patches exist to avoid, the struct layouts, and the argument checks that are host arithmetic."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import xambg_patch_oracle as PO
from conftest import REPO, load_golden, rel_err
from oracle import np_oracle as O
from passiveradar_amd import _lib, engine, scene
from passiveradar_amd.range_doppler_processing import patch_origins, xambg_patch
from passiveradar_amd.target_detection import refine_peaks


def direct_surface_args(n, R, F, fs):
    """the patch that is direct_xambg's surface: (lag0, doppler0, nlags, ndoppler, step); columns come out reversed"""
    cpi = n / fs
    return 0, -0.5 * F / cpi, R + 1, F, 1.0 / cpi


def test_oracle_against_the_reference_made_direct_xambg_golden():
    """wrap=False, no window, doppler0 = -F/2/CPI, step 1/CPI, nlags = R+1, ndoppler = F, columns reversed, is the
    reference's direct_xambg (its float32 phase ramp is what separates them): 2e-6 of the peak, the bar of the small goldens"""
    g = load_golden("direct_xambg")
    for t in "ab":
        ref, srv, R, F, fs = g[f"ref_{t}"], g[f"srv_{t}"], int(g[f"R_{t}"]), int(g[f"F_{t}"]), float(g[f"fs_{t}"])
        lag0, dop0, nl, nd, step = direct_surface_args(ref.shape[0], R, F, fs)
        X = PO.patch(ref, srv, fs, lag0, dop0, nl, nd, step, None, wrap=False)[:, ::-1]
        err = rel_err(X, g[f"out_{t}"][:, :, 0])
        print(f"direct_xambg golden {t}: {err:.3g}")
        assert err < 2e-6


@pytest.mark.parametrize("window", [None, "kaiser"])
def test_oracle_closed_form(window):
    """srv = roll(ref, D) exp(j 2 pi f i / Fs) with f n / Fs an integer and wrap: X(D, f) = exp(-j 2 pi f D / Fs) sum w |ref|^2"""
    n, fs, D, f = 4099, 4099.0, 7, 5.0
    ref = scene.white_reference(n, 5).astype(np.complex128)
    srv = np.roll(ref, D) * np.exp(2j * np.pi * f * np.arange(n) / fs)
    w = None if window is None else np.kaiser(n, 5.0)
    X = PO.patch(ref, srv, fs, D - 1, f - 2.0, 3, 5, 1.0, w, wrap=True)
    want = np.exp(-2j * np.pi * f * D / fs) * np.sum((1.0 if w is None else w) * np.abs(ref) ** 2)
    assert abs(X[2, 1] - want) <= 1e-12 * abs(want)
    assert np.unravel_index(np.argmax(np.abs(X)), X.shape) == (2, 1)


def test_patch_origins_agree_with_expected_peak_cell():
    n, fs, R, F = 65536, 65536.0, 16, 64
    for delay, fd in ((5, 3.0), (0, -30.0), (16, 31.0), (9, 0.0), (3, -1.0)):
        row, col = scene.expected_peak_cell(delay, fd, n, fs, R, F)
        for nl, nd, step in ((1, 1, 1.0), (3, 17, 0.25), (16, 16, 0.5)):
            lags, dops = patch_origins([row], [col], R, F, n, fs, nl, nd, step)
            assert lags[0] + nl // 2 == delay
            assert dops[0] + (nd // 2) * step == pytest.approx(fd, abs=1e-12)
    lags, dops = patch_origins([1, 2], [3, 4], R, F, n, fs, 4, 4, 1.0)
    assert lags.tolist() == [R - 3 - 2, R - 4 - 2] and dops.tolist() == [F / 2 - 1 - 2, F / 2 - 2 - 2]


DROOP_SCENE = dict(n=65536, fs=65536.0, R=16, F=64, seed=779, delay=5)


@pytest.mark.parametrize("fd", [3.3, 28.3, -30.6])
def test_fast_xambg_droop_is_the_dirichlet_gain(fd):
    """the boxcar decimator of q + 1 = 1025 taps leaves |sin(pi f 1025 / Fs) / (1025 sin(pi f / Fs))| of an echo at f: the
    fast_xambg oracle's peak over the exact (patch oracle) value at that cell.  Within 0.02 (aliasing and the window)."""
    s = DROOP_SCENE
    ref, srv = scene.make_scene(s["n"], s["fs"], s["R"], s["seed"], targets=((s["delay"], fd, 1.0),), clutter=())
    w = np.kaiser(s["n"], 5.0)
    A = np.abs(O.fast_xambg(ref, srv, s["R"], s["F"], s["n"], w)[:, :, 0])
    row, col = np.unravel_index(np.argmax(A), A.shape)
    assert (row, col) == scene.expected_peak_cell(s["delay"], fd, s["n"], s["fs"], s["R"], s["F"])
    lags, dops = patch_origins([row], [col], s["R"], s["F"], s["n"], s["fs"], 1, 1, 1.0)
    exact = abs(PO.patch(ref, srv, s["fs"], lags[0], dops[0], 1, 1, 1.0, w, wrap=True)[0, 0])
    ratio, gain = A[row, col] / exact, PO.dirichlet_gain(fd, s["fs"], s["n"] // s["F"] + 1)
    print(f"fd {fd}: fast_xambg / exact {ratio:.4f}, closed form {gain:.4f}")
    assert abs(ratio - gain) <= 0.02


def test_oracle_refinement_recovers_the_doppler():
    """a 3-point parabola over a patch of 0.25 Hz spacing finds the echo's Doppler well inside the 1 Hz cell"""
    s = DROOP_SCENE
    for fd in (3.3, 28.3, -30.6):
        ref, srv = scene.make_scene(s["n"], s["fs"], s["R"], s["seed"], targets=((s["delay"], fd, 1.0),), clutter=())
        lag0, dop0 = s["delay"] - 1, round(fd) - 2.0
        X = PO.patch(ref, srv, s["fs"], lag0, dop0, 3, 17, 0.25, np.kaiser(s["n"], 5.0)).astype(np.complex64)
        pk = PO.refine(X[None], [lag0], [dop0], 0.25)[0]
        assert pk["l"] == 1 and pk["flags"] == 0 and abs(pk["doppler"] - fd) <= 0.005


def test_oracle_refinement_edges_and_flat():
    X = np.zeros((4, 5, 4), np.complex64)
    X[0, 2, 1], X[0, 1, 1], X[0, 3, 1], X[0, 2, 0], X[0, 2, 2] = 4, 2, 3, 1, 1     # interior
    X[1, 0, 2] = 1j                                                                # Doppler edge
    X[2, 3, 3] = -2                                                                # lag edge
    X[2, 3, 2] = 2                                                                 # an equal cell earlier in [d][l] order wins
    pk = PO.refine(X, [10, 20, 30, 40], [1.0, 2.0, 3.0, 4.0], 0.5)
    assert pk["flags"].tolist() == [0, PO.EDGE_DOPPLER, 0, PO.FLAT | PO.EDGE_DOPPLER | PO.EDGE_LAG]
    assert (pk["d"].tolist(), pk["l"].tolist()) == ([2, 0, 3, 0], [1, 2, 2, 0])
    assert pk["doppler"][0] == 1.0 + (2 + 0.5 * (2 - 3) / (2 - 8 + 3)) * 0.5 and pk["lag"][0] == 11.0
    assert pk["doppler"][1] == 2.0 and pk["lag"][3] == 40.0 and pk["doppler"][3] == 4.0
    assert pk["lag"][2] == 30 + 2 + 0.5 and pk["amplitude"].tolist() == [4.0, 1.0, 2.0, 0.0]
    assert np.all(np.isfinite(pk["lag"])) and np.all(np.isfinite(pk["doppler"]))


def test_patch_structs_match_the_header(tmp_path):
    """sizeof / offsetof of prc_patch_desc, prc_patch and prc_patch_peak as gcc lays them out == the ctypes and NumPy mirrors"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = {"prc_patch_desc": (_lib.PatchDesc, None), "prc_patch": (_lib.Patch, _lib.PATCH_DTYPE),
              "prc_patch_peak": (_lib.PatchPeak, _lib.PATCH_PEAK_DTYPE)}
    lines = []
    for name, (cls, _) in fields.items():
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f}));' for f, _t in cls._fields_]
        lines.append('  printf("\\n");')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n' + "\n".join(lines) +
                   '\n  prc_patch_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%u %u %u %d %d %d\\n", PRC_PATCH_DESC_SIZE_680, d.struct_size, d.magic, PRC_VERSION, PRC_PATCH_MAX_LAGS,\n'
                   '         PRC_PATCH_MAX_DOPPLER);\n  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", REPO, str(src), "-o", str(exe)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    for row, (name, (cls, dtype)) in zip(rows, fields.items()):
        assert row == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _t in cls._fields_], name
        if dtype is not None:
            assert dtype.itemsize == row[0] and [dtype.fields[f][1] for f, _t in cls._fields_] == row[1:], name
    assert PO.PEAK_DTYPE == _lib.PATCH_PEAK_DTYPE
    size = ctypes.sizeof(_lib.PatchDesc)
    assert rows[3] == [size, size, _lib.DESC_MAGIC, _lib.MIN_LIB_VERSION, _lib.PATCH_MAX_LAGS, _lib.PATCH_MAX_DOPPLER]
    assert _lib.MIN_LIB_VERSION == 680 and _lib.lib().prc_version() == 680
    assert ctypes.sizeof(_lib.Patch) == 16 and ctypes.sizeof(_lib.PatchPeak) == 32


def test_workspace_bytes_and_descriptor_checks_need_no_device():
    """prc_xambg_patch_workspace_bytes is host arithmetic: it grows with the patch count and refuses every bad descriptor"""
    good = dict(n=6001, nlags=16, ndoppler=16, sample_rate=6001.0, doppler_step=0.25)
    b1 = engine.xambg_patch_workspace_bytes(engine.patch_desc(**good), 1)
    assert b1 >= 16 * 16 * 16 and engine.xambg_patch_workspace_bytes(engine.patch_desc(**good), 7) == 7 * b1
    for bad in (dict(n=0), dict(nlags=0), dict(nlags=1025), dict(ndoppler=0), dict(ndoppler=4097), dict(sample_rate=float("nan")),
                dict(sample_rate=float("inf")), dict(sample_rate=0.0), dict(doppler_step=float("inf")),
                dict(doppler_step=float("nan")), dict(nframes=0), dict(nframes=2, frame_stride=6000)):
        with pytest.raises(ValueError):
            engine.xambg_patch_workspace_bytes(engine.patch_desc(**{**good, **bad}), 1)
    d = engine.patch_desc(**good)
    d.wrap = 2
    with pytest.raises(ValueError):
        engine.xambg_patch_workspace_bytes(d, 1)
    with pytest.raises(ValueError):
        engine.xambg_patch_workspace_bytes(engine.patch_desc(**good), -1)
    for size, magic in ((48, _lib.DESC_MAGIC), (58, _lib.DESC_MAGIC), (56, 0)):
        d = engine.patch_desc(**good)
        d.struct_size, d.magic = size, magic
        with pytest.raises(ValueError):
            engine.xambg_patch_workspace_bytes(d, 1)
    # null pointers are refused before a device is touched
    L, nb = _lib.lib(), ctypes.c_size_t(0)
    d = engine.patch_desc(**good)
    assert L.prc_xambg_patch_workspace_bytes(None, 1, ctypes.byref(nb)) == _lib.PRC_EINVAL
    assert L.prc_xambg_patch_workspace_bytes(ctypes.byref(d), 1, None) == _lib.PRC_EINVAL
    assert L.prc_xambg_patch(ctypes.byref(d), None, None, None, None, 1, None, None, None) == _lib.PRC_EINVAL
    assert L.prc_xambg_patch_peaks(ctypes.byref(d), None, 1, None, None, None) == _lib.PRC_EINVAL
    assert b"null pointer" in L.prc_last_error()


def test_host_built_patch_lists_are_validated():
    x = np.ones(64, np.complex64)
    with pytest.raises(ValueError, match="same length"):
        xambg_patch(x, x[:-1], 64.0, [0], [0.0])
    for kw in (dict(lags=[64]), dict(lags=[-64]), dict(dopplers=[float("nan")]), dict(frame=[1]), dict(frame=[-1]),
               dict(lags=[0, 1]), dict(lags=[0.5])):
        args = {**dict(lags=[0], dopplers=[0.0]), **kw}
        with pytest.raises(ValueError):
            xambg_patch(x, x, 64.0, args["lags"], args["dopplers"], frame=args.get("frame"))
    with pytest.raises(ValueError):
        xambg_patch(x, x, 64.0, [0], [0.0], window=np.ones(63, np.float32))
    with pytest.raises(ValueError):
        xambg_patch(x, x, 64.0, [0], [0.0], nlags=1025)
    with pytest.raises(ValueError):
        refine_peaks(np.zeros((2, 3, 3), np.complex64), [0], [0.0], 1.0)
    rec = engine.patch_list([3, -2], [1.5, 2.5], [1, 0], nframes=2, n=16)
    assert rec.dtype == _lib.PATCH_DTYPE and rec.tolist() == [(1, 3, 1.5), (0, -2, 2.5)]
    assert xambg_patch(x, x, 64.0, [], []).shape == (0, 16, 16)


def test_no_cpu_fallback_for_patches():
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    x = np.ones(64, np.complex64)
    with pytest.raises(_lib.PrcoreError):
        xambg_patch(x, x, 64.0, [0], [0.0])
    with pytest.raises(_lib.PrcoreError):
        refine_peaks(np.zeros((1, 3, 3), np.complex64), [0], [0.0], 1.0)
