"""Map fusion without a GPU: the ABI layout, the argument checks (host arithmetic), bistatic_axes / bistatic_cell, and the
design scene on the oracle alone (tests/fuse_oracle.py): exact statements, not tolerances."""
import ctypes

import numpy as np
import pytest

import fuse_oracle as FO

INF, NAN = float("inf"), float("nan")


def test_descriptor_matches_the_header(tmp_path):
    """sizeof / offsetof of prc_fuse_desc as gcc lays it out == the ctypes mirror; the constants agree; the symbol is declared,
    exported and bound"""
    import shutil
    import subprocess
    from conftest import REPO
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [n for n, _ in _lib.FuseDesc._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(prc_fuse_desc, {n}));\n' for n in fields)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_fuse_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %u %u %d %d %d %d %d %d %d %d %d %d\\n", sizeof(prc_fuse_desc), PRC_FUSE_DESC_SIZE_MIN, d.struct_size,\n'
                   '         PRC_FUSE_MAX_ILLUM, PRC_FUSE_MAX_ILLUM, PRC_FUSE_ILLUM_DOUBLES, PRC_FUSE_LDS_BYTES, (int)PRC_FUSE_SUM,\n'
                   '         (int)PRC_FUSE_MIN, (int)PRC_FUSE_FORM_AUTO, (int)PRC_FUSE_FORM_GLOBAL, (int)PRC_FUSE_FORM_LDS, PRC_VERSION);\n'
                   + body + '  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    D = _lib.FuseDesc
    assert [int(v) for v in lines[0].split()] == [ctypes.sizeof(D), ctypes.sizeof(D), ctypes.sizeof(D), _lib.FUSE_MAX_ILLUM,
                                                  _lib.CAF_MAX_REFS, _lib.FUSE_ILLUM_DOUBLES, _lib.FUSE_LDS_BYTES, _lib.FUSE_SUM,
                                                  _lib.FUSE_MIN, _lib.FUSE_FORM_AUTO, _lib.FUSE_FORM_GLOBAL, _lib.FUSE_FORM_LDS,
                                                  _lib.MIN_LIB_VERSION]
    assert [int(v) for v in lines[1:]] == [getattr(D, n).offset for n in fields]
    assert _lib.FUSE_LDS_BYTES <= 160 * 1024 and _lib.FUSE_MAX_ILLUM == 8
    assert not any(t is ctypes.c_int64 for _, t in D._fields_)             # the 64-bit quantities are function parameters
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert "prc_fuse" in _lib.EXPORTED_SYMBOLS and hasattr(handle, "prc_fuse")
    assert _lib.lib().prc_fuse.argtypes[3] is ctypes.c_int64 and _lib.lib().prc_fuse.argtypes[4] is ctypes.c_int64


def _call(nframes=0, stat=None, best=None, vel=None, illum="design", illum_stride=None, frame_stride=None, mutate=None, **kw):
    from passiveradar_amd import _lib, engine
    K = kw.pop("nillum", 3)
    H, W = kw.pop("H", FO.H), kw.pop("W", FO.W)
    grid, vels = list(FO.GRID), list(FO.VELS)
    for name, (lst, i) in dict(x0=(grid, 0), dx=(grid, 1), nx=(grid, 2), y0=(grid, 3), dy=(grid, 4), ny=(grid, 5), vx0=(vels, 0),
                               dvx=(vels, 1), nvx=(vels, 2), vy0=(vels, 3), dvy=(vels, 4), nvy=(vels, 5)).items():
        if name in kw:
            lst[i] = kw.pop(name)
    d = engine.fuse_desc(K, H, W, grid, vels, kw.pop("rx", FO.RX), kw.pop("z", FO.Z), kw.pop("combine", 0), kw.pop("form", None))
    assert not kw, kw
    if mutate:
        mutate(d)
    if isinstance(illum, str):
        rows = FO.illum_rows(FO.design_illuminators(), FO.RX)
        illum = np.concatenate([rows] * 3)[:max(K, 1)].copy()
    ip = None if illum is None else np.ascontiguousarray(illum, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    HW = H * W
    illum_stride = max(nframes, 1) * HW if illum_stride is None else illum_stride
    frame_stride = HW if frame_stride is None else frame_stride
    return _lib.lib().prc_fuse(ctypes.byref(d), ip, stat, illum_stride, frame_stride, nframes, best, vel, None)


def test_c_abi_argument_errors_need_no_device():
    """every PRC_EINVAL of prc_fuse from host arithmetic; nframes == 0 is a no-op"""
    from passiveradar_amd import _lib
    one = ctypes.c_void_p(8)          # a non-null pointer nothing dereferences: every case below fails or returns before a launch
    OK, BAD = _lib.PRC_OK, _lib.PRC_EINVAL
    assert _call() == OK
    assert _call(nillum=1) == OK and _call(nillum=8) == OK and _call(combine=1, form=2) == OK and _call(form=1) == OK
    assert _call(H=1, W=1, nx=1, ny=1, nvx=1, nvy=1) == OK
    # shapes < 1, too many illuminators, products above 2^31 - 1
    for kw in (dict(nillum=0), dict(nillum=9), dict(nillum=-1), dict(H=0), dict(W=0), dict(H=-4), dict(nx=0), dict(ny=0), dict(nx=-1),
               dict(nvx=0), dict(nvy=0), dict(nvy=-2), dict(nvx=65536, nvy=32768), dict(nvx=2**31 - 1, nvy=2),
               dict(H=65536, W=32768), dict(nx=65536, ny=32768), dict(nx=2**31 - 1, ny=1)):
        assert _call(**kw) == BAD, kw
    assert _call(nvx=2**31 - 1, nvy=1) == OK and _call(nvx=46340, nvy=46340) == OK
    # an unknown combine or form
    for kw in (dict(combine=2), dict(combine=-1), dict(form=3), dict(form=-1)):
        assert _call(**kw) == BAD, kw
    # a non-finite grid, velocity or receiver parameter
    for name in ("x0", "dx", "y0", "dy", "z", "vx0", "dvx", "vy0", "dvy"):
        for v in (NAN, INF, -INF):
            assert _call(**{name: v}) == BAD, (name, v)
    for i in range(3):
        rx = list(FO.RX)
        rx[i] = NAN
        assert _call(rx=rx) == BAD
    assert _call(dx=0.0, dy=-3.0, dvx=0.0, dvy=-1.0) == OK                 # finite is all the grid has to be
    # a non-finite illuminator parameter, a wavelength <= 0 -- in any row that counts, and only there
    rows = FO.illum_rows(FO.design_illuminators(), FO.RX)
    for k in range(3):
        for i in range(9):
            for v in (NAN, INF):
                bad = rows.copy()
                bad[k, i] = v
                assert _call(illum=bad) == BAD, (k, i, v)
                assert _call(illum=bad, nillum=k) == (OK if k else BAD)   # row k is not read with k illuminators (k = 0: refused)
        for v in (0.0, -3.0):
            bad = rows.copy()
            bad[k, 3] = v
            assert _call(illum=bad) == BAD, (k, v)
    assert _call(illum=None) == BAD
    # nframes, null pointers with work to do
    assert _call(nframes=-1) == BAD
    assert _call(nframes=2) == BAD and _call(nframes=2, stat=one) == BAD and _call(nframes=2, best=one) == BAD
    assert _call(nframes=2, vel=one) == BAD
    # strides that let maps overlap
    HW = FO.H * FO.W
    for kw in (dict(illum_stride=HW - 1), dict(illum_stride=0), dict(illum_stride=-HW), dict(nframes=2, frame_stride=HW - 1, stat=one, best=one),
               dict(nframes=2, frame_stride=0, stat=one, best=one), dict(nframes=2, frame_stride=-HW, stat=one, best=one),
               dict(nframes=2, illum_stride=HW, frame_stride=HW, stat=one, best=one),             # frame 1 of k is frame 0 of k + 1
               dict(nframes=2, illum_stride=2 * HW - 1, frame_stride=HW, stat=one, best=one),
               dict(nframes=2, illum_stride=HW, frame_stride=3 * HW - 1, stat=one, best=one),
               dict(nframes=3, illum_stride=HW + 5, frame_stride=2 * HW, stat=one, best=one)):
        assert _call(**kw) == BAD, kw
    assert _call(nillum=1, illum_stride=0) == OK and _call(nillum=1, illum_stride=-7) == OK     # one illuminator: the stride is not looked at
    assert _call(nframes=0, frame_stride=0) == OK                                               # no second frame either
    assert _call(illum_stride=HW) == OK and _call(illum_stride=2**40) == OK
    # the descriptor header
    assert _lib.lib().prc_fuse(None, None, None, 0, 0, 0, None, None, None) == BAD
    assert _call(mutate=lambda d: setattr(d, "struct_size", 36)) == BAD
    assert _call(mutate=lambda d: setattr(d, "magic", 0)) == BAD


def test_python_argument_errors_need_no_device():
    from passiveradar_amd.target_detection import fuse_maps, locate_maps
    stat = np.zeros((3, 1, FO.H, FO.W), np.float32)
    il = FO.design_illuminators()
    with pytest.raises(ValueError):
        fuse_maps(stat, il, FO.RX, FO.GRID, FO.VELS, combine="max")
    with pytest.raises(ValueError):
        fuse_maps(stat[:2], il, FO.RX, FO.GRID, FO.VELS)
    with pytest.raises(ValueError):
        fuse_maps(stat[0], il, FO.RX, FO.GRID, FO.VELS)
    with pytest.raises(ValueError):
        fuse_maps(stat, il, FO.RX, FO.GRID[:5], FO.VELS)
    with pytest.raises(ValueError):
        fuse_maps(stat, il, FO.RX, FO.GRID, FO.VELS, form=7)
    with pytest.raises(ValueError):
        fuse_maps(stat, [(FO.TXS[0], 0.0, FO.AXES)] + il[1:], FO.RX, FO.GRID, FO.VELS)
    with pytest.raises(ValueError):
        fuse_maps(stat, il, FO.RX, (NAN,) + FO.GRID[1:], FO.VELS)
    best, vel = fuse_maps(stat[:, :0], il, FO.RX, FO.GRID, FO.VELS)
    assert best.shape == (0, 13, 17) and vel.shape == (0, 13, 17) and best.dtype == np.float32 and vel.dtype == np.int32
    x = np.ones((FO.H, FO.W, 2), np.complex64)
    with pytest.raises(ValueError):
        locate_maps([x, x, x], il, FO.RX, FO.GRID, FO.VELS, FO.Z, thresh=1.0, npeaks=0)
    with pytest.raises(ValueError):
        locate_maps([x, x], il, FO.RX, FO.GRID, FO.VELS, FO.Z, thresh=1.0, npeaks=2)
    with pytest.raises(ValueError):
        locate_maps([x, x, x], il, FO.RX, FO.GRID, FO.VELS, FO.Z, thresh=1.0, npeaks=2, cfar="median")


@pytest.mark.parametrize("delay,doppler", [(0, 0.0), (5, 100.0), (17, -140.0), (40, 260.0), (63, -300.0)])
def test_bistatic_axes_invert_expected_peak_cell(delay, doppler):
    """an echo delay samples late (delay c / fs metres of excess range) at doppler Hz: the axes put it where fast_xambg does"""
    from passiveradar_amd import scene
    from passiveradar_amd.target_detection import bistatic_axes
    col0, col_per_m, row0, row_per_hz = bistatic_axes(FO.R, FO.F, FO.N, FO.FS)
    assert (col0, col_per_m, row0, row_per_hz) == FO.AXES
    row, col = scene.expected_peak_cell(delay, doppler, FO.N, FO.FS, FO.R, FO.F)
    assert int(np.rint(col0 + (delay * FO.C0 / FO.FS) * col_per_m)) == col
    assert int(np.rint(row0 + doppler * row_per_hz)) % FO.F == row


def test_bistatic_cell_is_the_oracle_forward_model():
    from passiveradar_amd.target_detection import bistatic_cell
    rows = FO.illum_rows(FO.design_illuminators(), FO.RX)
    for pos, v in (FO.TARGET_A, FO.TARGET_B, ((0.0, 0.0, 10.0), (30.0, -40.0)), (FO.TXS[1], (1.0, 2.0))):
        for k, tx in enumerate(FO.TXS):
            assert bistatic_cell(pos, v, tx, FO.RX, FO.LAM, FO.AXES) == FO.cell_of(pos, v, rows[k], FO.RX)
    # closing on both ends of the path: positive Doppler, a row above the centre (row_per_hz < 0); a longer path: a lower column
    # (transmitter 0 and the receiver both lie towards -x of the target)
    r_in, c_in = bistatic_cell((6000.0, 4000.0, 3000.0), (-150.0, 0.0), FO.TXS[0], FO.RX, FO.LAM, FO.AXES)
    r_out, _ = bistatic_cell((6000.0, 4000.0, 3000.0), (150.0, 0.0), FO.TXS[0], FO.RX, FO.LAM, FO.AXES)
    assert r_in < FO.F / 2 < r_out
    _, c_far = bistatic_cell((12000.0, 8000.0, 3000.0), (0.0, 0.0), FO.TXS[0], FO.RX, FO.LAM, FO.AXES)
    assert c_far < c_in


def _design(targets, combine):
    stat = FO.design_maps(targets)
    return FO.fuse(stat, FO.illum_rows(FO.design_illuminators(), FO.RX), FO.RX, FO.GRID, FO.VELS, FO.Z, combine)


def test_oracle_design_scene_one_target():
    """A alone, sum: best is 3.0 at (8, 11) only, vel = 25 there; no other cell reaches 2.0"""
    best, vel = _design([FO.TARGET_A], FO.SUM)
    assert best.shape == (1, 13, 17) and best.dtype == np.float32 and vel.dtype == np.int32
    assert np.argwhere(best[0] == 3.0).tolist() == [list(FO.CELL_A)] and vel[0][FO.CELL_A] == FO.VEL_A
    rest = best[0].copy()
    rest[FO.CELL_A] = 0.0
    assert rest.max() < 2.0


def test_oracle_design_scene_two_targets_sum():
    """A and B, sum: 3.0 at exactly (8, 11) and (3, 4), vel 25 and 75; one ghost cell at 2.0"""
    best, vel = _design([FO.TARGET_A, FO.TARGET_B], FO.SUM)
    assert np.argwhere(best[0] == 3.0).tolist() == [list(FO.CELL_B), list(FO.CELL_A)]
    assert vel[0][FO.CELL_A] == FO.VEL_A and vel[0][FO.CELL_B] == FO.VEL_B
    assert int((best[0] == 2.0).sum()) == 1 and int((best[0] > 2.0).sum()) == 2


def test_oracle_design_scene_two_targets_min():
    """A and B, min: 1.0 at exactly those two cells and 0 everywhere else"""
    best, vel = _design([FO.TARGET_A, FO.TARGET_B], FO.MIN)
    assert np.argwhere(best[0] == 1.0).tolist() == [list(FO.CELL_B), list(FO.CELL_A)]
    assert vel[0][FO.CELL_A] == FO.VEL_A and vel[0][FO.CELL_B] == FO.VEL_B
    rest = best[0].copy()
    rest[FO.CELL_A] = rest[FO.CELL_B] = 0.0
    assert (rest == 0.0).all()


def test_oracle_ties_nan_and_inf():
    """ties go to the lowest j; a NaN is never chosen; +Inf is; a cell whose every hypothesis is NaN keeps (-Inf, -1)"""
    il = [((-5000.0, 0.0, 100.0), 3.0, FO.AXES)]
    rows = FO.illum_rows(il, FO.RX)
    grid, vels = (1000.0, 500.0, 3, 2000.0, 500.0, 2), (-100.0, 100.0, 3, -100.0, 100.0, 3)
    stat = np.ones((1, 1, FO.H, FO.W), np.float32)
    best, vel = FO.fuse(stat, rows, FO.RX, grid, vels, 500.0)
    assert (best == 1.0).all() and (vel == 0).all()
    r, c = FO.cells(rows, FO.RX, grid, vels, 500.0)
    stat[0, 0, int(r[0, 0, 0, 0]), int(c[0, 0, 0])] = NAN                   # hypothesis 0 of cell (0, 0)
    best, vel = FO.fuse(stat, rows, FO.RX, grid, vels, 500.0)
    assert best[0, 0, 0] == 1.0 and vel[0, 0, 0] > 0
    stat[0, 0, int(r[0, 1, 2, 4]), int(c[0, 1, 2])] = INF
    best, vel = FO.fuse(stat, rows, FO.RX, grid, vels, 500.0)
    assert best[0, 1, 2] == INF and vel[0, 1, 2] <= 4
    stat[:] = NAN
    best, vel = FO.fuse(stat, rows, FO.RX, grid, vels, 500.0)
    assert (best == -INF).all() and (vel == -1).all()
