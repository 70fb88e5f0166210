"""Track-before-detect without a GPU: the ABI layout, the argument checks (host arithmetic), tbd_row_shifts, properties of the
oracle (tests/tbd_oracle.py) and the scene the feature exists for, on the oracle alone."""
import ctypes

import numpy as np
import pytest

import tbd_oracle as TO

INF = float("inf")


def test_descriptor_matches_the_header(tmp_path):
    """sizeof / offsetof of prc_tbd_desc as gcc lays it out == the ctypes mirror; the constants agree; both symbols are
    declared and exported"""
    import shutil
    import subprocess
    from conftest import REPO
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [n for n, _ in _lib.TbdDesc._fields_]
    body = "".join(f'  printf("%zu\\n", offsetof(prc_tbd_desc, {n}));\n' for n in fields)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_tbd_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %u %u %d %d %d %d %d %d\\n", sizeof(prc_tbd_desc), PRC_TBD_DESC_SIZE_MIN, d.struct_size,\n'
                   '         PRC_TBD_FRAMES, PRC_TBD_FRAMES_MAX, PRC_TBD_LDS_BYTES, (int)PRC_OPT_TBD_FRAMES, (int)PRC_OPT_TBD_ROWS,\n'
                   '         PRC_VERSION);\n' + body + '  return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    D = _lib.TbdDesc
    assert [int(v) for v in lines[0].split()] == [ctypes.sizeof(D), ctypes.sizeof(D), ctypes.sizeof(D), _lib.TBD_FRAMES,
                                                  _lib.TBD_FRAMES_MAX, _lib.TBD_LDS_BYTES, _lib.OPT_TBD_FRAMES, _lib.OPT_TBD_ROWS,
                                                  _lib.MIN_LIB_VERSION]
    assert [int(v) for v in lines[1:]] == [getattr(D, n).offset for n in fields]
    assert 2 <= _lib.TBD_FRAMES <= _lib.TBD_FRAMES_MAX and _lib.TBD_LDS_BYTES <= 160 * 1024
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("prc_tbd", "prc_tbd_trace"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(handle, sym)


def test_c_abi_argument_errors_need_no_device():
    """PRC_EINVAL / PRC_ESHAPE from host arithmetic; nframes == 0 and nends == 0 are no-ops"""
    from passiveradar_amd import _lib, engine
    lib = _lib.lib()
    one = ctypes.c_void_p(8)          # a non-null pointer nothing dereferences: every case below fails or returns before a launch

    def run(nframes=0, stat=None, score=None, **kw):
        d = engine.tbd_desc(kw.pop("H", 24), kw.pop("W", 40), **kw)
        return lib.prc_tbd(ctypes.byref(d), stat, None, None, nframes, score, None, None)

    def trace(nframes=3, nends=0, depth=4, back=None, ends=None, paths=None, **kw):
        d = engine.tbd_desc(kw.pop("H", 24), kw.pop("W", 40), **kw)
        return lib.prc_tbd_trace(ctypes.byref(d), back, None, nframes, ends, nends, depth, paths, None)

    assert run() == _lib.PRC_OK and trace() == _lib.PRC_OK
    assert run(H=1, W=1) == _lib.PRC_OK and run(alpha=1.0, clip=3.0, doppler_reach=0, range_reach=127) == _lib.PRC_OK
    assert run(doppler_reach=7, range_reach=8) == _lib.PRC_OK                     # 15 x 17 = 255 codes
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768), dict(H=2**31 - 1, W=2)):
        assert run(**kw) == _lib.PRC_ESHAPE, kw
        assert trace(**kw) == _lib.PRC_ESHAPE, kw
    assert run(H=2**31 - 1, W=1) == _lib.PRC_OK
    bad = (dict(doppler_reach=-1), dict(range_reach=-1), dict(range_guard=-1), dict(doppler_guard=-2),
           dict(doppler_reach=8, range_reach=8), dict(doppler_reach=1, range_reach=43), dict(doppler_reach=0, range_reach=128), dict(doppler_reach=2**30, range_reach=2**30),
           dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0000001), dict(alpha=float("nan")), dict(alpha=INF),
           dict(clip=float("nan")))
    for kw in bad:
        assert run(**kw) == _lib.PRC_EINVAL, kw
        assert trace(**kw) == _lib.PRC_EINVAL, kw
    assert run(clip=-INF) == _lib.PRC_OK and run(clip=INF) == _lib.PRC_OK
    assert run(nframes=-1) == _lib.PRC_EINVAL
    assert run(nframes=2) == _lib.PRC_EINVAL and run(nframes=2, stat=one) == _lib.PRC_EINVAL
    assert run(nframes=2, score=one) == _lib.PRC_EINVAL
    assert trace(depth=0) == _lib.PRC_EINVAL and trace(depth=-1) == _lib.PRC_EINVAL
    assert trace(nends=-1) == _lib.PRC_EINVAL and trace(nframes=-1) == _lib.PRC_EINVAL
    assert trace(nends=2) == _lib.PRC_EINVAL
    assert trace(nends=2, back=one, ends=one) == _lib.PRC_EINVAL and trace(nends=2, back=one, paths=one) == _lib.PRC_EINVAL
    assert trace(nends=2, ends=one, paths=one) == _lib.PRC_EINVAL
    d = engine.tbd_desc(24, 40)
    assert lib.prc_tbd(None, None, None, None, 0, None, None, None) == _lib.PRC_EINVAL
    d.struct_size = 36
    assert lib.prc_tbd(ctypes.byref(d), None, None, None, 0, None, None, None) == _lib.PRC_EINVAL
    d = engine.tbd_desc(24, 40)
    d.magic = 0
    assert lib.prc_tbd_trace(ctypes.byref(d), None, None, 0, None, 0, 1, None, None) == _lib.PRC_EINVAL


def test_options_are_range_checked():
    from passiveradar_amd import _lib
    assert _lib.get_option(_lib.OPT_TBD_FRAMES) == 0 and _lib.get_option(_lib.OPT_TBD_ROWS) == 0
    for opt, good, bad in ((_lib.OPT_TBD_FRAMES, _lib.TBD_FRAMES_MAX, _lib.TBD_FRAMES_MAX + 1), (_lib.OPT_TBD_ROWS, 4096, 4097)):
        old = _lib.set_option(opt, good)
        try:
            assert old == 0 and _lib.get_option(opt) == good
            for v in (bad, -1):
                with pytest.raises(ValueError):
                    _lib.set_option(opt, v)
        finally:
            _lib.set_option(opt, 0)


def test_python_argument_errors_need_no_device():
    from passiveradar_amd.target_detection import tbd_maps, tbd_paths, tbd_row_shifts, track_before_detect
    s = np.ones((3, 24, 40), np.float32)
    bad = [dict(alpha=0.0), dict(alpha=1.5), dict(doppler_reach=-1), dict(range_reach=200), dict(clip=float("nan")),
           dict(range_guard=-1), dict(doppler_guard=-1), dict(row_shifts=np.zeros(23, np.int32)),
           dict(row_shifts=np.zeros(24, np.float32)), dict(row_shifts=np.full(24, 2**31, np.int64)),
           dict(prev=np.zeros((24, 41), np.float32))]
    for kw in bad:
        with pytest.raises(ValueError):
            track_before_detect(s, **kw)
    for shape in ((40,), (2, 3, 4, 5)):
        with pytest.raises(ValueError):
            track_before_detect(np.ones(shape, np.float32))
    b = np.zeros((3, 24, 40), np.uint8)
    for args, kw in (((b, [[0, 0]], 0), {}), ((b[0], [[0, 0]], 4), {}), ((b, [0, 0, 0], 4), {}), ((b, [[0, 0]], 4), dict(doppler_reach=-1)),
                     ((b, [[0, 0]], 4), dict(row_shifts=np.zeros(5, np.int32)))):
        with pytest.raises(ValueError):
            tbd_paths(*args, **kw)
    assert tbd_paths(b, np.zeros((0, 2), np.int32), 4).shape == (0, 4)
    for args in ((1, 40, [250.0, 300.0], 0.5, 3.0), (24, 1, [250.0, 300.0], 0.5, 3.0), (24, 40, [250.0, 0.0], 0.5, 3.0),
                 (24, 40, [250.0, 300.0], float("nan"), 3.0), (24, 40, [250.0, 1e-9], 1e6, 3.0)):
        with pytest.raises(ValueError):
            tbd_row_shifts(*args)
    x = np.ones((24, 40, 3), np.complex64)
    with pytest.raises(ValueError):
        tbd_maps(x, [250.0, 300.0], 0.5, 3.0, thresh=5.0, cfar="median")
    with pytest.raises(ValueError):
        tbd_maps(x, [250.0, 300.0], 0.5, 3.0, thresh=5.0, alpha=2.0)
    with pytest.raises(ValueError):
        tbd_maps(x[:, :, 0], [250.0, 300.0], 0.5, 3.0, thresh=5.0)
    with pytest.raises(TypeError):
        tbd_maps(x, [250.0, 300.0], 0.5, 3.0, thresh=5.0, return_back=False)


def test_row_shifts():
    """the formula, by hand at the centre row and at both edges, and its antisymmetry"""
    from passiveradar_amd.target_detection import tbd_row_shifts
    # the issue's geometry: lambda 3 m, 0.5 s hops, 125 m range cells: 250 Hz walks 3 cells a frame
    H, W = 1025, 177
    R = 125.0 * (W - 1) / 1000.0                       # km: one column is 125 m
    s = tbd_row_shifts(H, W, [500.0, R], 0.5, 3.0)
    assert s.dtype == np.int32 and s.shape == (H,)
    assert s[H // 2] == 0                              # 0 Hz
    assert s[0] == 6 and s[H - 1] == -6                # +-500 Hz: 3 * 500 * 0.5 / 125 = 6 cells, closing = w rises
    assert s[256] == 3 and s[768] == -3                # +-250 Hz
    assert np.array_equal(s, -s[::-1])
    for Hh, Ww, ext, dt, lam in ((64, 96, [250.0, 300.0], 0.5, 3.0), (33, 130, [400.0, 20.0], 1.0, 0.6), (2, 2, [1.0, 1.0], 1.0, 1.0)):
        s = tbd_row_shifts(Hh, Ww, ext, dt, lam)
        f = (Hh - 1 - 2 * np.arange(Hh, dtype=np.float64)) * ext[0] / (Hh - 1)
        want = np.rint(lam * f * dt * (Ww - 1) / (1000.0 * ext[1])).astype(np.int32)
        assert np.array_equal(s, want) and np.array_equal(s, -s[::-1])
        # the axis the issue states, D - h 2D/(H-1), is the same Doppler to rounding
        assert np.allclose(f, ext[0] - np.arange(Hh) * 2 * ext[0] / (Hh - 1), rtol=0, atol=1e-12 * ext[0])


def test_oracle_running_sum():
    """qd = qr = 0, zero shifts, alpha = 1, no zones: the running float32 sum per cell"""
    rng = np.random.default_rng(3)
    x = rng.random((6, 5, 7)).astype(np.float32)
    score, back = TO.tbd(x, 0, 0, 1.0, range_guard=0, doppler_guard=0)
    run = np.zeros((5, 7), np.float32)
    for k in range(6):
        run = (run + x[k]).astype(np.float32)
        assert np.array_equal(score[k], run)
    assert (back[0] == TO.NONE).all() and (back[1:] == 0).all()
    # with prev the first frame already has a predecessor
    score2, back2 = TO.tbd(x[1:], 0, 0, 1.0, range_guard=0, doppler_guard=0, prev=score[0])
    assert np.array_equal(score2, score[1:]) and (back2 == 0).all()


@pytest.mark.parametrize("reach", [(1, 1), (2, 3)])
def test_oracle_path_re_adds_to_its_score(reach):
    """alpha = 1: the z' along the path traced from any cell, added oldest first in float32, is that cell's score"""
    rng = np.random.default_rng(5)
    N, H, W = 7, 9, 13
    x = rng.rayleigh(1.0, (N, H, W)).astype(np.float32)
    sh = rng.integers(-3, 4, H).astype(np.int32)
    score, back = TO.tbd(x, *reach, 1.0, clip=2.5, range_guard=1, doppler_guard=1, row_shift=sh)
    z = TO.inputs(x, 2.5, 1, 1)
    ends = [[f, c] for f in range(N) for c in range(H * W)]
    paths = TO.trace(back, ends, N + 2, *reach, sh)
    for (f, c), p in zip(ends, paths):
        p = p[p >= 0]
        acc = np.float32(0.0)
        for j in range(len(p) - 1, -1, -1):
            acc = np.float32(acc + z[f - j].ravel()[p[j]])
        assert acc == score[f].ravel()[c], (f, c)
        # a path ends early only where no predecessor was in bounds
        assert len(p) == f + 1 or back[f - len(p) + 1].ravel()[p[-1]] == TO.NONE


def test_oracle_ties_nan_and_inf():
    x = np.ones((2, 3, 4), np.float32)
    score, back = TO.tbd(x, 1, 1, 0.5, range_guard=0, doppler_guard=0)
    # all ties: the smallest in-bounds code wins: the corner (0, 0) has only dh, dw >= 0: code (0+1)*3 + (0+1) = 4
    assert back[1, 0, 0] == 4 and back[1, 1, 1] == 0 and back[1, 0, 1] == 3 and back[1, 1, 0] == 1
    assert (score[1] == 1.5).all()
    x[0, 1, 1], x[0, 1, 2], x[0, 0, 0] = np.nan, -np.inf, np.inf
    score, back = TO.tbd(x, 1, 1, 0.5, range_guard=0, doppler_guard=0)
    assert np.isnan(score[0, 1, 1]) and not np.isnan(score[1]).any()          # a NaN stays in its cell and is never chosen
    assert score[1, 0, 1] == np.inf and back[1, 0, 1] == 3                     # +Inf is chosen
    assert back[1, 2, 3] == 1 and score[1, 2, 3] == 1.5                        # -Inf (that cell's code 0) is not
    assert back[1, 2, 2] == 2 and score[1, 2, 2] == 1.5                        # codes 0, 1 there are the NaN and the -Inf


ROWS = slice(18, 23)


def scene_shifts(H=64):
    s = np.zeros(H, np.int32)
    s[ROWS] = 2
    return s


@pytest.mark.parametrize("seed", range(20))
def test_seeded_scene(seed):
    """The issue's scene (20 frames of 64 x 96, |unit complex Gaussian|, amplitude 2.5 added at (20, 10 + 2 k), shifts 2 on
    rows 18 .. 22, reach (1, 1), alpha 0.9), evaluated as the issue's model was: without excluded zones (guards 0).  With the
    shifts the integrated score at the target's last cell exceeds the maximum of the noise-only integrated map of the same
    seed; with zero shifts it does not; the path traced from that cell is within one cell of the planted track on at least 15
    of its last 16 frames (the oracle reaches 16 of 16 on every seed).  (With prc_plots' default guards (8, 4) the zero-shift
    case exceeds in seed 12 alone, 17.874 against 17.609: the zones remove the noise cell that holds that map's maximum.)"""
    H, W, N = 64, 96, 20
    x, noise = TO.planted_scene(seed), TO.planted_scene(seed, with_target=False)
    kw = dict(qd=1, qr=1, alpha=0.9, range_guard=0, doppler_guard=0)
    last = (20, 10 + 2 * (N - 1))
    s, back = TO.tbd(x, row_shift=scene_shifts(), **kw)
    sn, _ = TO.tbd(noise, row_shift=scene_shifts(), **kw)
    assert s[N - 1][last] > sn[N - 1].max()
    s0, _ = TO.tbd(x, **kw)
    sn0, _ = TO.tbd(noise, **kw)
    assert not s0[N - 1][last] > sn0[N - 1].max()
    path = TO.trace(back, [[N - 1, last[0] * W + last[1]]], 16, 1, 1, scene_shifts())[0]
    near = sum(1 for j, c in enumerate(path)
               if c >= 0 and abs(c // W - 20) <= 1 and abs(c % W - (10 + 2 * (N - 1 - j))) <= 1)
    assert near >= 15, near
