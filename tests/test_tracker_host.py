"""Host-side checks of the tracker feature: the NumPy restatement (tests/tracker_oracle.py) against the reference's
goldens, its percentile / linspace helpers against NumPy, the C ABI's struct layouts, and no CPU fallback."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tracker_oracle as T
from conftest import REPO, load_golden


def measure_frames():
    g = load_golden("tracker_measure")
    for i in range(int(g["nframes"])):
        yield (g[f"f{i}"].astype(np.float64) / 256.0, g[f"ext{i}"], g[f"cand{i}"], g[f"idx{i}"], bool(g[f"tied{i}"]))


def check_candidates(m, cand, idx, tied):
    """the bars of the measurement golden: indices and order exact, coordinates bitwise, strengths 1e-12 relative;
    frames whose candidates all tie (8 x 17: every cell masked) compare as a set -- the reference's order is undefined"""
    if tied:
        o = np.argsort(idx)
        p = np.argsort(m["idx"])
        assert np.array_equal(np.asarray(m["idx"])[p], idx[o])
        assert np.array_equal(np.asarray(m["range"])[p], cand[0][o])
        assert np.array_equal(np.asarray(m["doppler"])[p], cand[1][o])
        assert np.array_equal(np.asarray(m["strength"])[p], cand[2][o])
        return
    assert np.array_equal(np.asarray(m["idx"]), idx)
    assert np.array_equal(np.asarray(m["range"]), cand[0])
    assert np.array_equal(np.asarray(m["doppler"]), cand[1])
    np.testing.assert_allclose(m["strength"], cand[2], rtol=1e-12, atol=0)


def check_history(h, g):
    """the bars of the tracker golden: status, lifetime, found history exact; states within 1e-9"""
    assert np.array_equal(h["status"], g["status"])
    assert np.array_equal(h["lifetime"], g["lifetime"])
    assert np.array_equal(h["hist"], g["history"])
    for k in ("measurement", "estimate", "x", "P", "S"):
        np.testing.assert_allclose(h[k], g[k], rtol=1e-9, atol=1e-9, err_msg=k)


def test_restatement_matches_the_measurement_golden():
    for f, ext, cand, idx, tied in measure_frames():
        check_candidates(T.measure(f, ext), cand, idx, tied)


def test_restatement_matches_the_tracker_golden():
    g = load_golden("tracker_scene")
    frames = g["frames"].astype(np.float64) / 256.0
    h = T.history_arrays(T.multitarget_tracker(frames, g["extent"], int(g["ntracks"])))
    check_history(h, g)
    st = g["status"]
    trans = {(int(a), int(b)) for a, b in zip(st[:-1].ravel(), st[1:].ravel())}
    assert {(0, 1), (1, 0), (1, 2), (2, 0)} <= trans


@pytest.mark.parametrize("p", [99.8, 0.0, 100.0, 50.0, 12.5, 99.0, 75.0])
def test_percentile_helper_is_numpy_bitwise(p):
    rng = np.random.default_rng(7)
    for n in list(range(1, 40)) + [136, 501, 1001, 4608, 5001, 4097]:
        x = rng.standard_normal(n)
        assert T.percentile(x, p) == np.percentile(x, p), (n, p)
        q = np.round(x * 2) / 2                 # many ties: a == b
        assert T.percentile(q, p) == np.percentile(q, p), (n, p)


def test_percentile_kt_cases():
    # q (n-1) integral: t == 0 and the result is x(k) itself
    assert T.percentile_kt(1001, 50.0) == (500, 0.0)
    assert T.percentile_kt(136, 100.0) == (135, 0.0)
    assert T.percentile_kt(136, 0.0) == (0, 0.0)
    k, t = T.percentile_kt(96 * 48)
    assert k == int(np.floor(0.998 * (96 * 48 - 1))) and 0 <= t < 1


def test_lerp_upper_branch():
    a, b = 1.0, 1.0 + 2 ** -40
    for t in (0.25, 0.5, 0.75, 0.999):
        assert T.lerp(a, b, t) == np.percentile([a, b], 100 * t)


def test_linspace_helper_is_numpy_bitwise():
    for start, stop, num in ((120.0, 0, 48), (-150.0, 150.0, 96), (77.25, 0, 49), (-251.5, 251.5, 97),
                             (300.0, 0, 177), (-10.0, 10.0, 1024), (1.0 / 3, 0, 17)):
        assert np.array_equal(T.linspace(start, stop, num), np.linspace(start, stop, num))


def test_track_structs_match_the_header(tmp_path):
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "tr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_track_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %u %u %u %u\\n", sizeof(prc_track_desc), offsetof(prc_track_desc, H),\n'
                   '         offsetof(prc_track_desc, percentile), offsetof(prc_track_desc, range_extent),\n'
                   '         sizeof(prc_track_record), offsetof(prc_track_record, history), offsetof(prc_track_record, overflow),\n'
                   '         PRC_TRACK_DESC_SIZE_610, PRC_TRACK_RECORD_SIZE, PRC_TRACK_CAND_SIZE, d.struct_size);\n'
                   '  printf("%zu %zu\\n", sizeof(prc_track_cand), offsetof(prc_track_cand, index)); return 0; }\n')
    exe = tmp_path / "tr"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    D, Rc = _lib.TrackDesc, _lib.TrackRecord
    assert rows[0] == [ctypes.sizeof(D), D.H.offset, D.percentile.offset, D.range_extent.offset, ctypes.sizeof(Rc),
                       Rc.history.offset, Rc.overflow.offset, ctypes.sizeof(D), ctypes.sizeof(Rc),
                       ctypes.sizeof(_lib.TrackCand), ctypes.sizeof(D)]
    assert rows[1] == [ctypes.sizeof(_lib.TrackCand), _lib.TrackCand.index.offset]
    assert _lib.TRACK_RECORD_DTYPE.itemsize == ctypes.sizeof(Rc)
    assert _lib.TRACK_RECORD_DTYPE.fields["overflow"][1] == Rc.overflow.offset
    assert _lib.TRACK_CAND_DTYPE.itemsize == ctypes.sizeof(_lib.TrackCand)


def test_track_plan_arguments_are_checked_without_a_gpu():
    from passiveradar_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    good = dict(H=16, W=17, ntracks=10, capacity=64, percentile=99.8, doppler_extent=1.0, range_extent=1.0)
    for bad in (dict(H=7), dict(W=16), dict(ntracks=0), dict(ntracks=65), dict(percentile=-0.1),
                dict(percentile=100.5), dict(capacity=0)):
        d = _lib.TrackDesc(**{**good, **bad})
        d.struct_size, d.magic = ctypes.sizeof(_lib.TrackDesc), _lib.DESC_MAGIC
        assert lib.prc_track_plan_create(ctypes.byref(h), ctypes.byref(d)) == _lib.PRC_EINVAL, bad
    d = _lib.TrackDesc(**good)
    d.struct_size, d.magic = ctypes.sizeof(_lib.TrackDesc), _lib.DESC_MAGIC
    assert lib.prc_track_plan_create(ctypes.byref(h), ctypes.byref(d)) == _lib.PRC_OK
    assert lib.prc_track_plan_destroy(h) == _lib.PRC_OK


def test_tracker_functions_raise_without_a_gpu():
    from passiveradar_amd import _lib
    from passiveradar_amd.target_detection import get_measurements, multitarget_tracker, track_maps
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    f = np.ones((32, 24))
    with pytest.raises(_lib.PrcoreError):
        get_measurements(f, 99.8, [10.0, 10.0])
    with pytest.raises(_lib.PrcoreError):
        multitarget_tracker(np.ones((32, 24, 3)), [10.0, 10.0], 10)
    with pytest.raises(_lib.PrcoreError):
        track_maps(np.ones((32, 24, 3), np.complex64), [10.0, 10.0])


def test_goldens_stay_small():
    for fn in ("tracker_measure.npz", "tracker_scene.npz"):
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", fn)) <= 1 << 20
