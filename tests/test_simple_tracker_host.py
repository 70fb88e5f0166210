"""Host-side checks of simple_target_tracker and persistence: the NumPy restatement (tests/simple_tracker_oracle.py)
against the reference's goldens, the C ABI's struct layouts, argument checks and no CPU fallback."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import simple_tracker_oracle as O
from conftest import GOLDEN, REPO, load_golden

STRACK = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "strack_*.npz")))


def strack_frames(g):
    """the golden's frames (H, W, N) as float64"""
    return g["f64"] if "f64" in g else g["q"].astype(np.float64) / 256.0


def check_strack(h, g):
    """the bars: lock modes, measurement indices and measurements exact; estimate, x, P, S within 1e-9 relative"""
    for k in ("lock_mode", "measurement_idx", "measurement"):
        assert np.array_equal(np.asarray(h[k]), g[k]), k
    for k in ("estimate", "x", "P", "S"):
        np.testing.assert_allclose(np.asarray(h[k]).reshape(g[k].shape), g[k], rtol=1e-9, atol=1e-9, err_msg=k)


def persistence_cases():
    g = load_golden("persistence")
    for (which, k, hold, decay), out in zip(g["cases"], g["out"]):
        yield (g["x64"] if which == 0 else g["x32"]), int(k), int(hold), float(decay), out


def test_there_are_goldens():
    assert len(STRACK) >= 9 and os.path.exists(os.path.join(GOLDEN, "persistence.npz"))


@pytest.mark.parametrize("name", STRACK)
def test_restatement_matches_the_golden(name):
    g = load_golden(name)
    with np.errstate(all="ignore"):
        h = O.simple_target_tracker(strack_frames(g), g["ext"][0], g["ext"][1])
    check_strack(h, g)
    assert np.abs(h["badness"] - 12).min() > 1e-6


def test_goldens_cover_every_lock_transition():
    seen = set()
    for name in STRACK:
        st = np.argmax(load_golden(name)["lock_mode"], axis=1)
        seen |= {(int(a), int(b)) for a, b in zip(np.concatenate(([0], st[:-1])), st)}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 2), (2, 2), (2, 3), (3, 0), (3, 2)}


def test_restatement_reproduces_the_probes():
    """the reference probes the issue lists: all-zero / NaN frames -> (8, 0), +Inf -> that cell, an empty gate -> (0, 0)"""
    lock0 = np.array([1.0, 0, 0, 0])
    f = np.zeros((64, 40))
    assert O.argmax_index(f, lock0, 35, -30) == (8, 0)
    f = np.ones((64, 40))
    f[5, 5] = np.nan
    assert O.argmax_index(f, lock0, 35, -30) == (8, 0)
    f = np.ones((64, 40))
    f[64 - 1 - 30, 20] = np.inf                     # s[20, 30]
    assert O.argmax_index(f, lock0, 35, -30) == (20, 30)
    f = np.random.default_rng(0).exponential(1.0, (80, 48))
    assert O.argmax_index(f, np.array([0.0, 1, 0, 0]), 20, 40) == (0, 0)     # rows s[-4:44] -> s[44:44]: empty
    assert O.window(20, 40, (24, 48), 48, 80)[0] == (44, 44)
    assert O.argmax_index(f, np.array([0.0, 0, 1, 0]), 20, 40) != (0, 0)     # rows s[4:36]


def test_persistence_restatement_matches_the_golden():
    n = 0
    for X, k, hold, decay, out in persistence_cases():
        with np.errstate(all="ignore"):
            mine = O.persistence(X, k, hold, decay)
        assert np.array_equal(mine.view(np.uint64), out.view(np.uint64)) or np.array_equal(mine, out, equal_nan=True)
        n += 1
    assert n == 240


def test_persistence_restatement_raises_past_the_stack():
    X = np.ones((3, 2, 4))
    with pytest.raises(IndexError):
        O.persistence(X, 4, 2, 0.9)
    assert np.array_equal(O.persistence(X, 4, 0, 0.9), np.zeros((3, 2)))


def test_strack_structs_match_the_header(tmp_path):
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "st.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  prc_strack_desc d; PRC_DESC_INIT(d);\n'
                   '  printf("%zu %zu %zu %zu %zu %u %u\\n", sizeof(prc_strack_desc), offsetof(prc_strack_desc, H),\n'
                   '         offsetof(prc_strack_desc, dtype), offsetof(prc_strack_desc, range_extent),\n'
                   '         offsetof(prc_strack_desc, doppler_extent), PRC_STRACK_DESC_SIZE_630, d.struct_size);\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %u %d %d %d\\n", sizeof(prc_strack_record),\n'
                   '         offsetof(prc_strack_record, measurement), offsetof(prc_strack_record, measurement_idx),\n'
                   '         offsetof(prc_strack_record, estimate), offsetof(prc_strack_record, x),\n'
                   '         offsetof(prc_strack_record, P), offsetof(prc_strack_record, S), PRC_STRACK_RECORD_SIZE,\n'
                   '         (int)PRC_REAL_F32, (int)PRC_REAL_F64, PRC_PERSISTENCE_TERMS_PER_LAUNCH); return 0; }\n')
    exe = tmp_path / "st"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    D, Rc = _lib.StrackDesc, _lib.StrackRecord
    assert rows[0] == [ctypes.sizeof(D), D.H.offset, D.dtype.offset, D.range_extent.offset, D.doppler_extent.offset,
                       ctypes.sizeof(D), ctypes.sizeof(D)]
    assert rows[1] == [ctypes.sizeof(Rc), Rc.measurement.offset, Rc.measurement_idx.offset, Rc.estimate.offset,
                       Rc.x.offset, Rc.P.offset, Rc.S.offset, ctypes.sizeof(Rc), _lib.REAL_F32, _lib.REAL_F64,
                       _lib.PERSISTENCE_TERMS_PER_LAUNCH]
    dt = _lib.STRACK_RECORD_DTYPE
    assert dt.itemsize == ctypes.sizeof(Rc)
    assert [dt.fields[k][1] for k in ("measurement_idx", "P", "S")] == [Rc.measurement_idx.offset, Rc.P.offset,
                                                                        Rc.S.offset]


def test_strack_arguments_are_checked_without_a_gpu():
    from passiveradar_amd import _lib
    lib = _lib.lib()
    nb = ctypes.c_size_t(0)
    good = dict(H=96, W=48, dtype=0, range_extent=100.0, doppler_extent=100.0)
    d = _lib.StrackDesc(**good)
    assert lib.prc_strack_workspace_bytes(ctypes.byref(d), 10, ctypes.byref(nb)) == _lib.PRC_OK and nb.value > 0
    assert lib.prc_strack_workspace_bytes(ctypes.byref(d), -1, ctypes.byref(nb)) == _lib.PRC_EINVAL
    for bad in (dict(H=0), dict(W=0), dict(dtype=2), dict(dtype=-1), dict(H=1 << 16, W=1 << 16)):
        d = _lib.StrackDesc(**{**good, **bad})
        assert lib.prc_strack_workspace_bytes(ctypes.byref(d), 1, ctypes.byref(nb)) == _lib.PRC_EINVAL, bad
        assert lib.prc_strack_run(ctypes.byref(d), 8, 1, None, 8, 8, None) == _lib.PRC_EINVAL, bad
    d = _lib.StrackDesc(**good)
    assert lib.prc_strack_run(ctypes.byref(d), 8, -1, None, 8, 8, None) == _lib.PRC_EINVAL
    assert lib.prc_strack_run(ctypes.byref(d), None, 1, None, 8, 8, None) == _lib.PRC_EINVAL
    d.magic = 0
    assert lib.prc_strack_run(ctypes.byref(d), 8, 1, None, 8, 8, None) == _lib.PRC_EINVAL
    assert lib.prc_strack_run(ctypes.byref(_lib.StrackDesc(**good)), 8, 0, None, 8, 8, None) == _lib.PRC_OK


def test_persistence_arguments_are_checked_without_a_gpu():
    from passiveradar_amd import _lib
    f = _lib.lib().prc_persistence
    assert f(8, 2, 10, 4, 0, 4, 3, 0.9, 8, 1, None) == _lib.PRC_EINVAL          # in dtype
    assert f(8, 0, 10, 4, 0, 4, 3, 0.9, 8, 5, None) == _lib.PRC_EINVAL          # out dtype
    assert f(8, 0, -1, 4, 0, 4, 3, 0.9, 8, 1, None) == _lib.PRC_EINVAL          # frame_elems
    assert f(8, 0, 10, -1, 0, 4, 3, 0.9, 8, 1, None) == _lib.PRC_EINVAL         # nframes
    assert f(8, 0, 10, 4, 0, -1, 3, 0.9, 8, 1, None) == _lib.PRC_EINVAL         # k_count
    assert f(8, 0, 10, 4, 2, 3, 3, 0.9, 8, 1, None) == _lib.PRC_EINVAL          # frame 4 of 4 read
    assert f(8, 0, 10, 4, 0, 4, 3, 0.9, None, 1, None) == _lib.PRC_EINVAL       # null out
    assert f(8, 0, 10, 300, 0, 300, 300, 0.9, 8, 0, None) == _lib.PRC_EINVAL   # > 256 terms into a float32 out
    assert f(8, 0, 10, 4, 0, 0, 3, 0.9, 8, 1, None) == _lib.PRC_OK              # nothing to do


def test_drop_ins_raise_without_a_gpu():
    from passiveradar_amd import _lib
    from passiveradar_amd.plotting_tools import persistence, persistence_stack
    from passiveradar_amd.target_detection import simple_target_tracker, simple_track_maps
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.PrcoreError):
        simple_target_tracker(np.ones((32, 24, 3)), 10.0, 10.0)
    with pytest.raises(_lib.PrcoreError):
        simple_track_maps(np.ones((32, 24, 3), np.complex64), 10.0, 10.0)
    with pytest.raises(_lib.PrcoreError):
        persistence(np.ones((4, 3, 5)), 2, 20, 0.9)
    with pytest.raises(_lib.PrcoreError):
        persistence_stack(np.ones((4, 3, 5)), 20, 0.9)


def test_drop_ins_have_the_reference_signatures():
    import inspect
    from passiveradar_amd import plotting_tools, target_detection
    assert list(inspect.signature(target_detection.simple_target_tracker).parameters)[:3] == \
        ["data", "rangeExtent", "dopplerExtent"]
    assert list(inspect.signature(plotting_tools.persistence).parameters) == ["X", "k", "hold", "decay"]
    assert "simple_target_tracker" in target_detection.__all__ and "persistence" in plotting_tools.__all__
    dt = target_detection.target_track_dtype_simple
    assert dt.names == ("lock_mode", "measurement", "measurement_idx", "estimate", "range_extent", "doppler_extent",
                        "kalman_state")
    assert dt["measurement_idx"].base == np.int64 and dt["lock_mode"].base == np.float64


def test_goldens_stay_small():
    for fn in glob.glob(os.path.join(GOLDEN, "strack_*.npz")) + [os.path.join(GOLDEN, "persistence.npz")]:
        assert os.path.getsize(fn) <= 1 << 20, fn
