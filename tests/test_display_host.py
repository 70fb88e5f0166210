"""The display contract on the host (no GPU): the gnuplot2 table against its recorded bytes and matplotlib, the NumPy
restatement (tests/display_oracle.py) against np.percentile and matplotlib's own to_rgba, and the argument checks of the
Python layer."""
import os

import numpy as np
import pytest

import display_oracle as D
from conftest import GOLDEN


def recorded_lut():
    """plt.get_cmap('gnuplot2')(np.arange(256), bytes=True), recorded with matplotlib 3.10.8"""
    return np.load(os.path.join(GOLDEN, "gnuplot2_lut.npy"), allow_pickle=False)


def host_cases():
    c = D.frame_cases()
    rng = np.random.default_rng(11)
    c["dense_1024x177"] = rng.exponential(1.0, (1024, 177))
    f = rng.exponential(1.0, (1024, 177))
    f[rng.random(f.shape) < 0.5] = 0.0
    c["half_zero_1024x177"] = f
    return c


def test_gnuplot2_table_equals_the_recorded_bytes():
    from passiveradar_amd.plotting_tools import gnuplot2_lut
    want = recorded_lut()
    assert want.shape == (256, 4) and want.dtype == np.uint8
    got = gnuplot2_lut()
    assert got.dtype == np.uint8 and got.shape == (256, 4) and got.flags.c_contiguous
    assert np.array_equal(got, want)
    assert np.array_equal(D.gnuplot2_lut(), want)


def test_gnuplot2_table_equals_matplotlib():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from passiveradar_amd.plotting_tools import gnuplot2_lut
    want = plt.get_cmap("gnuplot2")(np.arange(256), bytes=True)
    assert np.array_equal(gnuplot2_lut(), want) and np.array_equal(recorded_lut(), want)


@pytest.mark.parametrize("p", [(35, 99), (0, 100), (50, 50), (12.5, 99.8)])
def test_oracle_limits_equal_numpy(p):
    for name, f in host_cases().items():
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.array([np.percentile(f.flatten(), p[0]), 1.5 * np.percentile(f.flatten(), p[1])])
        assert np.array_equal(D.limits(f, p[0], p[1], 1.5), want, equal_nan=True), name


def test_oracle_rgba_equals_matplotlib():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import Normalize
    cmap = plt.get_cmap("gnuplot2")
    for name, f in host_cases().items():
        lim = D.limits(f)
        s = np.fliplr(f.T)
        with np.errstate(invalid="ignore", over="ignore"):
            want = ScalarMappable(Normalize(lim[0], lim[1]), cmap).to_rgba(s, bytes=True)
        got = D.render(f)
        assert got.shape == s.shape + (4,) and np.array_equal(got, want), name
    # given limits: a fixed scale, and vmin == vmax (Normalize fills with 0)
    f = host_cases()["negative"]
    for lim in ((-2.0, 3.0), (0.5, 0.5)):
        want = ScalarMappable(Normalize(*lim), cmap).to_rgba(np.fliplr(f.T), bytes=True)
        assert np.array_equal(D.render(f, lim=lim), want), lim
    with pytest.raises(ValueError):      # the deviation: matplotlib raises, the device paints (0, 0, 0, 0)
        ScalarMappable(Normalize(3.0, -2.0), cmap).to_rgba(f, bytes=True)
    assert not D.render(f, lim=(3.0, -2.0)).any()


def test_python_layer_refuses_bad_arguments():
    """checked before anything touches a device"""
    from passiveradar_amd import plotting_tools as P
    X = np.ones((4, 3, 2))
    for bad in (dict(p_lo=-1), dict(p_hi=100.5), dict(p_lo=float("nan"))):
        with pytest.raises(ValueError):
            P.display_limits(X, **bad)
        with pytest.raises(ValueError):
            P.render_frames(X, **bad)
    with pytest.raises(ValueError):
        P.display_limits(np.ones((4, 3)))
    with pytest.raises(ValueError):
        P.render_frames(np.ones((4, 3)))
    with pytest.raises(ValueError):
        P.render_frames(X, orient="sideways")
    for lut in (np.zeros((255, 4), np.uint8), np.zeros((256, 3), np.uint8), np.zeros((256, 4), np.float32)):
        with pytest.raises(ValueError):
            P.render_frames(X, lut=lut)
    with pytest.raises(ValueError):
        P.render_frames(X, limits=np.zeros((3, 2)))
    with pytest.raises(ValueError):
        P.render_maps(np.ones((4, 3)))
    with pytest.raises(ValueError):
        P.render_maps(np.ones((4, 3, 2)), slab=0)
    assert {"gnuplot2_lut", "display_limits", "render_frames", "render_maps"} <= set(P.__all__)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """prc_display_limits / prc_display_rgba check their arguments before they launch anything"""
    import ctypes as C
    from passiveradar_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                 # never dereferenced: every call below is refused
    E = _lib.PRC_EINVAL
    assert lib.prc_display_limits(p, 2, 10, 1, 35.0, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 0, 1, 35.0, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 2 ** 31, 1, 35.0, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 10, -1, 35.0, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 10, 1, -0.5, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 10, 1, 35.0, 100.5, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 10, 1, float("nan"), 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(None, 1, 10, 1, 35.0, 99.0, 1.5, p, None) == E
    assert lib.prc_display_limits(p, 1, 10, 1, 35.0, 99.0, 1.5, None, None) == E
    assert "prc_display_limits" in lib.prc_last_error().decode()
    assert lib.prc_display_rgba(p, 3, 4, 4, 1, p, None, 0, p, None) == E
    assert lib.prc_display_rgba(p, 1, 4, 4, 1, p, None, 2, p, None) == E
    assert lib.prc_display_rgba(p, 1, 0, 4, 1, p, None, 0, p, None) == E
    assert lib.prc_display_rgba(p, 1, 65536, 32768, 1, p, None, 0, p, None) == E
    assert lib.prc_display_rgba(p, 1, 4, 4, -1, p, None, 0, p, None) == E
    assert lib.prc_display_rgba(None, 1, 4, 4, 1, p, None, 0, p, None) == E
    assert lib.prc_display_rgba(p, 1, 4, 4, 1, None, None, 0, p, None) == E
    assert lib.prc_display_rgba(p, 1, 4, 4, 1, p, None, 0, None, None) == E
    assert "prc_display_rgba" in lib.prc_last_error().decode()
    assert lib.prc_display_limits(p, 1, 10, 0, 35.0, 99.0, 1.5, p, None) == _lib.PRC_OK      # no frames: a no-op
    assert lib.prc_display_rgba(p, 1, 4, 4, 0, p, None, 0, p, None) == _lib.PRC_OK
