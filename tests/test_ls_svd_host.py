"""LS_Filter_SVD without a GPU: the float64 restatement (tests/ls_svd_oracle.py) against the reference's goldens, the public
names, the C ABI's declarations, the argument checks that run before the library is touched, and the committed profile."""
import glob
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden, rel_err
from ls_svd_oracle import default_rcond, ls_filter_svd
from passiveradar_amd import _lib
from passiveradar_amd.clutter_removal import LS_Filter_SVD

SVD_GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ls_svd_*.npz")))
EXPECTED = {"ls_svd_white", "ls_svd_white_peek0", "ls_svd_white_t74", "ls_svd_ar2", "ls_svd_periodic", "ls_svd_periodic_noise",
            "ls_svd_zero_ref"}


def test_the_goldens_are_there():
    assert set(SVD_GOLDENS) == EXPECTED


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_restatement_against_golden(name):
    """the reference's complex64 result lies within 2x its recorded float32 distance of the restatement (the generator
    recorded that distance with the NumPy of its day: 2x is the room another LAPACK may take); a silent reference is exact"""
    g = load_golden(name)
    L, peek = int(g["filterLen"]), int(g["peek"])
    out, taps = ls_filter_svd(g["ref"], g["srv"], L, peek)
    assert out.dtype == taps.dtype == np.complex128 and taps.shape == (L + peek,)
    if name == "ls_svd_zero_ref":
        assert np.array_equal(out, g["srv"].astype(np.complex128)) and not taps.any()
        assert np.array_equal(g["out"], g["srv"]) and not g["taps"].any()
        return
    d_out, d_taps = rel_err(g["out"], out), rel_err(g["taps"], taps)
    print(f"{name}: out {d_out:.2e} (recorded {float(g['dist_out']):.2e}) taps {d_taps:.2e} (recorded {float(g['dist_taps']):.2e})")
    assert d_out <= 2 * float(g["dist_out"]) and d_taps <= 2 * float(g["dist_taps"])
    assert float(g["dist_out"]) <= 5e-5                       # the room under the 1e-4 parity bar of the GPU test


def test_restatement_cut_rule():
    """rcond = 0 keeps everything above 1e-10; the default drops the null space of a periodic reference (rank 8 of 26)"""
    g = load_golden("ls_svd_periodic")
    info = {}
    ls_filter_svd(g["ref"], g["srv"], 16, 10, None, info)
    assert info["kept"] == 8 and info["cut"] == default_rcond(26) * info["sv"][0]
    assert abs(default_rcond(26) - 3.0e-7) < 0.05e-7 and abs(default_rcond(1044) - 1.9e-6) < 0.05e-6
    ls_filter_svd(g["ref"], g["srv"], 16, 10, 0.0, info)
    assert info["cut"] == 1e-10 and info["kept"] == int((info["sv"] >= 1e-10).sum())
    with pytest.raises(ValueError):
        ls_filter_svd(np.zeros(8), np.zeros(9), 2, 0)


def test_public_names():
    from passiveradar_amd import clutter_removal
    assert "LS_Filter_SVD" in clutter_removal.__all__
    assert "deliberately absent" not in clutter_removal.__doc__
    import inspect
    sig = inspect.signature(LS_Filter_SVD)
    assert list(sig.parameters) == ["refChannel", "srvChannel", "filterLen", "peek", "return_filter", "rcond", "return_singular_values"]
    assert sig.parameters["peek"].default == 10 and sig.parameters["return_filter"].default is False
    assert sig.parameters["rcond"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["rcond"].default is None
    assert sig.parameters["return_singular_values"].kind is inspect.Parameter.KEYWORD_ONLY


def test_abi_declarations():
    with open(os.path.join(REPO, "include", "prcore.h")) as f:
        header = f.read()
    for sym in ("prc_ls_svd_workspace_bytes", "prc_ls_svd_execute"):
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
    assert int(re.search(r"#define\s+PRC_VERSION\s+(\d+)", header).group(1)) >= 670
    assert _lib.MIN_LIB_VERSION >= 670
    from passiveradar_amd import engine
    assert callable(engine.ls_svd_workspace_bytes) and callable(engine.ls_svd_execute)


def test_shape_mismatch_raises_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    from passiveradar_amd import engine
    monkeypatch.setattr(engine, "lib", boom)
    with pytest.raises(ValueError, match="Input vectors must have the same length"):
        LS_Filter_SVD(np.zeros(100, np.complex64), np.zeros(101, np.complex64), 8)


def test_backend_argument_check():
    pytest.importorskip("torch")
    from passiveradar_amd.stream import HipBackend
    assert "ls_svd" in HipBackend.CLUTTER_MODES and "svd" not in HipBackend.CLUTTER_MODES
    with pytest.raises(ValueError):
        HipBackend(4096, 16, 32, 2.6e5, batch=2, clutter="svd")
    try:                                                  # past the argument check; without a GPU the device set-up then fails
        HipBackend(4096, 16, 32, 2.6e5, batch=2, clutter="ls_svd", ls_rcond=1e-5)
    except ValueError as e:
        pytest.fail(f"clutter='ls_svd' was rejected: {e}")
    except Exception:
        pass


def test_committed_profile_has_the_stage_keys():
    with open(os.path.join(REPO, "profiles", "ls_svd_bench.json")) as f:
        prof = json.load(f)
    assert {"cfg2", "cfg3"} <= set(prof["shapes"])
    for shape in prof["shapes"].values():
        assert {"n", "filter_len", "peek", "sweeps"} <= set(shape)
        assert {"correlate", "jacobi", "taps", "apply"} <= set(shape["ms"])
        assert all(v > 0 for v in shape["ms"].values())
        assert 0 < shape["correlate_fraction_of_fp64_fma_floor"] <= 1
    assert prof["reference_cpu"]["seconds"] > 0 and prof["reference_cpu"]["n"] > 0
