"""GAL_JPE without a GPU: the NumPy restatement (tests/gal_oracle.py) against the reference's goldens, the drop-in's argument
errors (raised before the library is touched) and the C ABI's declarations."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden
from gal_oracle import gal_jpe

GAL_GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "gal_*.npz")))


def _rel(a, b):
    s = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (s if s > 0 else 1.0)


def test_goldens_present():
    assert len(GAL_GOLDENS) >= 11, GAL_GOLDENS


@pytest.mark.parametrize("name", GAL_GOLDENS)
def test_restatement_matches_reference(name):
    g = load_golden(name)
    out, k, h = gal_jpe(g["ref"], g["srv"], int(g["L"]), int(g["D"]), float(g["mu1"]), float(g["mu2"]), int(g["peek"]),
                        np.complex64, True)
    assert out.shape == g["out"].shape and k.shape == g["k"].shape and h.shape == g["h"].shape
    if not np.any(g["out"]):
        assert not np.any(out) and not np.any(k) and not np.any(h)
        return
    assert _rel(out, g["out"]) <= 2e-6
    assert _rel(k, g["k"]) <= 2e-6 if np.any(g["k"]) else not np.any(k)
    assert _rel(h, g["h"]) <= 2e-6


def test_restatement_caps_mu1():
    g = load_golden("gal_fm_L4_D64_cap")
    st = {}
    gal_jpe(g["ref"], g["srv"], int(g["L"]), int(g["D"]), float(g["mu1"]), float(g["mu2"]), int(g["peek"]), stats=st)
    assert st["caps"] >= 1
    g = load_golden("gal_white_L8_D64")
    gal_jpe(g["ref"], g["srv"], int(g["L"]), int(g["D"]), float(g["mu1"]), float(g["mu2"]), int(g["peek"]), stats=st)
    assert st["caps"] == 0


def test_drop_in_argument_errors():
    from passiveradar_amd.clutter_removal import GAL_JPE
    x = np.ones(64, np.complex64)
    with pytest.raises(ValueError, match="same length"):
        GAL_JPE(x, x[:63], 4, 8, 1e-3, 1e-2)
    with pytest.raises(ValueError):
        GAL_JPE(x, x, 9, 8, 1e-3, 1e-2)           # lattice longer than the delay line
    with pytest.raises(ValueError):
        GAL_JPE(x, x, 0, 8, 1e-3, 1e-2)           # no lattice at all
    with pytest.raises(ValueError):
        GAL_JPE(x, x, -2, 8, 1e-3, 1e-2)


def test_drop_in_signature():
    import inspect
    from passiveradar_amd import clutter_removal
    assert "GAL_JPE" in clutter_removal.__all__
    params = inspect.signature(clutter_removal.GAL_JPE).parameters
    assert list(params) == ["refChannel", "srvChannel", "latticeLen", "delayLineLen", "mu1", "mu2", "peek", "return_filter"]
    assert params["peek"].default == 10 and params["return_filter"].default is False


def test_abi_declares_gal():
    import re
    from passiveradar_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "prcore.h")).read(), flags=re.S)
    for sym in ("prc_gal_execute", "prc_gal_workspace_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", text), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define PRC_VERSION (\d+)", text).group(1)) >= 620
    assert _lib.MIN_LIB_VERSION >= 620


def test_workspace_bytes_without_gpu():
    from passiveradar_amd import engine
    assert engine.gal_workspace_bytes(2048, 7) == 0
    nb = engine.gal_workspace_bytes(2100, 3)
    assert nb >= 3 * 2100 * 36 and nb % 16 == 0


def test_backend_rejects_bad_lattice():
    pytest.importorskip("torch")
    from passiveradar_amd.stream import HipBackend
    with pytest.raises(ValueError):
        HipBackend(4096, 16, 32, 2.6e5, batch=2, clutter="gal", gal_lattice=17)
