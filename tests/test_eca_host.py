"""The float64 restatement of ECA_Filter (tests/eca_oracle.py) held to the reference's goldens and to its own normal equations,
and the reason the canceller exists: on slowly fluctuating clutter the joint solve leaves 20 dB less than LS_Filter_Multiple's
chain.  No GPU.

With one bin of 0 the restatement is LS_Filter_Toeplitz; measured distance to the reference's goldens (peak-normalised):
    ls_toeplitz_white     out 1.0e-7, taps 3.3e-8
    ls_toeplitz_peek0     out 2.5e-7, taps 5.3e-8
    ls_toeplitz_coloured  out 2.7e-7, taps 2.6e-7
`ls_multiple_bin50` is a two-bin chain (bins [0, 50]), not a single-bin one, so there is no single non-zero bin to hold against
it here; the device holds single non-zero bins against prc_ls_execute (tests/test_gpu_ls_eca.py)."""
import functools
import os
import re

import numpy as np
import pytest

import eca_oracle as E
from conftest import REPO, load_golden, rel_err
from oracle import np_oracle as O


@pytest.mark.parametrize("name", ["ls_toeplitz_white", "ls_toeplitz_peek0", "ls_toeplitz_coloured"])
def test_one_zero_bin_is_ls_filter_toeplitz(name):
    g = load_golden(name)
    out, taps = E.ECA_Filter(g["ref"], g["srv"], int(g["L"]), 1.0, [0.0], int(g["peek"]), 0.0, True)
    eo, et = rel_err(out, g["out"]), rel_err(taps[0], g["taps"])
    print(f"{name}: out {eo:.2e}, taps {et:.2e}")
    assert taps.shape == (1, int(g["L"]) + int(g["peek"])) and out.dtype == np.complex128
    assert eo <= 1e-4 and et <= 1e-4


def test_ls_multiple_bin50_is_a_two_bin_chain():
    """why no single-bin golden of LS_Filter_Multiple is held here (module docstring)"""
    assert len(load_golden("ls_multiple_bin50")["bins"]) == 2


@functools.lru_cache(maxsize=None)
def _scene_solution():
    ref, srv, floor = E.scene(1)
    out, taps, system = E.ECA_Filter(ref, srv, E.SCENE_L, E.SCENE_FS, E.SCENE_BINS, E.SCENE_PEEK, 0.0, True, True)
    return ref, srv, floor, out, taps, system


def test_normal_equation_residual():
    G, rhs, x = _scene_solution()[5]
    res = np.abs(G @ x - rhs).max() / np.abs(rhs).max()
    print(f"residual {res:.2e}, cond(G) {np.linalg.cond(G):.3g}")
    assert np.abs(G - G.conj().T).max() <= 1e-14 * np.abs(G).max() and res <= 1e-12


def test_joint_solve_beats_the_chain_by_15_dB():
    """Suppression condition.  Scene: n = 16384, Fs = 2n, filterLen 6, peek 10, bins [0, 1, -1, 2, -2]; echoes (delay, Doppler,
    amplitude) (2, 0, 1), (4, 0.6 Hz, 0.3), (5, -1.4 Hz, 0.2), (3, 1 Hz, 0.1); floor = a 40 Hz target of 0.01 + noise of 0.001.
    Re-measured: the chain leaves -26.0 dB of clutter above the floor, the joint solve -46.9 dB: 20.8 dB better
    (cond(G) = 5.1e2)."""
    ref, srv, floor, out, taps, _ = _scene_solution()
    T = E.SCENE_L + E.SCENE_PEEK
    chain = O.LS_Filter_Multiple(ref, srv, E.SCENE_L, E.SCENE_FS, E.SCENE_BINS)
    joint_db, chain_db = E.clutter_db(out, floor, T), E.clutter_db(chain, floor, T)
    print(f"chain {chain_db:.2f} dB, joint {joint_db:.2f} dB, gain {chain_db - joint_db:.2f} dB")
    assert chain_db - joint_db >= 15.0


def test_oracle_raises_on_a_length_mismatch():
    with pytest.raises(ValueError):
        E.ECA_Filter(np.zeros(64, np.complex64), np.zeros(65, np.complex64), 6, 1.0)


def test_public_surface():
    """ECA_Filter is exported, checks its lengths before it touches the library, "eca" is a HipBackend mode, the header declares
    the four entry points"""
    from passiveradar_amd import clutter_removal
    from passiveradar_amd.stream import HipBackend
    assert "ECA_Filter" in clutter_removal.__all__
    with pytest.raises(ValueError):
        clutter_removal.ECA_Filter(np.zeros(64, np.complex64), np.zeros(65, np.complex64), 6, 1.0)
    srv = np.ones(64, np.complex64)
    assert clutter_removal.ECA_Filter(np.ones(64, np.complex64), srv, 6, 1.0, dopplerBins=[]) is srv
    assert "eca" in HipBackend.CLUTTER_MODES
    header = open(os.path.join(REPO, "include", "prcore.h")).read()
    for sym in ("prc_eca_workspace_bytes", "prc_eca_execute", "prc_eca_set_profiling", "prc_eca_get_profile"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym


def test_size_limits_without_a_gpu():
    """prc_eca_workspace_bytes: 1 <= T < n, 1 <= nbins <= 8, nbins * T <= 4096 -- PRC_EINVAL (ValueError) otherwise"""
    from passiveradar_amd import engine
    assert engine.eca_workspace_bytes(27, 16, 10, 1, 1) > 0
    assert engine.eca_workspace_bytes(8192, 502, 10, 8, 2) > engine.eca_workspace_bytes(8192, 502, 10, 8, 1)
    for n, L, peek, nbins, nblocks in ((26, 16, 10, 1, 1), (100, 0, 0, 1, 1), (8192, 16, 10, 0, 1), (8192, 16, 10, 9, 1),
                                       (8192, 503, 10, 8, 1), (8192, 4087, 10, 1, 1), (8192, 16, 10, 1, 0), (8192, -1, 10, 1, 1)):
        with pytest.raises(ValueError):
            engine.eca_workspace_bytes(n, L, peek, nbins, nblocks)
