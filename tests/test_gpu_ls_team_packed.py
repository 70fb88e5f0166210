"""The fused pass of the 4096-point cached LS chain on packed-f32 transforms, two T2 twiddles read from LDS.

Shapes: the smallest at which every T2 twiddle (the 14 in registers and the 2 parked in LDS serve every transform), both
instantiations of the fused kernel (first bin zero / first bin rotated) and the edge code (a last piece of a few samples, a
last piece that is cut inside a 256-sample register row) run:
    L = 48   T = 58   slot origin 64    pieces of 4032    n = 2 * 4032 + 5 and 3 * 4032 + 5
    L = 256  T = 266  slot origin 272   pieces of 3824    n = 3 * 3824 + 1000
at fs = 1e4, where the per-bin rotation turns by whole radians inside one block.  The plan takes the 4096-point chain from
8192 samples on (prc_ls_plan_create), so 2 * 4032 + 5 = 8069 samples run the 1024-point chain even when method 4 is asked
for: that length stays as the boundary case just below the switch, and 3 * 4032 + 5 is the same edge on the team kernels.

Bars: the ones tests/test_gpu_parity.py holds this chain to -- 5e-6 peak-normalised against the float64 oracle for
LS_Filter_Multiple (test_ls_team_chain_last_piece_shorter_than_peek), and its TIGHT for the output and taps of the
peek = 0 run through LS_Filter_Toeplitz in that same test.
"""
import numpy as np
import pytest

from conftest import rel_err
from oracle import np_oracle as O
from passiveradar_amd import scene

pytestmark = pytest.mark.gpu

FS = 1.0e4
BAR = 5e-6
TIGHT = 2e-5
SHAPES = ((48, 2 * 4032 + 5), (48, 3 * 4032 + 5), (256, 3 * 3824 + 1000))
BINS = ([0, 1, -1, 2, -2], [2, 0, -1])


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    yield


@pytest.fixture(scope="module")
def scenes():
    """(ref, srv) per shape and the oracle's output per (shape, bins): made once, read only"""
    inputs, expected = {}, {}
    for L, n in SHAPES:
        ref, srv = scene.make_scene(n, FS, 50, 9000 + L)
        ref.setflags(write=False)
        srv.setflags(write=False)
        inputs[L, n] = (ref, srv)
        for bins in BINS:
            exp = O.LS_Filter_Multiple(ref, srv, L, FS, bins)
            exp.setflags(write=False)
            expected[L, n, tuple(bins)] = exp
    return inputs, expected


def _team_chain(fn, *args):
    from passiveradar_amd import clutter_removal as cr
    cr.set_default_ls_method(4)
    try:
        return fn(cr, *args)
    finally:
        cr.set_default_ls_method(0)


@pytest.mark.parametrize("bins", BINS, ids=lambda b: "bins" + "_".join(str(x) for x in b))
@pytest.mark.parametrize("L,n", SHAPES)
def test_ls_team_chain_packed_vs_oracle(L, n, bins, scenes):
    inputs, expected = scenes
    ref, srv = inputs[L, n]
    got = _team_chain(lambda cr: cr.LS_Filter_Multiple(ref, srv, L, FS, bins))
    e = rel_err(got, expected[L, n, tuple(bins)])
    print(f"L={L} n={ref.shape[0]} bins={bins}: rel err {e:.3e} (bar {BAR:g})")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert e < BAR, (L, bins, e)


def test_ls_team_toeplitz_peek0(scenes):
    ref, srv = scenes[0][48, 3 * 4032 + 5]
    got, taps = _team_chain(lambda cr: cr.LS_Filter_Toeplitz(ref, srv, 48, 0, True))
    exp, etaps = O.LS_Filter_Toeplitz(ref, srv, 48, 0, True)
    e, et = rel_err(got, exp), rel_err(taps, etaps)
    print(f"peek=0 L=48: output rel err {e:.3e}, taps rel err {et:.3e} (bar {TIGHT:g})")
    assert e < TIGHT and et < TIGHT, (e, et)


@pytest.mark.parametrize("L,n", SHAPES[1:])
def test_ls_team_chain_repeats_itself(L, n, scenes):
    """two calls on the same input return the same bits (nothing in the pass depends on what LDS or registers held)"""
    ref, srv = scenes[0][L, n]
    for bins in BINS:
        a = _team_chain(lambda cr: cr.LS_Filter_Multiple(ref, srv, L, FS, bins))
        b = _team_chain(lambda cr: cr.LS_Filter_Multiple(ref, srv, L, FS, bins))
        assert np.array_equal(a, b), (L, n, bins)
