"""The shared device primitives of passiveradar_amd/csrc/order_select.h and wave.h on their own, through the test-only
probe tests/csrc/libosprobe.so (one workgroup per call): prc_resolve_digit against np.cumsum, prc_bitonic against np.sort,
and the wavefront reductions against NumPy emulations of their own addition trees, bit for bit.  The units that use them
(display, tracker, plots, OS-CFAR, NLMS, GAL) are held to their oracles by their own tests."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")

WAVE_IN = np.dtype([("d", np.float64, 64), ("q", np.uint64, 64), ("u", np.uint32, 64),
                    ("yr", np.float32, 64), ("yi", np.float32, 64), ("bb", np.float32, 64)])
WAVE_OUT = np.dtype([("sum", np.float64, 64), ("minq", np.uint64, 64), ("minu", np.uint32, 64), ("a2r", np.float32, 64),
                     ("a2i", np.float32, 64), ("a3r", np.float32, 64), ("a3i", np.float32, 64), ("a3b", np.float32, 64)])


@pytest.fixture(scope="module")
def probe(gpu_ready):
    so = os.path.join(CSRC, "libosprobe.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", CSRC, "libosprobe.so"])
    from passiveradar_amd import _lib
    _lib.lib()                              # one HIP runtime per process (loads torch's copy first when present)
    h = ctypes.CDLL(so)
    h.osp_resolve.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    h.osp_bitonic.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
    h.osp_wave.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert h.osp_wave_in_bytes() == WAVE_IN.itemsize and h.osp_wave_out_bytes() == WAVE_OUT.itemsize

    def call(name, *args):
        rc = getattr(h, name)(*args)
        if rc in (-3, -4):                  # the launch or the device failed: nothing more runs on it from this module
            pytest.exit("order-select probe %s: HIP error %d" % (name, rc), returncode=3)
        assert rc == 0, (name, rc)
    return call


# ---- prc_resolve_digit ----------------------------------------------------------------------------------------------
def _bin_ranks(hist, bins):
    """the first and the last rank of each (non-empty) bin"""
    cum = np.cumsum(hist)
    out = []
    for b in bins:
        assert hist[b] > 0, b
        out += [cum[b] - hist[b], cum[b] - 1]
    return out


def _resolve_cases(nb):
    """(name, histogram, ranks)"""
    rng = np.random.default_rng(nb)
    # thread t owns bins 2t, 2t+1 and a wavefront 128 of them: every boundary between two wavefronts, both ends, and a
    # stretch of empty bins with a populated bin on either side
    spread = rng.integers(0, 6, nb).astype(np.uint32)
    edges = [b for w in range(1, nb // 128) for b in (128 * w - 1, 128 * w)]
    spread[[0, nb - 1] + edges] = rng.integers(1, 6, 2 + len(edges))
    spread[300:340] = 0
    spread[[299, 340]] = [3, 2]
    ranks = _bin_ranks(spread, [0, nb - 1] + edges + [299, 340]) + rng.integers(0, spread.sum(), 32).tolist()
    yield "spread", spread, ranks
    # one bin holds every count: an inner bin, the first and the last
    for b in (201, 0, nb - 1):
        one = np.zeros(nb, np.uint32)
        one[b] = 5000
        yield "all_in_bin_%d" % b, one, [0, 2500, 4999]
    # counts whose running sum needs all 32 bits of the scan
    big = np.full(nb, (2 ** 32 - 1) // nb, np.uint32)
    yield "large_counts", big, [0, int(big.sum(dtype=np.uint64)) - 1, int(big[0]) * 128 - 1, int(big[0]) * 128]


@pytest.mark.parametrize("nb", [512, 1024, 2048])
def test_resolve_digit_finds_the_bin_of_a_rank(probe, nb):
    for name, hist, ranks in _resolve_cases(nb):
        ranks = np.asarray(ranks, np.uint32)
        out = np.zeros((len(ranks), 3), np.uint32)
        probe("osp_resolve", hist.ctypes.data, nb, ranks.ctypes.data, len(ranks), out.ctypes.data)
        cum = np.cumsum(hist, dtype=np.uint64)
        bins = np.searchsorted(cum, ranks, side="right")          # the first bin whose running count exceeds the rank
        exp = np.stack([bins, cum[bins] - hist[bins], hist[bins]], axis=1).astype(np.uint32)
        assert np.array_equal(out, exp), (nb, name, ranks[(out != exp).any(axis=1)][:4], out[(out != exp).any(axis=1)][:4])


# ---- prc_bitonic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carried", [False, True], ids=["keys_only", "with_values"])
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("P,in_global", [(2, 0), (64, 0), (1024, 0), (2048, 0), (8192, 1)])
def test_bitonic_sorts_keys_and_carries_values(probe, P, in_global, desc, carried):
    rng = np.random.default_rng(P + 2 * desc + carried)
    keys = rng.integers(0, 2 ** 64, P, dtype=np.uint64)
    keys[rng.integers(0, P, P // 8)] = np.uint64(2 ** 64 - 1)        # the padding value of plots.hip, and 0, track.hip's
    keys[rng.integers(0, P, P // 8)] = np.uint64(0)
    if carried:                                                     # a value is identified by its key: make the keys unique
        keys = rng.permutation((keys & np.uint64(0xffffffffffff0000)) | np.arange(P, dtype=np.uint64))
    else:                                                           # planted duplicates
        keys[rng.integers(0, P, max(P // 4, 1))] = keys[0]
    vals = rng.permutation(P).astype(np.uint32)
    k, v = keys.copy(), vals.copy()
    probe("osp_bitonic", k.ctypes.data, v.ctypes.data if carried else None, P, int(desc), in_global)
    order = np.argsort(keys, kind="stable")
    if desc:
        order = order[::-1]
    assert np.array_equal(k, keys[order])
    if carried:
        assert len(np.unique(keys)) == P and np.array_equal(v, vals[order])
    else:
        assert np.array_equal(v, vals)


# ---- wave.h ---------------------------------------------------------------------------------------------------------
LANE = np.arange(64)


def _butterfly_sum(x):
    """wave_sum: lane l adds lane l ^ o, o = 32 .. 1, in the input's own precision"""
    v = x.copy()
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[LANE ^ o]
    return v


def _fold_chain(lo, hi):
    """one chain of wave_allsum2 / wave_allsum3 in float32: lanes 0-31 take lo(l) + lo(l+32), lanes 32-63 hi(l-32) + hi(l);
    then every lane adds its partner under quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and row_mirror; then
    rows 1 and 3 add lane 15 of the row before them (rows 0 and 2 add 0).  Lane 31 holds sum(lo), lane 63 sum(hi)."""
    v = np.concatenate([lo[:32] + lo[32:], hi[:32] + hi[32:]]).astype(np.float32)
    for partner in (LANE ^ 1, LANE ^ 2, (LANE & ~7) | (7 - (LANE & 7)), (LANE & ~15) | (15 - (LANE & 15))):
        v = v + v[partner]
    row = LANE >> 4
    bcast = np.where(row % 2 == 1, v[(row - 1) * 16 + 15], np.float32(0))
    return (v + bcast).astype(np.float32)


def _wave_inputs(seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(1, WAVE_IN)
    # magnitudes spread over many binades, so that a different pairing order rounds differently
    x["d"] = rng.standard_normal(64) * 10.0 ** rng.integers(-6, 7, 64)
    x["q"] = rng.integers(2 ** 40, 2 ** 64, 64, dtype=np.uint64)
    x["u"] = rng.integers(2 ** 10, 2 ** 32, 64, dtype=np.uint32)
    for f in ("yr", "yi"):
        x[f] = (rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4, 64)).astype(np.float32)
    x["bb"] = (rng.standard_normal(64) ** 2).astype(np.float32)
    return x


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_wave_reductions_follow_their_own_trees_bit_for_bit(probe, seed):
    x = _wave_inputs(seed)
    if seed == 1:                           # the minimum in the last lane, and one that differs only in its upper word
        x["q"][0, 63] = 5
        x["u"][0, 63] = 3
    if seed == 2:
        x["q"][0, :] |= np.uint64(2 ** 63)
        x["q"][0, 17] = np.uint64(2 ** 32 + 0xffffffff)
        x["q"][0, 40] = np.uint64(2 ** 33)
    out = np.zeros(1, WAVE_OUT)
    probe("osp_wave", x.ctypes.data, out.ctypes.data)
    i, o = x[0], out[0]
    assert np.array_equal(o["sum"].view(np.uint64), _butterfly_sum(i["d"]).view(np.uint64))
    assert (o["minq"] == i["q"].min()).all() and (o["minu"] == i["u"].min()).all()
    c0 = _fold_chain(i["yr"], i["yi"])
    c1 = _fold_chain(i["bb"], i["bb"])
    for got, exp in (("a2r", c0[31]), ("a2i", c0[63]), ("a3r", c0[31]), ("a3i", c0[63]), ("a3b", c1[31])):
        assert (o[got].view(np.uint32) == exp.view(np.uint32)).all(), (got, o[got][:4], exp)
    # the trees are sums: close to the float64 sum of the inputs (a wrong lane pattern that is still a tree would pass
    # the emulation only if the emulation had the same mistake)
    assert abs(float(c0[31]) - i["yr"].astype(np.float64).sum()) <= 64 * 2.0 ** -24 * np.abs(i["yr"]).astype(np.float64).sum()
    assert abs(float(c0[63]) - i["yi"].astype(np.float64).sum()) <= 64 * 2.0 ** -24 * np.abs(i["yi"]).astype(np.float64).sum()
    assert abs(float(c1[31]) - i["bb"].astype(np.float64).sum()) <= 64 * 2.0 ** -24 * np.abs(i["bb"]).astype(np.float64).sum()
