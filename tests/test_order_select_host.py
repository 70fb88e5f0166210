"""Without a GPU: the host side of passiveradar_amd/csrc/order_select.h, reached through tests/csrc/libosselhost.so.

Keys: prc_okey / prc_okey_raw map floats to unsigned integers in the floats' own order and prc_key_value maps them back
bit for bit; prc_okey takes -0 as +0 (the display limits, the tracker's threshold and plot extraction rank values, as
np.sort does), prc_okey_raw keeps -0 below +0 (OS-CFAR hands the selected key back as its noise estimate, which may be -0).
Ranks: prc_percentile_rank is NumPy's linear percentile, floor and fraction of (n-1) * (p/100) in float64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")

# (float type, key type, entry point suffix)
FORMS = {"f32": (np.float32, np.uint32, "f32"), "f64": (np.float64, np.uint64, "f64")}


@pytest.fixture(scope="module")
def host():
    lib = os.path.join(HERE, "libosselhost.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-C", HERE, "libosselhost.so"])
    h = ctypes.CDLL(lib)
    for sfx in ("f32", "f64"):
        for name in ("osh_okey_", "osh_okey_raw_", "osh_key_value_"):
            fn = getattr(h, name + sfx)
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    h.osh_percentile_rank.restype = None
    h.osh_percentile_rank.argtypes = [ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]

    def call(name, x, out_dtype):
        x = np.ascontiguousarray(x)
        out = np.empty(x.shape, out_dtype)
        getattr(h, name)(x.ctypes.data, out.ctypes.data, x.size)
        return out
    call.lib = h
    return call


def _vector(ft):
    """±0, ±smallest denormal, ±1, ±max, ±inf, a quiet NaN and 1000 seeded normals"""
    fi = np.finfo(ft)
    special = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, 1.0, -1.0, fi.max, -fi.max, np.inf, -np.inf, np.nan]
    rng = np.random.default_rng(680)
    return np.concatenate([np.array(special, ft), rng.standard_normal(1000).astype(ft)])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_keys_keep_the_order_and_come_back_bit_for_bit(host, form):
    ft, kt, sfx = FORMS[form]
    x = _vector(ft)
    bits = x.view(kt)
    neg_zero = np.array(-0.0, ft).view(kt)
    assert (bits == neg_zero).sum() == 1 and np.isnan(x).sum() == 1
    key = host("osh_okey_" + sfx, x, kt)
    raw = host("osh_okey_raw_" + sfx, x, kt)
    # the round trip: every bit pattern (NaN included) comes back, but for -0 through the folding key
    back = host("osh_key_value_" + sfx, key, ft).view(kt)
    assert np.array_equal(back, np.where(bits == neg_zero, kt(0), bits))
    assert np.array_equal(host("osh_key_value_" + sfx, raw, ft).view(kt), bits)
    # the two zeros
    z = np.array([-0.0, 0.0], ft)
    kz, rz = host("osh_okey_" + sfx, z, kt), host("osh_okey_raw_" + sfx, z, kt)
    assert kz[0] == kz[1] and rz[0] < rz[1] and rz[1] == kz[1]
    # off -0 the two keys are one
    assert np.array_equal(key[bits != neg_zero], raw[bits != neg_zero])
    # sorting by key is np.sort on the finite values and the infinities (values compared: the zeros are equal there) ...
    ordered = x[~np.isnan(x)]
    for k in (key, raw):
        assert np.array_equal(ordered[np.argsort(k[~np.isnan(x)], kind="stable")], np.sort(ordered))
    # ... and the raw key also puts -0 before +0
    by_raw = ordered[np.argsort(raw[~np.isnan(x)], kind="stable")]
    zeros = by_raw[by_raw == 0]
    assert np.signbit(zeros).tolist() == [True, False]
    # a quiet NaN (sign clear) is just a key: above +inf
    assert key[np.isnan(x)][0] > key[x == np.inf][0]


@pytest.mark.parametrize("n", [1, 2, 17, 4071, 181248])
@pytest.mark.parametrize("p", [0, 35, 50, 99, 100])
def test_percentile_rank_is_numpys_linear_percentile(host, n, p):
    k = np.zeros(1, np.uint32)
    t = np.zeros(1, np.float64)
    host.lib.osh_percentile_rank(float(p), n, k.ctypes.data, t.ctypes.data)
    vi = np.float64(n - 1) * (np.float64(p) / np.float64(100.0))
    if vi >= n - 1:                             # at or above the last index: the last order statistic, no fraction
        exp_k, exp_t = n - 1, np.float64(0.0)
    else:
        exp_k, exp_t = int(np.floor(vi)), vi - np.floor(vi)
    assert int(k[0]) == exp_k and t[0] == exp_t, (n, p, int(k[0]), t[0], exp_k, exp_t)
    assert 0 <= k[0] <= n - 1 and 0.0 <= t[0] < 1.0
    # and with it np.percentile itself, on data whose order statistics are their own indices
    a, b = float(k[0]), float(min(int(k[0]) + 1, n - 1))
    d = b - a
    lerp = b - d * (1.0 - t[0]) if t[0] >= 0.5 else a + d * t[0]
    assert lerp == np.percentile(np.arange(n, dtype=np.float64), p)
