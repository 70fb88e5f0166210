"""Every size limit of include/prcore.h, without a GPU: the first refused value is refused with the documented status and a
message that names the argument and the limit; the largest accepted value is not refused for its size; a refused plan
create returns before the plan exists ("64-bit sizes", has the audit this table follows).

The checks precede any launch and any allocation, so fake (aligned, non-null) addresses do, as in
tests/test_channelize_host.py and tests/test_echo_host.py.  The accepted side is exercised only where it needs no device: on
the *_workspace_bytes twin that runs the same check, on a call with nothing to do, or -- plan creates and the entry points that
would launch -- on a call whose sizes are at the limit and whose NEXT argument is bad: the size checks stand first, so the
call must get past them and be refused for that argument, with its status and its word.  For plan creates the order of the
checks in the source is asserted as well: an accepted create would allocate.

That every int64_t of the header is a c_int64 in passiveradar_amd/_lib.py is tests/test_abi.py."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO
from passiveradar_amd import _lib

P = 64                                       # a fake device address: aligned, never dereferenced
LS_MAX_N = CAF_MAX_N = 2 ** 29 - 2 ** 16     # PRC_LS_MAX_N, PRC_CAF_MAX_N
MAX_BATCH = 65535                            # PRC_MAX_BATCH
XCORR_MAX_N = 4096 * (2 ** 31 - 1)


def _msg():
    return _lib.lib().prc_last_error().decode()


def _create(name, desc):
    fn = getattr(_lib.lib(), name)
    h = C.c_void_p()
    rc = fn(C.byref(h), C.byref(desc))
    assert rc != _lib.PRC_OK and h.value is None          # no case here creates a plan
    return rc, _msg()


def ls_create(n=40000, max_blocks=1, method=0):
    d = _lib.LsDesc()
    d.n, d.filter_len, d.peek, d.circular, d.max_blocks, d.method = n, 16, 10, 0, max_blocks, method
    return _create("prc_ls_plan_create", d)


def caf_create(n=8192, max_frames=1, method=0, doppler=0, multi=0):
    d = _lib.CafDesc()
    d.n, d.range_bins, d.freq_bins, d.max_frames, d.method, d.doppler, d.multi = n, 7, 64, max_frames, method, doppler, multi
    return _create("prc_caf_plan_create", d)


def frontend_create(n_in=4096, max_blocks=1, raw_dtype=0):
    taps = (C.c_float * 3)(0.25, 0.5, 0.25)
    d = _lib.FrontendDesc()
    d.n_in, d.raw_dtype, d.up, d.down, d.ntaps, d.n_pre_remove, d.max_blocks = n_in, raw_dtype, 1, 2, 3, 0, max_blocks
    d.taps_host = C.cast(taps, C.POINTER(C.c_float))
    return _create("prc_frontend_plan_create", d)


def svd_bytes(n=4096, nblocks=1):
    b = C.c_size_t(0)
    return _lib.lib().prc_ls_svd_workspace_bytes(n, 16, 10, nblocks, C.byref(b)), _msg()


def svd_execute(n=4096, nblocks=1):
    rc = _lib.lib().prc_ls_svd_execute(P, P, n, n, 16, 10, -1.0, nblocks, P, n, None, None, None, P, None)
    return rc, _msg()


def eca_bytes(n=4096, nblocks=1):
    b = C.c_size_t(0)
    return _lib.lib().prc_eca_workspace_bytes(n, 16, 10, 2, nblocks, C.byref(b)), _msg()


def eca_execute(n=4096, nblocks=1):
    bins = (C.c_double * 2)(0.0, 1.0)
    rc = _lib.lib().prc_eca_execute(P, P, n, n, 16, 10, 1e4, bins, 2, 0.0, nblocks, P, n, None, None, P, None)
    return rc, _msg()


def _echo_desc(n, nframes):
    d = _lib.EchoDesc()
    d.n, d.frame_stride, d.out_stride, d.nframes, d.max_atoms, d.wrap, d.ramp, d.refine = n, n, n, nframes, 2, 1, 0, 0
    d.sample_rate, d.reg = 1e4, 0.0
    return d


def echo_bytes(n=4096, nframes=1):
    b = C.c_size_t(0)
    return _lib.lib().prc_echo_cancel_workspace_bytes(C.byref(_echo_desc(n, nframes)), C.byref(b)), _msg()


def echo_cancel(n=4096, nframes=1):
    return _lib.lib().prc_echo_cancel(C.byref(_echo_desc(n, nframes)), P, P, P, P, P, P, P, P, None), _msg()


def firdec(nch=1):
    """n = 0 is the documented no-op: every check runs, nothing is launched"""
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix = 2, 41, 0, 0
    return _lib.lib().prc_fir_decimate(C.byref(d), P, P, 0, 1, 0, nch, P, 1, 0, None), _msg()


def xcorr(n, out=P):
    return _lib.lib().prc_xcorr(P, P, n, 8, 8, out, None), _msg()


def welch(nch, n=64 << 20, out=P):
    """rows of one 64-point segment each (2^20 of them at the default n): nch * rows workgroups"""
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.in_dtype, d.step, d.scale = 64, 0, 1, 0, 4, 1, 1.0
    return _lib.lib().prc_welch(C.byref(d), P, None, n, n, nch, P, out, P, None), _msg()


def cfar2d(nframes, X=P, c64=False):
    fn = _lib.lib().prc_cfar2d_c64 if c64 else _lib.lib().prc_cfar2d
    return fn(X, 64, 64, 18, 4, 0, 0.0, P, nframes, None), _msg()


def display_limits(frame_elems):
    """nframes = 0 is the documented no-op"""
    return _lib.lib().prc_display_limits(P, 0, frame_elems, 0, 1.0, 99.0, 1.0, P, None), _msg()


def persistence(frame_elems=16, k_count=1, out=P):
    return _lib.lib().prc_persistence(P, 0, frame_elems, k_count, 0, k_count, 2, 0.5, out, 0, None), _msg()


E = {"EINVAL": _lib.PRC_EINVAL, "ESHAPE": _lib.PRC_ESHAPE, "EUNSUPPORTED": _lib.PRC_EUNSUPPORTED}

OK = ("OK", "")

# id, refused call, status, words the message holds, the call at the limit, (the status it ends with, a word of its message)
LIMITS = [
    ("ls_plan_n", lambda: ls_create(n=LS_MAX_N + 1), "ESHAPE", ("n = %d" % (LS_MAX_N + 1), str(LS_MAX_N)),
     lambda: ls_create(n=LS_MAX_N, method=9), ("EINVAL", "method 9")),
    ("ls_plan_max_blocks", lambda: ls_create(max_blocks=MAX_BATCH + 1), "ESHAPE", ("max_blocks = 65536", "65535"),
     lambda: ls_create(max_blocks=MAX_BATCH, method=9), ("EINVAL", "method 9")),
    ("caf_plan_n", lambda: caf_create(n=CAF_MAX_N + 1), "ESHAPE", ("n = %d" % (CAF_MAX_N + 1), str(CAF_MAX_N)),
     lambda: caf_create(n=CAF_MAX_N, multi=9), ("EINVAL", "multi mode 9")),
    ("caf_plan_max_frames_direct", lambda: caf_create(max_frames=MAX_BATCH + 1, method=1), "ESHAPE", ("max_frames = 65536", "65535"),
     lambda: caf_create(max_frames=MAX_BATCH, method=1, doppler=7), ("EINVAL", "Doppler method 7")),
    ("caf_plan_max_frames_fft1024", lambda: caf_create(max_frames=MAX_BATCH + 1, method=2), "ESHAPE", ("max_frames = 65536", "65535"),
     lambda: caf_create(max_frames=MAX_BATCH, method=2, doppler=7), ("EINVAL", "Doppler method 7")),
    ("frontend_plan_n_in", lambda: frontend_create(n_in=2 ** 30), "EINVAL", ("n_in = 1073741824", "2^30 - 1"),
     lambda: frontend_create(n_in=2 ** 30 - 1, raw_dtype=9), ("EINVAL", "raw dtype 9")),
    ("frontend_plan_max_blocks", lambda: frontend_create(max_blocks=MAX_BATCH + 1), "ESHAPE", ("max_blocks = 65536", "65535"),
     lambda: frontend_create(max_blocks=MAX_BATCH, raw_dtype=9), ("EINVAL", "raw dtype 9")),
    ("ls_svd_n", lambda: svd_execute(n=2 ** 31), "ESHAPE", ("n = 2147483648", "2147483647"), lambda: svd_bytes(n=2 ** 31 - 1), OK),
    ("ls_svd_bytes_n", lambda: svd_bytes(n=2 ** 31), "ESHAPE", ("n = 2147483648", "2147483647"), lambda: svd_bytes(n=2 ** 31 - 1), OK),
    ("ls_svd_nblocks", lambda: svd_execute(nblocks=MAX_BATCH + 1), "ESHAPE", ("nblocks = 65536", "65535"),
     lambda: svd_bytes(nblocks=MAX_BATCH), OK),
    ("eca_n", lambda: eca_execute(n=2 ** 31), "ESHAPE", ("n = 2147483648", "2147483647"), lambda: eca_bytes(n=2 ** 31 - 1), OK),
    ("eca_bytes_n", lambda: eca_bytes(n=2 ** 31), "ESHAPE", ("n = 2147483648", "2147483647"), lambda: eca_bytes(n=2 ** 31 - 1), OK),
    ("eca_nblocks", lambda: eca_execute(nblocks=MAX_BATCH + 1), "ESHAPE", ("nblocks = 65536", "65535"),
     lambda: eca_bytes(nblocks=MAX_BATCH), OK),
    ("echo_n", lambda: echo_cancel(n=2 ** 31), "ESHAPE", ("n = 2147483648", "2^31"), lambda: echo_bytes(n=2 ** 31 - 1), OK),
    ("echo_nframes", lambda: echo_cancel(nframes=MAX_BATCH + 1), "ESHAPE", ("nframes = 65536", "65535"),
     lambda: echo_bytes(nframes=MAX_BATCH), OK),
    ("fir_decimate_nch", lambda: firdec(nch=MAX_BATCH + 1), "EINVAL", ("nch = 65536", "65535"), lambda: firdec(nch=MAX_BATCH), OK),
    ("cfar2d_nframes", lambda: cfar2d(MAX_BATCH + 1), "ESHAPE", ("nframes = 65536", "65535"),
     lambda: cfar2d(MAX_BATCH, X=None), ("EINVAL", "null")),
    ("cfar2d_c64_nframes", lambda: cfar2d(MAX_BATCH + 1, c64=True), "ESHAPE", ("nframes = 65536", "65535"),
     lambda: cfar2d(MAX_BATCH, X=None, c64=True), ("EINVAL", "null")),
    ("xcorr_n", lambda: xcorr(XCORR_MAX_N + 1), "ESHAPE", ("n = %d" % (XCORR_MAX_N + 1), str(XCORR_MAX_N)),
     lambda: xcorr(XCORR_MAX_N, out=None), ("EINVAL", "null")),
    ("welch_rows", lambda: welch(2048), "EUNSUPPORTED", ("2147483648 output rows", "limit 2147483647"),
     lambda: welch(1, n=64 * (2 ** 31 - 1), out=None), ("EINVAL", "null")),
    ("display_limits_frame_elems", lambda: display_limits(2 ** 31), "EINVAL", ("frame_elems",), lambda: display_limits(2 ** 31 - 1), OK),
    ("persistence_frame_elems", lambda: persistence(frame_elems=256 * (2 ** 31 - 1) + 1), "EINVAL",
     ("frame_elems = %d" % (256 * (2 ** 31 - 1) + 1), str(256 * (2 ** 31 - 1))),
     lambda: persistence(frame_elems=256 * (2 ** 31 - 1), out=None), ("EINVAL", "null out")),
    ("persistence_k_count", lambda: persistence(k_count=8 * MAX_BATCH + 1), "EINVAL", ("k_count = 524281", "524280"),
     lambda: persistence(k_count=8 * MAX_BATCH, out=None), ("EINVAL", "null out")),
]


@pytest.mark.parametrize("refused,status,words,at_limit,then", [c[1:] for c in LIMITS], ids=[c[0] for c in LIMITS])
def test_limit(refused, status, words, at_limit, then):
    rc, msg = refused()
    assert rc == E[status], (rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    rc, msg = at_limit()
    if then is OK:
        assert rc == _lib.PRC_OK, (rc, msg)
    else:
        assert rc == E[then[0]] and then[1] in msg, (rc, msg)
        assert not any(w in msg for w in words[:1]), msg            # and not for its size


def test_the_4096_point_caf_method_takes_any_frame_count():
    """the 4096-point kernels spread the frames over grid.x: 65536 frames are not refused for their number (the create ends at
    the unknown Doppler method, the check after the size checks)"""
    d = _lib.CafDesc()
    d.n, d.range_bins, d.freq_bins, d.max_frames, d.method, d.doppler = 8192, 70, 2, MAX_BATCH + 1, 3, 7
    rc, msg = _create("prc_caf_plan_create", d)
    assert rc == _lib.PRC_EINVAL and "Doppler method 7" in msg, (rc, msg)


def _body(path, signature):
    """the text of one function of a source file, from its signature to the first line that closes it"""
    text = open(os.path.join(REPO, "passiveradar_amd", "csrc", path)).read()
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


@pytest.mark.parametrize("path,signature,limits,made", [
    ("ls.hip", "static int ls_plan_create_impl(", ("PRC_LS_MAX_N", "PRC_MAX_BATCH"), "new prc_ls_plan()"),
    ("caf.hip", 'extern "C" int prc_caf_plan_create(', ("PRC_CAF_MAX_N",), "new prc_caf_plan()"),
    ("frontend.hip", 'extern "C" int prc_frontend_plan_create(', ("1 << 30", "PRC_MAX_BATCH"), "new prc_frontend_plan()"),
])
def test_a_refused_plan_create_returns_before_the_plan_exists(path, signature, limits, made):
    """every size check stands before the `new` of the plan, and no device allocation stands before that (caf.hip: 'every
    argument check comes before the plan exists')"""
    body = _body(path, signature)
    at = body.index(made)
    for word in limits:
        checks = [m.start() for m in re.finditer(re.escape(word), body)]
        assert checks and min(checks) < at, (path, word)
    assert "hipMalloc" not in body[:at] and "rocfft_plan_create" not in body[:at]


def test_the_constants_match_the_header(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "lim.c"
    src.write_text('#include <stdio.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  printf("%lld %lld %d\\n", (long long)PRC_LS_MAX_N, (long long)PRC_CAF_MAX_N, PRC_MAX_BATCH); return 0; }\n')
    exe = tmp_path / "lim"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [LS_MAX_N, CAF_MAX_N, MAX_BATCH]
