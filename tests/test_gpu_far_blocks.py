"""Blocks, frames and channels more than 4 GiB apart: every strided entry point of include/prcore.h with block 1 of each
argument FAR(itemsize) = 2^32 // itemsize + 4099 elements beyond block 0 -- more than 2^32 bytes and an odd number of elements
on -- and every dense stack long enough for its last frame to begin beyond 2^32 bytes ("64-bit sizes", has the
audit these cases follow and their measured times and memory).

Strided arguments run through tests/guard.py as it is, two blocks of the smallest payload the entry point's own bounds test
uses: guard.check asserts that every promised element is written and finite, that no sentinel in the 4 GiB between the blocks
changed, and that the payload equals the tight call's bit for bit; the tight call is then held to the oracle at the entry
point's own bar.  The cases call the per-entry helpers and test bodies of the bounds modules with the far gap.

Dense stacks [nframes][H][W] hold device-generated noise in the middle frames.  Frame 0 and the last frame must equal, bit for
bit, the same two frames run as a two-frame call (a frame's bytes do not depend on its position or its neighbours), and the
last frame of that call is held to the kind's oracle at its own bar.  prc_tbd and prc_persistence, whose frames do depend on
earlier ones, are checked through their own recursions.

Every case says what it allocates before it does, skips below that plus 8 GiB of free device memory (none skips on an idle
MI355X) and leaves the device memory as it found it."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import guard
from conftest import rel_err
from passiveradar_amd import _lib, engine

pytestmark = pytest.mark.gpu

GiB = 1 << 30


def FAR(itemsize):
    return 2 ** 32 // itemsize + 4099


FAR8 = FAR(8)          # complex64 elements
FARP = FAR(2)          # int8 I/Q pairs: the element a stride of the raw types counts


@pytest.fixture(autouse=True)
def _clean(gpu_ready, request):
    """a HIP fault is sticky: if an earlier case left one, nothing more is started on the device (tests/test_gpu_bounds.py)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reports a fault from an earlier case, stopping: {e}", returncode=3)
    torch.cuda.reset_peak_memory_stats()
    try:
        yield
    finally:
        print(f"\n[{request.node.name}: peak {torch.cuda.max_memory_allocated() / GiB:.1f} GiB of tensors]")
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def need(gib):
    """skip unless ``gib`` GiB (what the case allocates at its peak) plus 8 GiB are free"""
    assert gib <= 40
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < (gib + 8) * GiB:
        pytest.skip(f"needs {gib} GiB + 8 GiB of device memory, {free / GiB:.1f} GiB are free")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- strided entry points through tests/guard.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("method,n,R,F,team8", [(1, 5000, 4, 51, None), (2, 8192, 70, 128, None), (3, 8192, 70, 2, 0),
                                                (3, 8192, 70, 2, 1)], ids=["direct", "fft1024", "team4", "team8"])
def test_caf_frame_stride(method, n, R, F, team8):
    import test_gpu_bounds as B
    need(14)           # ref, srv: 4 GiB each, guarded; the rest is small
    import contextlib
    with B._option(_lib.OPT_CAF_TEAM8, team8) if team8 is not None else contextlib.nullcontext():
        plan = engine.CafPlan(n, R, F, 2, method=method)
        try:
            assert plan.method == method
            B._caf_check(plan, n, R, F, FAR8, np.kaiser(n, 5.0), n, 100 + n + R, nf=2)
        finally:
            plan.close()


def test_caf_multi_frame_stride():
    import test_gpu_bounds as B
    need(22)           # three references and the surveillance channel, 4 GiB each
    B._caf_multi_check(65536, 1024, 8, 3, 0, None, "shared", [(FAR8, True)], NF=2)


@pytest.mark.parametrize("method,n,L", [(1, 4000, 16), (2, 40000, 64), (3, 40000, 64), (4, 40000, 128)],
                         ids=lambda v: str(v))
def test_ls_strides(method, n, L):
    """stride and out_stride both far and different; the single bin and, where the method has a cached chain, five bins"""
    import test_gpu_bounds as B
    from oracle import np_oracle as O
    need(20)           # ref, srv, out: 4 GiB each, and the masks of guard.report over out
    T = L + 10
    ref, srv = B._ls_scene(n, L, 4000 + n + L + method, 2)
    plan = engine.LsPlan(n, L, 10, False, 2, method)
    try:
        out, taps = B._ls_check(plan, n, T, (0,), FAR8, ref, srv)
        exp, etaps = O.LS_Filter_Toeplitz(ref[1], srv[1], L, 10, True)
        assert rel_err(taps[1], etaps) < B.TIGHT and rel_err(out[1], exp) < B.TIGHT
        if method >= 3:
            out, _ = B._ls_check(plan, n, T, B.FIVE, FAR8, ref, srv)
            assert rel_err(out[1], O.LS_Filter_Multiple(ref[1], srv[1], L, 1.0e4, list(B.FIVE))) < B.TOL
    finally:
        plan.close()


@pytest.mark.parametrize("L", [24, 8300])
def test_nlms_strides(L):
    import test_gpu_bounds as B
    need(20)
    B._nlms_check(L, gaps=(FAR8,), NS=2)


def test_gal_strides():
    import test_gpu_bounds as B
    need(20)
    B._gal_check(64, 8, gaps=(FAR8,), NS=2)


def test_ls_svd_strides():
    import test_gpu_ls_svd as S
    need(20)
    S.test_guard_bands(FAR8)


def test_eca_strides():
    import test_gpu_ls_eca as E
    need(20)
    E.test_guard_bands(FAR8)


@pytest.mark.parametrize("method", [0, 1], ids=["group", "per_thread"])
@pytest.mark.parametrize("dt", ["int8", "complex64"])
def test_front_end_strides(dt, method):
    """prc_frontend_execute and _execute2 at 13:119, raw_stride and out_stride far; integer raw runs with both gap fills"""
    import test_gpu_bounds as B
    need(36 if dt == "int8" else 22)       # a, b: 4 GiB each; oa, ob: 4 GiB each, twice for the two fills of integer raw
    up, dn, nb = 13, 119, 2
    n_in = 64 * dn + 37
    width = 1 if dt == "complex64" else 2
    gap = FAR(8 if dt == "complex64" else 1)
    rng = np.random.default_rng(up * 100 + dn)
    plan = engine.FrontendPlan(n_in, dt, up, dn, nb)
    try:
        n_out = plan.n_out
        ra, rb = B._raw(rng, dt, (nb, n_in)), B._raw(rng, dt, (nb, n_in))
        from oracle import np_oracle as O
        phases = O.block_phase_offsets(nb, 2 * n_in, B.FE_FS, B.FE_FOFF)
        ins = {"a": guard.In(dev(ra), width * n_in + gap), "b": guard.In(dev(rb), width * n_in + gap)}
        one = {"out": guard.Out(nb, n_out, torch.complex64, n_out + FAR8)}
        two = {"oa": guard.Out(nb, n_out, torch.complex64, n_out + FAR8), "ob": guard.Out(nb, n_out, torch.complex64, n_out + FAR8)}

        def run1(a, s):
            plan.execute(a["a"], a["out"], nb, s["a"], s["out"], B.FE_FOFF, B.FE_FS, phases, True)
            B._sync()

        def run2(a, s):
            plan.execute2(a["a"], a["b"], a["oa"], a["ob"], nb, s["a"], s["oa"], B.FE_FOFF, B.FE_FS, phases, True)
            B._sync()
        with B._option(_lib.OPT_FE_METHOD, method):
            first = guard.check(run1, {"a": ins["a"]}, one).tight["out"].clone()
            torch.cuda.empty_cache()
            g2 = guard.check(run2, ins, two)
        assert torch.equal(g2.tight["oa"], first)
        e = rel_err(B._host(g2.tight["ob"])[1], B._fe_oracle(rb[1], dt, True, up, dn, phases[1]))
        assert e < B.TIGHT, e
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", ["complex64", "int8"])
def test_welch_stride(gpu_ready, dtype):
    import test_gpu_psd as W
    need(16)
    W.test_guard_bands(gpu_ready, dtype, False, nfft=64, gap=FAR8 if dtype == "complex64" else FARP)


@pytest.mark.parametrize("q", [10, _lib.FIRDEC_TILE_MAX_Q + 1], ids=["tile", "direct"])
def test_fir_decimate_strides(gpu_ready, q):
    import test_gpu_preproc as P
    need(24)           # x: 4 GiB of int8, out: 4 GiB, each twice for the two gap fills
    P.test_guard_bands_fir_decimate(gpu_ready, q, 1, gap=FAR8, far_in=FARP)


def test_fir_decimate_steps_past_4gib():
    """one int8 channel whose samples lie 2^20 + 1 pairs apart and whose outputs 2^21 + 1 elements apart: the last sample is
    at byte 8.8e9 and the last output at byte 7.0e9.  Bit for bit the dense call's outputs, which are held to the oracle."""
    import preproc_oracle as O
    lib = _lib.lib()
    n, q, step, ostep = 4200, 10, 2 ** 20 + 1, 2 ** 21 + 1
    m = O.out_len(n, q)
    need((2 * (n - 1) * step + 3 * 8 * (m - 1) * ostep) / GiB + 1)      # the recording; out, and the masks and copies of its comparison
    assert 2 * (n - 1) * step > 2 ** 32 and 8 * (m - 1) * ostep > 2 ** 32
    raw = O.raw_int8(2 * n, 97)
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix, d.fc, d.fs = q, 20 * q + 1, _lib.RAW_DTYPES["int8"], 1, 1e5, 2.4e6
    taps = dev(O.taps32(q))
    st = _lib.torch_stream_ptr()
    sentinel = complex(7.0, -3.0)
    big = torch.full((2 * ((n - 1) * step + 1),), 127, dtype=torch.int8, device="cuda")
    big.view(-1, 2)[::step] = dev(raw.reshape(-1, 2))
    out = torch.full(((m - 1) * ostep + 1,), sentinel, dtype=torch.complex64, device="cuda")
    _lib.check(lib.prc_fir_decimate(C.byref(d), taps.data_ptr(), big.data_ptr(), n, step, 0, 1, out.data_ptr(), ostep, 0, st))
    dense = torch.empty(m, dtype=torch.complex64, device="cuda")
    _lib.check(lib.prc_fir_decimate(C.byref(d), taps.data_ptr(), dev(raw).data_ptr(), n, 1, 0, 1, dense.data_ptr(), 1, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(out[::ostep]), torch.view_as_real(dense))
    written = int((torch.view_as_real(out) != torch.view_as_real(torch.full((1,), sentinel, dtype=torch.complex64, device="cuda"))).any(dim=1).sum())
    assert written == m                                              # and nothing between the outputs
    assert rel_err(dense.cpu().numpy(), O.fir_decimate(O.tuned(raw, 1e5, 2.4e6), q)) <= 4e-6          # tests/test_gpu_preproc.py's bar


@pytest.mark.parametrize("form", ["tile", "direct"])
def test_channelize_out_stride(form):
    import channelize_oracle as O
    need(20)           # out: two rows 4 GiB apart, twice (channels is an integer argument: two gap fills)
    lib = _lib.lib()
    st = _lib.torch_stream_ptr()
    M, D, CH = 12, 10, [1, -5]
    L = 20 * D + 1
    n = O.TILE_OUTPUTS * D + 1
    cs, sn = O.twiddles32(M)
    tw = (cs + 1j * sn).astype(np.complex64)
    x = O.case_input(n, M, D, "int8")
    m = O.out_len(n, D)
    d = _lib.ChannelizeDesc()
    d.nchan, d.dec, d.ntaps, d.raw_dtype, d.nsel, d.start = M, D, L, _lib.RAW_DTYPES["int8"], len(CH), 7
    old = _lib.set_option(_lib.OPT_CHANNELIZE_FORM, int(form == "direct"))
    try:
        def run(a, s):
            _lib.check(lib.prc_channelize(C.byref(d), a["taps"].data_ptr(), a["twiddles"].data_ptr(), a["channels"].data_ptr(),
                                          a["x"].data_ptr(), n, a["out"].data_ptr(), s["out"], st))
            torch.cuda.synchronize()
        ins = {"x": guard.In(dev(x).reshape(1, -1)), "taps": guard.In(dev(O.taps32(D)).reshape(1, -1)),
               "twiddles": guard.In(dev(tw).reshape(1, -1)), "channels": guard.In(dev(np.array(CH, np.int32)).reshape(1, -1))}
        got = guard.check(run, ins, {"out": guard.Out(len(CH), m, torch.complex64, stride=m + FAR8)})
        err = O.rel_err(got.tight["out"].cpu().numpy(), O.channelize(x, M, D, CH, start=7))
        assert err <= O.GPU_BAR, (form, err)
    finally:
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, old)


def test_xambg_patch_frame_stride(gpu_ready):
    import test_gpu_patch_bounds as P
    need(14)
    P.test_guard_bands_patch(gpu_ready, 4096, True, gap=FAR8)


def test_echo_cancel_strides(gpu_ready):
    import test_gpu_echo_bounds as E
    need(20)
    E.test_echo_cancel_guard_bands(gpu_ready, True, NF=2, STRIDE=E.N + FAR8, OUT_STRIDE=E.N + FAR8 + 16)


# ---- dense stacks: the last frame begins beyond 2^32 bytes ------------------------------------------------------------------
def frames_past_4gib(cells, itemsize):
    """frames of ``cells`` elements so that the last one begins beyond 2^32 bytes"""
    return 2 ** 32 // (cells * itemsize) + 2


def noise_stack(nf, cells, dtype, first, last, seed):
    """[nf][cells] on the device: seeded noise in the middle, the two given host frames at the ends"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.complex64:
        x = torch.view_as_complex(torch.randn((nf, cells, 2), generator=g, device="cuda", dtype=torch.float32))
    else:
        x = torch.rand((nf, cells), generator=g, device="cuda", dtype=dtype) + 0.05
    x[0], x[nf - 1] = dev(first).reshape(-1), dev(last).reshape(-1)
    return x


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def test_caf_out_stack():
    """prc_caf_execute with so many overlapped frames (hop 64) that the last surface of out begins beyond 2^32 bytes: the 1024-point
    kernels, whose frames are grid.y, just below PRC_MAX_BATCH.  Every surface is finite; the first and the last are held to
    the oracle at the bounds test's bar"""
    import test_gpu_bounds as B
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    n, R, Fb, hop = 8192, 70, 128, 64
    surf = Fb * (R + 1)
    nf = 2 ** 32 // (surf * 8) + 2
    assert nf <= 65535 and (nf - 1) * surf * 8 > 2 ** 32
    need(4 * nf * surf * 8 / GiB + 2)      # out, the plan's two slow-time buffers of the same size, the mask of isfinite
    ref, srv = scene.make_scene((nf - 1) * hop + n, 1e4, 70, 4242)
    plan = engine.CafPlan(n, R, Fb, nf, method=2)
    try:
        out = torch.full((nf, Fb, R + 1), float("nan"), dtype=torch.complex64, device="cuda")
        plan.execute(dev(ref), dev(srv), out, nf, hop, n, None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(torch.view_as_real(out)).all())
        for b in (0, nf - 1):
            exp = O.fast_xambg(ref[b * hop:b * hop + n], srv[b * hop:b * hop + n], R, Fb, n, None, True)[:, :, 0]
            e = rel_err(out[b].cpu().numpy(), exp)
            assert e < B.TIGHT, (b, e)
    finally:
        plan.close()


@pytest.mark.parametrize("cplx", [False, True], ids=["f32", "c64"])
def test_cfar2d_stack(cplx):
    from oracle import np_oracle as O
    H, W, fw, gw = 509, 1031, 18, 4
    cells = H * W
    nf = frames_past_4gib(cells, 8 if cplx else 4)
    need((2 * (8 if cplx else 4) + 2 * 4 + 1) * nf * cells / GiB + 1)      # X and the noise it is made from, out, its copy and masks
    rng = np.random.default_rng(61)
    ends = (rng.standard_normal((2, H, W)) + 1j * rng.standard_normal((2, H, W))).astype(np.complex64)
    ends[1, H // 2, W // 3] += 1e3
    if not cplx:
        ends = np.abs(ends).astype(np.float32)
    X = noise_stack(nf, cells, torch.complex64 if cplx else torch.float32, ends[0], ends[1], 62)
    assert (nf - 1) * cells * X.element_size() > 2 ** 32
    fn = _lib.lib().prc_cfar2d_c64 if cplx else _lib.lib().prc_cfar2d
    out = torch.full((nf, cells), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(fn(X.data_ptr(), H, W, fw, gw, 0, 0.0, out.data_ptr(), nf, _lib.torch_stream_ptr()))
    two_in = dev(ends.reshape(2, -1))
    two = torch.full((2, cells), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(fn(two_in.data_ptr(), H, W, fw, gw, 0, 0.0, two.data_ptr(), 2, _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(out[0]), bits(two[0])) and torch.equal(bits(out[nf - 1]), bits(two[1]))
    assert bool(torch.isfinite(out).all())
    assert rel_err(two[1].cpu().numpy().reshape(H, W), O.CFAR_2D(np.abs(ends[1]).astype(np.float32), fw, gw)) < 2e-5


def test_cfar_os_stack():
    import cfar_os_oracle as CO
    import test_gpu_cfar_os as TC
    H, W, fw, gw = 127, 131, 18, 4
    cells = H * W
    nf = frames_past_4gib(cells, 4)
    assert nf <= 65535
    need(14)
    rng = np.random.default_rng(63)
    ends = rng.exponential(1.0, (2, H, W)).astype(np.float32)
    X = noise_stack(nf, cells, torch.float32, ends[0], ends[1], 64)
    d = engine.cfar_os_desc(H, W, fw, gw, scale="reference")

    def call(x, n):
        out = torch.full((n, cells), float("nan"), dtype=torch.float32, device="cuda")
        noise = torch.full((n, cells), float("nan"), dtype=torch.float32, device="cuda")
        ws = torch.empty(max(engine.cfar_os_workspace_bytes(d, n), 4), dtype=torch.uint8, device="cuda")
        engine.cfar_os_execute(d, x, out, noise, n, ws, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        return out, noise
    out, noise = call(X, nf)
    two, two_noise = call(dev(ends.reshape(2, -1)), 2)
    for a, b in ((out, two), (noise, two_noise)):
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[nf - 1]), bits(b[1]))
    want, z = CO.CFAR_2D_OS(ends[1], fw, gw, return_noise=True)
    assert np.array_equal(two_noise[1].cpu().numpy().reshape(H, W), z)                  # the order statistic is exact
    assert rel_err(two[1].cpu().numpy().reshape(H, W), want) < TC.TIGHT


def test_display_stack():
    """prc_display_limits and prc_display_rgba chained on one stream: limits [nf][2], pixels [nf][H][W][4]"""
    import display_oracle as DO
    H, W = 509, 1031
    cells = H * W
    nf = frames_past_4gib(cells, 4)
    need(12)
    rng = np.random.default_rng(65)
    ends = rng.exponential(1.0, (2, H, W)).astype(np.float32)
    X = noise_stack(nf, cells, torch.float32, ends[0], ends[1], 66)
    lib, st = _lib.lib(), _lib.torch_stream_ptr()

    def call(x, n):
        lim = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
        px = torch.zeros((n, cells, 4), dtype=torch.uint8, device="cuda")
        _lib.check(lib.prc_display_limits(x.data_ptr(), _lib.REAL_F32, cells, n, 35.0, 99.0, 1.5, lim.data_ptr(), st))
        _lib.check(lib.prc_display_rgba(x.data_ptr(), _lib.REAL_F32, H, W, n, lim.data_ptr(), None, _lib.DISPLAY_PLOT, px.data_ptr(), st))
        torch.cuda.synchronize()
        return lim, px
    lim, px = call(X, nf)
    lim2, px2 = call(dev(ends.reshape(2, -1)), 2)
    assert torch.equal(bits(lim[0]), bits(lim2[0])) and torch.equal(bits(lim[nf - 1]), bits(lim2[1]))
    assert torch.equal(px[0], px2[0]) and torch.equal(px[nf - 1], px2[1])
    want_lim = DO.limits(ends[1].astype(np.float64), 35, 99, 1.5)
    assert tuple(lim2[1].cpu().numpy()) == tuple(np.float64(v) for v in want_lim)
    want_px = DO.render(ends[1].astype(np.float64), lim=want_lim)
    assert np.array_equal(px2[1].cpu().numpy().reshape(W, H, 4), want_px)


def test_persistence_stack():
    """L float32 frames in, L float64 frames out (hold = 2): out[L-1] reads frames L-1 and L-2 beyond 2^32 bytes and is written
    beyond 2^33; it equals the two-frame stack's out[1] bit for bit, out[0] the one-frame stack's, both the oracle's"""
    import simple_tracker_oracle as SO
    cells = 2 ** 20 + 3
    L = frames_past_4gib(cells, 4) + 1
    need((2 * 4 + 2 * 8 + 1) * L * cells / GiB + 1)      # X and the noise it is made from, out and the copy isfinite makes, masks
    rng = np.random.default_rng(67)
    ends = rng.exponential(1.0, (3, cells)).astype(np.float32)
    X = noise_stack(L, cells, torch.float32, ends[0], ends[2], 68)
    X[L - 2] = dev(ends[1])
    lib, st = _lib.lib(), _lib.torch_stream_ptr()

    def call(x, nframes, k_first, k_count):
        out = torch.full((k_count, cells), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.prc_persistence(x.data_ptr(), _lib.REAL_F32, cells, nframes, k_first, k_count, 2, 0.9, out.data_ptr(),
                                       _lib.REAL_F64, st))
        torch.cuda.synchronize()
        return out
    out = call(X, L, 0, L)
    assert (L - 1) * cells * 4 > 2 ** 32 and bool(torch.isfinite(out).all())
    last = call(dev(ends[1:]), 2, 1, 1)
    first = call(dev(ends[:1]), 1, 0, 1)
    assert torch.equal(bits(out[L - 1]), bits(last[0])) and torch.equal(bits(out[0]), bits(first[0]))
    Xh = np.moveaxis(ends[1:].reshape(2, cells, 1), 0, 2)
    assert np.array_equal(last[0].cpu().numpy(), SO.persistence(Xh, 1, 2, 0.9)[:, 0])


def test_tbd_stack_split_before_the_last_frame():
    """prc_tbd's own property at this length: the stack run whole equals the stack split before the last frame with `prev`
    carried over (the last frames of stat and score begin beyond 2^32 bytes; back, one byte per cell, is compared whole)"""
    H, W = 509, 1031
    cells = H * W
    nf = frames_past_4gib(cells, 4)
    need(18)
    g = torch.Generator(device="cuda").manual_seed(69)
    stat = torch.rand((nf, cells), generator=g, device="cuda", dtype=torch.float32)
    d = engine.tbd_desc(H, W)
    st = _lib.torch_stream_ptr()

    def call(x, prev, n):
        score = torch.full((n, cells), float("nan"), dtype=torch.float32, device="cuda")
        back = torch.full((n, cells), 77, dtype=torch.uint8, device="cuda")
        engine.tbd_execute(d, x, None, prev, n, score, back, st)
        torch.cuda.synchronize()
        return score, back
    score, back = call(stat, None, nf)
    head, hback = call(stat, None, nf - 1)
    tail, tback = call(stat[nf - 1:], head[nf - 2], 1)
    assert torch.equal(bits(score[:nf - 1]), bits(head)) and torch.equal(back[:nf - 1], hback)
    assert torch.equal(bits(score[nf - 1]), bits(tail[0])) and torch.equal(back[nf - 1], tback[0])
    assert bool(torch.isfinite(score[nf - 1]).all()) and float(score[nf - 1].max()) > 2.0       # scores have accumulated


def test_plots_stack():
    import plots_oracle as PO
    H, W, cap = 127, 131, 256
    cells = H * W
    nf = frames_past_4gib(cells, 4)
    need(10)
    rng = np.random.default_rng(71)
    ends = rng.exponential(1.0, (2, H, W)).astype(np.float32)
    thresh, ext = 6.0, (100.0, 50.0)
    X = noise_stack(nf, cells, torch.float32, ends[0], ends[1], 72)       # the middle frames: uniform below 1.05, no detections
    d = engine.plots_desc(H, W, thresh, ext, capacity=cap)
    assert engine.plots_workspace_bytes(d, nf) == 0

    def call(x, n):
        counts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ncells = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        cands = torch.zeros((n, cap, 4), dtype=torch.float64, device="cuda")
        engine.plots_execute(d, x, None, n, counts, ncells, cands, None, None, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        return counts, ncells, cands
    counts, ncells, cands = call(X, nf)
    c2, n2, k2 = call(dev(ends.reshape(2, -1)), 2)
    for a, b in ((counts, c2), (ncells, n2), (cands, k2)):
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[nf - 1]), bits(b[1]))
    assert int(counts[1:nf - 1].abs().max()) == 0
    want = PO.plots(ends[1], thresh, ext)
    k = int(c2[1])
    assert 0 < k <= cap and k == len(want["strength"])
    got = k2[1].cpu().numpy().view(_lib.TRACK_CAND_DTYPE).reshape(cap)[:k]
    assert np.array_equal(got["strength"], want["strength"]) and np.array_equal(got["index"], want["index"])


def test_track_measure_stack():
    import tracker_oracle as TO
    from passiveradar_amd.target_detection import TrackPlan
    H, W, cap, ext = 509, 1031, 2048, [100.0, 50.0]
    cells = H * W
    nf = frames_past_4gib(cells, 4)
    need(10)
    rng = np.random.default_rng(73)
    ends = rng.exponential(1.0, (2, H, W)).astype(np.float32)
    X = noise_stack(nf, cells, torch.float32, ends[0], ends[1], 74)
    plan = TrackPlan(H, W, 4, cap, ext)

    def call(x, n):
        counts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        cands = torch.zeros((n, cap, 4), dtype=torch.float64, device="cuda")
        plan.measure(x.data_ptr(), n, counts.data_ptr(), cands.data_ptr(), _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        return counts, cands
    try:
        counts, cands = call(X, nf)
        c2, k2 = call(dev(ends.reshape(2, -1)), 2)
    finally:
        plan.close()
    for a, b in ((counts, c2), (cands, k2)):
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[nf - 1]), bits(b[1]))
    want = TO.measure(ends[1], ext)
    k = int(c2[1])
    assert k == want["count"] and 0 < k <= cap
    got = k2[1].cpu().numpy().view(_lib.TRACK_CAND_DTYPE).reshape(cap)[:k]
    assert np.array_equal(got["index"], want["idx"]) and np.array_equal(got["strength"], want["strength"])
