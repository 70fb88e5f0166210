"""Guard-band tests: no device entry point of include/prcore.h reads or writes outside its arguments, needs more than
element alignment, or depends on what a plan was used for before (the last Conventions bullet of the header).

Every case hands the entry point -- at the ``engine`` / ``_lib`` level, the NumPy drop-ins would re-stage into tight
buffers -- arguments built by tests/guard.py: one allocation ``lead | block 0 | gap | block 1 | ... | tail`` per device
pointer, lead and tail 4099 elements (an odd, element-aligned base), gaps of 1 and of 4099 elements, NaN everywhere
outside the input payload (0 and the type's maximum for integer raw types), a sentinel NaN everywhere in the outputs.
``guard.check`` then asserts (1) every promised output element is written, (2) finite, (3) no sentinel outside the
extents changed, (4) the payload is bit-identical to the same call on tight exactly-sized tensors; each test then
holds one block of the tight call to the oracle at the bar the entry point's parity test uses (5).
tests/test_guard_selftest.py shows on the CPU that each of (1)-(4) can fail.

Entry point -> test
    prc_caf_execute, prc_caf_execute_segments, prc_caf_execute_doppler   test_caf
    prc_caf_execute_multi                                                test_caf_multi
    prc_ls_execute                                                       test_ls, test_ls_circular, test_ls_ragged_tail
    prc_nlms_execute                                                     test_nlms
    prc_gal_execute                                                      test_gal
    prc_frontend_execute, prc_frontend_execute2                          test_front_end
    prc_cfar2d, prc_cfar2d_c64                                           test_cfar
    prc_xcorr                                                            test_xcorr
    prc_frequency_shift, _block, _phases                                 test_frequency_shift
    prc_deinterleave                                                     test_deinterleave
    prc_decimate_iir, prc_channel_offset                                 test_decimate_and_channel_offset
    prc_persistence                                                      test_persistence
    prc_track_measure, prc_track_run                                     test_track
    prc_strack_run                                                       test_strack
    plans and scratch reused at a smaller size                           test_leftover_*
Not covered: prc_comm_loopback and prc_gather_frames (with prc_comm_unique_id / _create / _count / _destroy), which need
more than one rank to mean anything; prc_malloc / prc_free / prc_memcpy_* / prc_memset, which are the allocator itself.

(4) is bit identity everywhere: no entry point has been shown not to be deterministic, so none falls back to a bar.

Every strided case runs the whole cross-product of strides and options: nothing is trimmed.  Wall time of this module
on one MI355X (`python -m pytest tests/test_gpu_bounds.py -q -m gpu`): 23 s for its 91 cases, the slowest 3.3 s
(test_leftover_track_plan_and_decimator) and every CAF case under 1.5 s.  That is below a tenth of the 374 s the
`-m gpu` suite took before this module (profiles/asm_identity_ablation_strip.md), about 37 s, the mark above which the
strides x options product would have to be trimmed (never the entry points or kernel paths).
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guard
from conftest import rel_err
from oracle import np_oracle as O
from passiveradar_amd import _lib, engine, scene

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the bars of tests/test_gpu_parity.py
TIGHT = 2e-5
GAPS = (1, 4099)


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    """a HIP fault is sticky: if an earlier case left one, nothing more is started on the device"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        # pytest.exit ends the WHOLE run on purpose, the other modules' tests included: every later GPU test would
        # start work on a device that has already faulted
        pytest.exit(f"the device reports a fault from an earlier case, stopping: {e}", returncode=3)
    yield


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _sync():
    torch.cuda.synchronize()


def _cplx(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@contextlib.contextmanager
def _option(option, value):
    old = _lib.set_option(option, value)
    try:
        yield
    finally:
        _lib.set_option(option, old)


def _nan_bytes(nbytes):
    """a device workspace of at least nbytes holding NaN in every float32"""
    return torch.full(((max(int(nbytes), 4) + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda")


# ---- CAF ----------------------------------------------------------------------------------------------------------------
NF = 3


@functools.lru_cache(maxsize=4)
def _caf_scene(n, n_valid, R, overlap, seed, nref, nf=NF):
    m = n // 2 * (nf + 1) if overlap else n_valid * nf
    refs, srv = scene.make_multi_scene(m, 1e4, max(min(R, 200), 1), [seed + 13 * i for i in range(nref)])
    if overlap:
        return [r[None] for r in refs], srv[None]
    return [r.reshape(nf, n_valid) for r in refs], srv.reshape(nf, n_valid)


def _caf_data(n, n_valid, R, mode, seed, nref=1, nf=NF):
    """``mode`` = "overlap": one stream, frames at n/2; else (a gap) distinct frames [nf, n_valid] cut from one scene"""
    return _caf_scene(n, n_valid, R, mode == "overlap", seed, nref, nf)


def _caf_in(x, n, n_valid, mode):
    if mode == "overlap":
        return guard.In(_dev(x))                        # no gaps: lead and tail only
    # [n_valid, frame_stride) of every frame is poison, not just the gap: those samples are taken as zero
    return guard.In(_dev(x), n + mode, n, guard.TAIL + n - n_valid)


def _caf_frame(x, n, mode, b):
    return x[0, b * (n // 2):b * (n // 2) + n] if mode == "overlap" else x[b]


def _caf_check(plan, n, R, F, mode, win, n_valid, seed, via="execute", oracle=True, nf=NF):
    """``nf`` frames of a plan made for at least as many (tests/test_gpu_far_blocks.py runs two, 4 GiB apart)"""
    refs, srv = _caf_data(n, n_valid, R, mode, seed, 1, nf)
    ins = {"ref": _caf_in(refs[0], n, n_valid, mode), "srv": _caf_in(srv, n, n_valid, mode)}
    if win is not None:
        ins["win"] = guard.In(_dev(win.astype(np.float32))[None])
    outs = {"out": guard.Out(1, nf * F * (R + 1), torch.complex64)}

    def run(a, s):
        stride = n // 2 if mode == "overlap" else s["ref"]
        if via == "execute":
            plan.execute(a["ref"], a["srv"], a["out"], nf, stride, n_valid, a.get("win"))
        else:
            plan.execute_segments(a["ref"], a["srv"], nf, stride, n_valid, a.get("win"))
            plan.execute_doppler(a["out"], nf)
        _sync()
    got = _host(guard.check(run, ins, outs).tight["out"]).reshape(nf, F, R + 1)
    if oracle:
        b = nf - 1
        exp = O.fast_xambg(_caf_frame(refs[0], n, mode, b), _caf_frame(srv, n, mode, b), R, F, n, win,
                           plan._taps is None)[:, :, 0]
        e = rel_err(got[b], exp)
        assert e < TIGHT, e
    return got


CAF_CASES = [
    # method, n, R, F, n_valid, team8 values
    (1, 5000, 4, 51, None, (None,)),            # direct: non-dividing q, rocFFT Doppler
    (1, 4096, 7, 64, None, (None,)),            # direct with the long FIR: the `longfilt` golden's shape (taps below)
    (2, 8192, 70, 128, None, (None,)),          # 1024-point
    (2, 65536, 40, 256, None, (None,)),         # 1024-point, column Doppler
    (3, 8192, 70, 2, None, (0, 1)),             # 4096-point teams, both forms from here on
    (3, 65536, 300, 16, None, (0, 1)),          # remainder piece
    (3, 131072, 2048, 32, None, (0, 1)),        # direct tail sample
    (3, 40000, 9000, 2, None, (0, 1)),          # several lag blocks, wrap inside pieces
    (3, 8192, 4000, 1, None, (0, 1)),           # everything wraps
    (3, 20000, 700, 3, 17000, (0, 1)),          # n_valid < n
    (1, 8192, 70, 128, 7000, (None,)),          # n_valid < n on the direct and the 1024-point kernels
    (2, 8192, 70, 128, 7000, (None,)),
]


@pytest.mark.parametrize("method,n,R,F,n_valid,teams", CAF_CASES,
                         ids=[f"m{c[0]}-{c[1]}-{c[2]}-{c[3]}" + (f"-valid{c[4]}" if c[4] else "") for c in CAF_CASES])
def test_caf(method, n, R, F, n_valid, teams):
    """prc_caf_execute at frame strides n + 1, n + 4099 and the overlapped n / 2, with a Kaiser window and once without;
    prc_caf_execute_segments + prc_caf_execute_doppler once.  The strides and the window do not change a frame's
    arithmetic, so the oracle is asked once per shape and window (last frame of the first run)."""
    from passiveradar_amd.range_doppler_processing import _long_taps
    taps = _long_taps(n // F) if (n, R, F) == (4096, 7, 64) else None
    kaiser = np.kaiser(n, 5.0)
    valid = n if n_valid is None else n_valid
    modes = GAPS + (("overlap",) if n_valid is None else ())       # n_valid < n: frame_stride >= n
    for team8 in teams:
        with _option(_lib.OPT_CAF_TEAM8, team8) if team8 is not None else contextlib.nullcontext():
            plan = engine.CafPlan(n, R, F, NF, method=method, taps=taps)
            assert plan.method == method
            first = team8 == teams[0]                   # (the dense tight call of the other team form: test_caf_team_vs_oracle_shapes)
            for mode in modes:
                _caf_check(plan, n, R, F, mode, kaiser, valid, 100 + n + R, oracle=first)
                first = False
            # without a window; the oracle again where it is cheap (seconds at 10^8 lag products and more)
            _caf_check(plan, n, R, F, 1, None, valid, 100 + n + R, oracle=team8 == teams[0] and n * (R + 1) < 1e8)
            _caf_check(plan, n, R, F, 4099, kaiser, valid, 100 + n + R, via="segments", oracle=False)
            plan.close()


@pytest.mark.parametrize("n,R,F,nref,method,n_valid", [
    (65536, 1024, 8, 3, 0, None),
    (131072, 2048, 32, 4, 0, None),
    (20000, 700, 3, 4, 3, 17000),
])
@pytest.mark.parametrize("mode", ["turns", "shared", "pairs"])
def test_caf_multi(n, R, F, nref, method, n_valid, mode):
    """prc_caf_execute_multi: every reference channel, the surveillance channel, the window and each outs[i] guarded
    separately, at frame strides n + 1, n + 4099 and (full frames) the overlapped n / 2 with a Kaiser window, and once
    without a window; outs[i] of the first tight call against the oracle (last frame, last illuminator)"""
    strides = GAPS + (("overlap",) if n_valid is None else ())      # n_valid < n: frame_stride >= n
    _caf_multi_check(n, R, F, nref, method, n_valid, mode, [(st, True) for st in strides] + [(1, False)])


def _caf_multi_check(n, R, F, nref, method, n_valid, mode, runs, NF=NF):
    """``runs``: (frame stride mode, windowed) per guarded call; the first one is held to the oracle"""
    valid = n if n_valid is None else n_valid
    kaiser = np.kaiser(n, 5.0)
    plan = engine.CafPlan(n, R, F, NF * nref, method=method, multi=mode)
    for k, (st, win) in enumerate([(st, kaiser if w else None) for st, w in runs]):
        refs, srv = _caf_data(n, valid, R, st, 7000 + n + R, nref, NF)
        ins = {f"ref{i}": _caf_in(refs[i], n, valid, st) for i in range(nref)}
        ins["srv"] = _caf_in(srv, n, valid, st)
        if win is not None:
            ins["win"] = guard.In(_dev(win.astype(np.float32))[None])
        outs = {f"out{i}": guard.Out(1, NF * F * (R + 1), torch.complex64) for i in range(nref)}

        def run(a, s):
            plan.execute_multi([a[f"ref{i}"] for i in range(nref)], a["srv"], [a[f"out{i}"] for i in range(nref)], NF,
                               n // 2 if st == "overlap" else s["srv"], valid, a.get("win"))
            _sync()
        got = guard.check(run, ins, outs)
        if k == 0:
            i, b = nref - 1, NF - 1
            exp = O.fast_xambg(_caf_frame(refs[i], n, st, b), _caf_frame(srv, n, st, b), R, F, n, kaiser)[:, :, 0]
            assert rel_err(_host(got.tight[f"out{i}"]).reshape(NF, F, R + 1)[b], exp) < TIGHT
    plan.close()


# ---- LS -----------------------------------------------------------------------------------------------------------------
NB = 3
FIVE = (0, 1, -1, 2, -2)


def _ls_check(plan, n, T, bins, gap, ref, srv, fs=1.0e4, reg=0.0, out_gap=7):
    nb = ref.shape[0]                                                              # NB, or fewer blocks of a plan made for NB
    ins = {"ref": guard.In(_dev(ref), n + gap), "srv": guard.In(_dev(srv), n + gap)}
    outs = {"out": guard.Out(nb, n, torch.complex64, n + gap + out_gap),          # an out_stride different from stride
            "taps": guard.Out(1, nb * T, torch.complex128)}

    def run(a, s):
        plan.execute(a["ref"], a["srv"], a["out"], nb, s["ref"], s["out"], fs, bins, reg, a["taps"])
        _sync()
    got = guard.check(run, ins, outs)
    return _host(got.tight["out"]), _host(got.tight["taps"]).reshape(nb, T)


def _ls_scene(n, L, seed, nb=NB):
    ref, srv = scene.make_scene(n * nb, 1.0e4, min(L, 200), seed)
    return ref.reshape(nb, n), srv.reshape(nb, n)


LS_CASES = [(1, 4000, 16), (2, 40000, 64), (3, 40000, 64), (0, 40000, 64), (4, 40000, 128), (4, 40000, 2100)]


@pytest.mark.parametrize("method,n,L", LS_CASES, ids=[f"m{m}-{n}-{L}" for m, n, L in LS_CASES])
def test_ls(method, n, L):
    """prc_ls_execute, linear form: one bin and the five-bin chain (n >= 2000 * peek: the cached chain where the method
    has one), stride n + {1, 4099}, another out_stride, taps_out guarded"""
    T = L + 10
    ref, srv = _ls_scene(n, L, 4000 + n + L + method)
    plan = engine.LsPlan(n, L, 10, False, NB, method)
    b = NB - 1
    for bins in ((0,), FIVE):
        for k, gap in enumerate(GAPS):
            out, taps = _ls_check(plan, n, T, bins, gap, ref, srv)
            if k:
                continue
            if len(bins) == 1:
                exp, etaps = O.LS_Filter_Toeplitz(ref[b], srv[b], L, 10, True)
                assert rel_err(taps[b], etaps) < TIGHT and rel_err(out[b], exp) < TIGHT
            else:
                assert rel_err(out[b], O.LS_Filter_Multiple(ref[b], srv[b], L, 1.0e4, list(bins))) < TOL
    plan.close()


@pytest.mark.parametrize("n,L", [(4000, 16), (40000, 64)])
def test_ls_circular(n, L):
    """circular = 1 with reg (LS_Filter): the peek shift and the correlations wrap INSIDE the block -- with NaN in the
    gap a read of ref[n .. n + peek) shows at once"""
    T = L + 10
    ref, srv = _ls_scene(n, L, 5000 + n)
    plan = engine.LsPlan(n, L, 10, True, NB, 0)
    for k, gap in enumerate(GAPS):
        out, taps = _ls_check(plan, n, T, (0,), gap, ref, srv, 1.0, 1.0)
        if k == 0:
            exp, etaps = O.LS_Filter(ref[NB - 1], srv[NB - 1], L, 1.0, 10, True)
            assert rel_err(out[NB - 1], exp) < TIGHT and rel_err(taps[NB - 1], etaps) < TIGHT
    plan.close()


@pytest.mark.parametrize("method,piece,pieces", [(3, 1025, 30), (4, 4097, 6)], ids=["chain1024", "chain4096"])
@pytest.mark.parametrize("tail", [1, 10])
def test_ls_ragged_tail(method, piece, pieces, tail):
    """the block lengths of test_ls_chain_last_piece_shorter_than_peek / test_ls_team_chain_...: the last overlap-save
    piece holds `tail` <= peek samples, so the run of `peek` wrapped reference samples straddles the last two pieces --
    and the piece after the last one is the gap"""
    L = 48
    n = pieces * (piece - (L + 10)) + tail
    ref, srv = _ls_scene(n, L, 12345 + tail)
    plan = engine.LsPlan(n, L, 10, False, NB, method)
    for bins in ((2, 0, -1), (0,)):
        out, _ = _ls_check(plan, n, L + 10, bins, 1, ref, srv)
        _ls_check(plan, n, L + 10, bins, 4099, ref, srv)
        bar = 5e-6 if len(bins) > 1 else TIGHT          # the bars of those two tests (chain / single bin)
        assert rel_err(out[0], O.LS_Filter_Multiple(ref[0], srv[0], L, 1.0e4, list(bins))) < bar, bins
    plan.close()


# ---- NLMS / GAL ---------------------------------------------------------------------------------------------------------
NS = 5


@pytest.mark.parametrize("L", [24, 2100, 4100, 8300])
def test_nlms(L):
    """prc_nlms_execute with one, two and four wavefronts per stream and the global-workspace kernel: inputs poisoned,
    taps_in and taps_out guarded, the documented zeros outside [filter_len, n - peek) written"""
    _nlms_check(L)


def _nlms_check(L, gaps=GAPS, NS=NS):
    from oracle import c_oracle
    n, T = L + 500, L + 10
    rng = np.random.default_rng(L)
    a, b = scene.make_scene(NS * 7 + n, 1e4, 50, 31 + L)
    ref = np.stack([a[7 * s:7 * s + n] for s in range(NS)])
    srv = np.stack([b[7 * s:7 * s + n] for s in range(NS)])
    tin = _cplx(rng, NS, T) * np.float32(0.05 / np.sqrt(T))
    for gap in gaps:
        ins = {"ref": guard.In(_dev(ref), n + gap), "srv": guard.In(_dev(srv), n + gap), "tin": guard.In(_dev(tin))}
        outs = {"out": guard.Out(NS, n, torch.complex64, n + gap + 3), "tout": guard.Out(1, NS * T, torch.complex64)}

        def run(a_, s):
            engine.nlms_execute(a_["ref"], a_["srv"], a_["out"], n, L, 0.05, 10, a_["tin"], a_["tout"], NS, s["ref"], s["out"])
            _sync()
        got = guard.check(run, ins, outs)
    out, tout = _host(got.tight["out"]), _host(got.tight["tout"]).reshape(NS, T)
    assert not out[:, :L].any() and not out[:, n - 10:].any()
    exp, etaps = c_oracle.nlms(ref[NS - 1], srv[NS - 1], L, 0.05, 10, tin[NS - 1])
    assert rel_err(out[NS - 1], exp) < TOL and rel_err(tout[NS - 1], etaps) < TOL


@pytest.mark.parametrize("D,L", [(64, 8), (1034, 32), (2100, 16)])
def test_gal(D, L):
    """prc_gal_execute: inputs poisoned, out / k_out / h_out guarded, the workspace holding NaN before the call"""
    _gal_check(D, L)


def _gal_check(D, L, gaps=GAPS, NS=NS):
    from gal_oracle import gal_jpe
    n = 300
    sc = [scene.make_ar2_scene(n, 262144.0, 64, 9000 + D + s) for s in range(NS)]
    ref, srv = np.stack([r[:n] for r, _ in sc]), np.stack([v[:n] for _, v in sc])
    for gap in gaps:
        ins = {"ref": guard.In(_dev(ref), n + gap), "srv": guard.In(_dev(srv), n + gap)}
        outs = {"out": guard.Out(NS, n, torch.complex64, n + gap + 5), "k": guard.Out(1, NS * D, torch.complex64),
                "h": guard.Out(1, NS * D, torch.complex64)}

        def run(a, s):
            wsb = engine.gal_workspace_bytes(D, NS)
            ws = _nan_bytes(wsb) if wsb else None
            engine.gal_execute(a["ref"], a["srv"], a["out"], n, L, D, 2e-3, 2e-2, 10, a["k"], a["h"], NS, s["ref"], s["out"], ws)
            _sync()
        got = guard.check(run, ins, outs)
    s = NS - 1
    out, k, h = (_host(got.tight[x]).reshape(NS, -1)[s] for x in ("out", "k", "h"))
    eo, ek, eh = gal_jpe(ref[s], srv[s], L, D, 2e-3, 2e-2, 10, np.complex64, True)
    assert not out[n - 11:].any()
    assert rel_err(out, eo) <= 1e-4 and rel_err(k, ek) <= 2e-4 and rel_err(h, eh) <= 2e-4       # tests/test_gpu_gal.py's bars


# ---- front end ----------------------------------------------------------------------------------------------------------
FE_FS, FE_FOFF = 2_400_000, 100_000


def _raw(rng, dt, shape):
    if dt == "complex64":
        return _cplx(rng, *shape)
    if dt == "float32":
        return rng.standard_normal(shape[:-1] + (2 * shape[-1],)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape[:-1] + (2 * shape[-1],), endpoint=True).astype(dt)


def _fe_oracle(raw_block, dt, mix, up, dn, phase):
    x = raw_block if dt == "complex64" else O.deinterleave_IQ(raw_block)
    if mix:
        x = O.frequency_shift(x, FE_FOFF, FE_FS, np.array([phase]))
    return O.resample(x, up, dn)


@pytest.mark.parametrize("up,dn", [(13, 119), (3, 7), (5, 4), (17, 40)])
@pytest.mark.parametrize("dt", ["int8", "uint8", "int16", "float32", "complex64"])
def test_front_end(dt, up, dn):
    """prc_frontend_execute and _execute2: raw_stride = the block + {1, 4099} raw scalars (complex samples for c64),
    out_stride = n_out + {1, 4099}, a block shorter than one window and a long one, mix on and off, the group form
    (folded and unfolded tap rows) and the one-output-per-thread form.  Integer raw types run with the gaps at 0 and at
    the type's maximum.  Every option combination runs at both gaps."""
    rng = np.random.default_rng(up * 100 + dn)
    width = 1 if dt == "complex64" else 2                   # raw elements per complex sample
    for n_in in (2 * dn + 3, 64 * dn + 37):
        plan = engine.FrontendPlan(n_in, dt, up, dn, NB)
        n_out = plan.n_out
        ra, rb = _raw(rng, dt, (NB, n_in)), _raw(rng, dt, (NB, n_in))
        phases = O.block_phase_offsets(NB, 2 * n_in, FE_FS, FE_FOFF)
        for mix in (True, False):
            forms = [(0, 1), (1, 1)] + ([(0, 0)] if (dn % 2 and up <= 16) else [])
            for method, fold, gap in [(m, f, g) for m, f in forms for g in GAPS]:
                ins = {"a": guard.In(_dev(ra), width * n_in + gap), "b": guard.In(_dev(rb), width * n_in + gap)}
                one = {"out": guard.Out(NB, n_out, torch.complex64, n_out + gap)}
                two = {"oa": guard.Out(NB, n_out, torch.complex64, n_out + gap), "ob": guard.Out(NB, n_out, torch.complex64, n_out + gap)}

                def run1(a, s):
                    plan.execute(a["a"], a["out"], NB, s["a"], s["out"], FE_FOFF, FE_FS, phases, mix)
                    _sync()

                def run2(a, s):
                    plan.execute2(a["a"], a["b"], a["oa"], a["ob"], NB, s["a"], s["oa"], FE_FOFF, FE_FS, phases, mix)
                    _sync()
                with _option(_lib.OPT_FE_METHOD, method), _option(_lib.OPT_FE_FOLD, fold):
                    g1 = guard.check(run1, {"a": ins["a"]}, one)
                    g2 = guard.check(run2, ins, two)
                assert torch.equal(g2.tight["oa"], g1.tight["out"])          # prcore.h: bit-identical to two calls
                if gap == 1:
                    b = NB - 1
                    e = rel_err(_host(g2.tight["ob"])[b], _fe_oracle(rb[b], dt, mix, up, dn, phases[b]))
                    assert e < TIGHT, (n_in, mix, method, fold, e)
        plan.close()


# ---- CFAR ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,fw,gw", [(5, 7, 18, 4), (33, 64, 7, 2), (64, 257, 18, 4)])
def test_cfar(H, W, fw, gw):
    """prc_cfar2d and prc_cfar2d_c64, both kernel forms, ratio and threshold outputs: no strides, lead and tail only"""
    rng = np.random.default_rng(H * 1000 + W)
    Xc = _cplx(rng, NF, H, W)
    Xc[1, H // 2, W // 3] += 1e3
    Xa = np.abs(Xc).astype(np.float32)
    for fn, X, dtype in ((_lib.lib().prc_cfar2d, Xa, np.float32), (_lib.lib().prc_cfar2d_c64, Xc, np.complex64)):
        ins = {"x": guard.In(_dev(X.reshape(1, -1)))}
        outs = {"out": guard.Out(1, NF * H * W, torch.float32)}
        for method in (0, 1):
            thr = 0.0
            for use_thresh in (0, 1):
                def run(a, s):
                    _lib.check(fn(a["x"].data_ptr(), H, W, fw, gw, use_thresh, thr, a["out"].data_ptr(), NF, None))
                    _sync()
                with _option(_lib.OPT_CFAR_METHOD, method):
                    got = _host(guard.check(run, ins, outs).tight["out"]).reshape(NF, H, W)
                if use_thresh:
                    assert set(np.unique(got)) <= {0.0, 1.0} and (got != (ratio > np.float32(thr))).mean() < 1e-3
                else:
                    ratio, thr = got, float(np.median(got))
                    for k in range(NF):
                        assert rel_err(got[k], O.CFAR_2D(Xa[k], fw, gw)) < TIGHT, (method, k)


# ---- the rest: one small case each, lead and tail on every device argument ---------------------------------------------
def test_xcorr():
    from conftest import load_golden
    g = load_golden("xcorr")
    s1, s2 = g["s1"].astype(np.complex64), g["s2"].astype(np.complex64)
    n = s1.shape[0]
    for nlead, nlag, key in ((3, 9, "z_3_9"), (7, 0, "z_7_0"), (0, 20, "z_0_20")):
        ins = {"s1": guard.In(_dev(s1)[None]), "s2": guard.In(_dev(s2)[None])}

        def run(a, s):
            _lib.check(_lib.lib().prc_xcorr(a["s1"].data_ptr(), a["s2"].data_ptr(), n, nlead, nlag, a["z"].data_ptr(), None))
            _sync()
        got = guard.check(run, ins, {"z": guard.Out(1, nlead + nlag + 1, torch.complex64)})
        assert rel_err(_host(got.tight["z"])[0], g[key]) < TIGHT


def test_frequency_shift():
    """prc_frequency_shift, _block and _phases with both phase types"""
    n, fs, fc = 5003, 2.4e5, 37500.5
    x, _ = scene.make_scene(n, fs, 8, 77)
    rng = np.random.default_rng(3)
    ph64 = rng.uniform(-3, 3, n)
    lib = _lib.lib()
    cases = [
        ("shift", torch.complex64, None, lambda a: lib.prc_frequency_shift(a["x"].data_ptr(), a["y"].data_ptr(), n, fc, fs, 0.3, None),
         O.frequency_shift(x, fc, fs, 0.3)),
        ("block", torch.complex128, None, lambda a: lib.prc_frequency_shift_block(a["x"].data_ptr(), a["y"].data_ptr(), n, fc, fs, 0.3, None),
         O.frequency_shift(x, fc, fs, np.array([0.3]))),
        ("phases64", torch.complex128, ph64, lambda a: lib.prc_frequency_shift_phases(a["x"].data_ptr(), a["y"].data_ptr(), n, fc, fs, a["ph"].data_ptr(), 0, None),
         O.frequency_shift(x, fc, fs, ph64)),
        ("phases32", torch.complex64, ph64.astype(np.float32), lambda a: lib.prc_frequency_shift_phases(a["x"].data_ptr(), a["y"].data_ptr(), n, fc, fs, a["ph"].data_ptr(), 1, None),
         O.frequency_shift(x, fc, fs, ph64.astype(np.float32))),
    ]
    for name, ydt, ph, call, exp in cases:
        ins = {"x": guard.In(_dev(x)[None])}
        if ph is not None:
            ins["ph"] = guard.In(_dev(ph)[None])

        def run(a, s):
            _lib.check(call(a))
            _sync()
        got = guard.check(run, ins, {"y": guard.Out(1, n, ydt)})
        assert np.abs(_host(got.tight["y"])[0] - exp).max() < 2e-6, name          # test_xcorr_and_freqshift's bar


@pytest.mark.parametrize("dt", ["int8", "uint8", "int16", "float32"])
def test_deinterleave(dt):
    n = 1001
    raw = _raw(np.random.default_rng(8), dt, (1, n))

    def run(a, s):
        _lib.check(_lib.lib().prc_deinterleave(a["raw"].data_ptr(), _lib.RAW_DTYPES[dt], n, a["out"].data_ptr(), None))
        _sync()
    got = guard.check(run, {"raw": guard.In(_dev(raw))}, {"out": guard.Out(1, n, torch.complex64)})
    assert np.array_equal(_host(got.tight["out"])[0], O.deinterleave_IQ(raw[0]))


def test_decimate_and_channel_offset():
    """prc_decimate_iir; prc_channel_offset with xc_out guarded (test_channel_offset_edges' delayed pair)"""
    rng = np.random.default_rng(5)
    s = _cplx(rng, 5000)
    s2 = np.roll(s, 333)
    dec = engine.IirDecimator(3)
    m = dec.out_len(5000)

    def run(a, st):
        dec.decimate(a["x"], 5000, a["y"])
        _sync()
    got = guard.check(run, {"x": guard.In(_dev(s)[None])}, {"y": guard.Out(1, m, torch.complex64)})
    assert rel_err(_host(got.tight["y"])[0], O.decimate_iir(s, 3)) < 5e-6
    nl = 200
    n_xc = dec.n_lags(5000, 5000, nl)
    found = []

    def run_co(a, st):
        am, k = dec.channel_offset(a["s1"], 5000, a["s2"], 5000, nl, a["xc"])
        _sync()
        found.append((am, k))
    got = guard.check(run_co, {"s1": guard.In(_dev(s)[None]), "s2": guard.In(_dev(s2)[None])},
                      {"xc": guard.Out(1, n_xc, torch.float32)})
    off, xc = O.find_channel_offset(s, s2, 3, nl, return_xc=True)
    assert all(((am - nl) * 3, k) == (off, n_xc) for am, k in found) and off == -333
    assert rel_err(_host(got.tight["xc"])[0], xc) < 2e-5


@pytest.mark.parametrize("in_dt,out_dt,L,hold", [
    (torch.float32, torch.float64, 40, 20), (torch.float64, torch.float64, 40, 20), (torch.float32, torch.float32, 40, 20),
    (torch.float64, torch.float32, 40, 20),
    (torch.float64, torch.float64, 300, 300),          # more than PRC_PERSISTENCE_TERMS_PER_LAUNCH terms: chained launches
])
def test_persistence(in_dt, out_dt, L, hold):
    import simple_tracker_oracle as SO
    elems, decay = 33 * 21, 0.9 if hold == 20 else 0.99
    assert hold == 20 or hold > _lib.PERSISTENCE_TERMS_PER_LAUNCH
    x = torch.from_numpy(np.random.default_rng(9).exponential(1.0, (L, elems))).to(in_dt)
    code = {torch.float32: _lib.REAL_F32, torch.float64: _lib.REAL_F64}

    def run(a, s):
        _lib.check(_lib.lib().prc_persistence(a["x"].data_ptr(), code[in_dt], elems, L, 0, L, hold, decay, a["out"].data_ptr(),
                                              code[out_dt], None))
        _sync()
    got = guard.check(run, {"x": guard.In(x.reshape(1, -1).cuda())}, {"out": guard.Out(1, L * elems, out_dt)})
    out = _host(got.tight["out"]).reshape(L, elems)
    X = np.moveaxis(_host(x).reshape(L, elems, 1), 0, 2)
    for k in (0, 19, 20, L - 1):
        want = SO.persistence(X, k, hold, decay)[:, 0]
        assert np.array_equal(out[k], want.astype(out.dtype)), k          # bitwise, as test_persistence_* hold it


def _track_frames(nf, H, W, seed):
    rng = np.random.default_rng(seed)
    f = rng.exponential(1.0, (nf, H, W)).astype(np.float32)
    for i in range(nf):
        f[i, H // 2 + 8 + i, W // 2] += 40.0
    return f


def test_track():
    """prc_track_measure (frames, counts, cands guarded; the first min(count, capacity) candidates promised) and
    prc_track_run (counts, cands, records guarded); the tight calls bit-identical to the drop-in's chain"""
    from passiveradar_amd.target_detection import TrackPlan, _device_measure
    nf, H, W, ntracks, cap, ext = 3, 48, 40, 4, 16, [100.0, 50.0]
    frames = _track_frames(nf, H, W, 11)
    anchor = _device_measure(frames, ext, ntracks, capacity=cap)
    counts = np.asarray(anchor.counts)
    assert counts.min() >= 1 and counts.max() <= cap
    promised = torch.zeros(nf, cap, 4, dtype=torch.bool)
    for i in range(nf):
        promised[i, :counts[i]] = True
    plan = TrackPlan(H, W, ntracks, cap, ext)

    def measure(a, s):
        plan.measure(a["frames"].data_ptr(), nf, a["counts"].data_ptr(), a["cands"].data_ptr())
        _sync()
    got = guard.check(measure, {"frames": guard.In(_dev(frames.reshape(1, -1)))},
                      {"counts": guard.Out(1, nf, torch.int32),
                       "cands": guard.Out(1, nf * cap * 4, torch.float64, promised=promised.reshape(1, -1), finite=False)})
    assert np.array_equal(_host(got.tight["counts"])[0], counts)
    cands = _host(got.tight["cands"]).reshape(nf, cap, 4)
    want = anchor.candidates()
    for i in range(nf):
        assert cands[i, :counts[i]].tobytes() == want[i, :counts[i]].tobytes(), i
    # prc_track_run on the candidates just measured (the unwritten tail of each frame's list zeroed)
    clean = np.where(_host(promised), cands, 0.0)

    def track(a, s):
        plan.run(a["counts"].data_ptr(), a["cands"].data_ptr(), nf, a["rec"].data_ptr())
        _sync()
    got = guard.check(track, {"counts": guard.In(_dev(counts.astype(np.int32))[None]), "cands": guard.In(_dev(clean.reshape(1, -1)))},
                      {"rec": guard.Out(1, nf * ntracks * 32, torch.int64, finite=False)})
    assert _host(got.tight["rec"]).tobytes() == anchor.run().tobytes()
    plan.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strack(dtype):
    """prc_strack_run: frames and records guarded, the workspace pre-filled with NaN; bit-identical to the drop-in"""
    from passiveradar_amd.target_detection import _strack_desc, simple_target_tracker
    nf, H, W = 6, 64, 40
    frames = _track_frames(nf, H, W, 21).astype(dtype)
    code = _lib.REAL_F32 if dtype == np.float32 else _lib.REAL_F64
    d = _strack_desc(H, W, code, 100.0, 100.0)
    nb = C.c_size_t(0)
    _lib.check(_lib.lib().prc_strack_workspace_bytes(C.byref(d), nf, C.byref(nb)))

    def run(a, s):
        ws = _nan_bytes(nb.value)
        _lib.check(_lib.lib().prc_strack_run(C.byref(d), a["frames"].data_ptr(), nf, None, a["rec"].data_ptr(), ws.data_ptr(), None))
        _sync()
    got = guard.check(run, {"frames": guard.In(_dev(frames.reshape(1, -1)))},
                      {"rec": guard.Out(1, nf * 34, torch.int64, finite=False)})
    rec = np.frombuffer(_host(got.tight["rec"]).tobytes(), dtype=_lib.STRACK_RECORD_DTYPE)
    h = simple_target_tracker(np.moveaxis(frames, 0, 2), 100.0, 100.0)
    for k in ("lock_mode", "measurement", "measurement_idx", "estimate"):
        assert np.array_equal(rec[k], h[k]), k
    assert np.array_equal(rec["x"], h["kalman_state"]["x"]) and np.array_equal(rec["P"], h["kalman_state"]["P"].reshape(nf, 16))


# ---- left-over state: a plan at full capacity on A, then smaller on B, equals a fresh plan on B ---------------------------
def _fresh_vs_used(make_plan, big, small):
    """``big(plan)`` runs input A at full capacity; ``small(plan)`` returns B's result(s) as tensors: the used plan's
    must be bit-identical to a fresh plan's"""
    used, fresh = make_plan(), make_plan()
    big(used)
    a, b = small(used), small(fresh)
    _sync()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if not x.is_complex() else torch.view_as_real(x).view(torch.int32),
                           y.view(torch.int32) if not y.is_complex() else torch.view_as_real(y).view(torch.int32))
    for p in (used, fresh):
        p.close()


@pytest.mark.parametrize("method,n,R,F", [(1, 5000, 4, 51), (2, 8192, 70, 128), (2, 65536, 40, 256), (3, 20000, 700, 3),
                                          (3, 65536, 1024, 8)])
def test_leftover_caf(method, n, R, F):
    """CafPlan(max_frames=4): 4 frames of A, then 1 frame of B (also with n_valid < n on the second call only, through
    execute_segments + execute_doppler, and execute_multi with nref = 4 then 1)"""
    A_ref, A_srv = (_dev(x) for x in scene.make_scene(4 * n, 1e4, min(R, 200), 1))
    A2 = [_dev(scene.white_reference(n, 50 + i)) for i in range(3)]
    B_ref, B_srv = (_dev(x) for x in scene.make_scene(n, 1e4, min(R, 200), 2))
    win = _dev(np.kaiser(n, 5.0).astype(np.float32))
    shape = (F, R + 1)

    def make():
        return engine.CafPlan(n, R, F, 4, method=method)

    def big(p):
        p.execute(A_ref, A_srv, torch.empty((4,) + shape, dtype=torch.complex64, device="cuda"), 4, n, n, win)

    def big_multi(p):
        outs = [torch.empty(shape, dtype=torch.complex64, device="cuda") for _ in range(4)]
        p.execute_multi([A_ref[:n]] + A2, A_srv[:n], outs, 1, n, n, win)

    def small(n_valid, via):
        def go(p):
            out = torch.zeros(shape, dtype=torch.complex64, device="cuda")
            if via == "execute":
                p.execute(B_ref, B_srv, out, 1, n, n_valid, win)
            elif via == "segments":
                p.execute_segments(B_ref, B_srv, 1, n, n_valid, win)
                p.execute_doppler(out, 1)
            else:
                p.execute_multi([B_ref], B_srv, [out], 1, n, n_valid, win)
            return [out]
        return go
    _fresh_vs_used(make, big, small(n, "execute"))
    _fresh_vs_used(make, big, small(n - n // 7, "execute"))
    _fresh_vs_used(make, big, small(n, "segments"))
    _fresh_vs_used(make, big_multi, small(n, "multi"))


@pytest.mark.parametrize("method,n,L", [(1, 4000, 16), (2, 40000, 64), (3, 40000, 64), (4, 40000, 128), (4, 40000, 2100)])
def test_leftover_ls(method, n, L):
    """LsPlan(max_blocks=4): 4 blocks x 5 bins of A, then 1 block x 1 bin of B (cached chain, then uncached), then
    1 block x 5 bins of B"""
    T = L + 10
    A_ref, A_srv = (_dev(x) for x in scene.make_scene(4 * n, 1e4, min(L, 200), 3))
    B_ref, B_srv = (_dev(x) for x in scene.make_scene(n, 1e4, min(L, 200), 4))

    def make():
        return engine.LsPlan(n, L, 10, False, 4, method)

    def big(p):
        p.execute(A_ref, A_srv, torch.empty(4 * n, dtype=torch.complex64, device="cuda"), 4, n, n, 1e4, FIVE, 0.0,
                  torch.empty(4 * T, dtype=torch.complex128, device="cuda"))

    def small(p):
        res = []
        for bins in ((0,), FIVE):
            out = torch.zeros(n, dtype=torch.complex64, device="cuda")
            taps = torch.zeros(T, dtype=torch.complex128, device="cuda")
            p.execute(B_ref, B_srv, out, 1, n, n, 1e4, bins, 0.0, taps)
            res += [out, taps]
        return res
    _fresh_vs_used(make, big, small)


def test_leftover_front_end():
    """FrontendPlan(max_blocks=4): 4 blocks with mix on, then 1 block with mix off"""
    rng = np.random.default_rng(6)
    for dt, up, dn in (("int8", 13, 119), ("int16", 17, 40)):
        n_in = 64 * dn + 37
        A, B = _dev(_raw(rng, dt, (4, n_in))), _dev(_raw(rng, dt, (1, n_in)))

        def make():
            return engine.FrontendPlan(n_in, dt, up, dn, 4)

        def big(p):
            p.execute(A, torch.empty(4 * p.n_out, dtype=torch.complex64, device="cuda"), 4, fc=FE_FOFF, fs=FE_FS,
                      phases=[0.1, 0.2, 0.3, 0.4], mix=True)

        def small(p):
            out = torch.zeros(p.n_out, dtype=torch.complex64, device="cuda")
            p.execute(B, out, 1, fc=FE_FOFF, fs=FE_FS, mix=False)
            return [out]
        _fresh_vs_used(make, big, small)


def test_leftover_cfar_scratch():
    """prc_cfar2d's per-stream scratch: nframes = 8, then nframes = 1, on the same stream; then the same pair on a second
    torch.cuda.Stream.  Each one-frame result must be bit-identical to ``alone``, the same one-frame call made first on
    a stream of its own.  torch's stream pool may have handed that stream out before, so its scratch need not be
    fresh: ``alone`` is therefore held to the oracle, once for each kernel form."""
    H, W, fw, gw = 64, 257, 18, 4
    rng = np.random.default_rng(12)
    A = _dev(np.abs(_cplx(rng, 8, H, W)) * np.float32(100.0))
    B = _dev(np.abs(_cplx(rng, 1, H, W)))
    want = O.CFAR_2D(_host(B)[0], fw, gw)
    _sync()

    def cfar(x, nf, stream):
        out = torch.zeros_like(x)
        _sync()                                  # the fill ran on the current stream
        with torch.cuda.stream(stream):
            _lib.check(_lib.lib().prc_cfar2d(x.data_ptr(), H, W, fw, gw, 0, 0.0, out.data_ptr(), nf, C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        return out
    for method in (0, 1):
        with _option(_lib.OPT_CFAR_METHOD, method):
            alone = cfar(B, 1, torch.cuda.Stream())
            assert rel_err(_host(alone)[0], want) < TIGHT, method
            for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
                cfar(A, 8, stream)
                assert torch.equal(cfar(B, 1, stream).view(torch.int32), alone.view(torch.int32)), method


def test_leftover_track_plan_and_decimator():
    """a TrackPlan and an IirDecimator after a large call, then a small one: as a fresh one"""
    from passiveradar_amd.target_detection import TrackPlan
    H, W, ntracks, cap, ext = 48, 40, 4, 64, [100.0, 50.0]
    A, B = _dev(_track_frames(12, H, W, 31) * np.float32(3.0)), _dev(_track_frames(2, H, W, 32))

    def chain(plan, x, nf):
        counts = torch.zeros(nf, dtype=torch.int32, device="cuda")
        cands = torch.zeros(nf * cap * 4, dtype=torch.float64, device="cuda")
        rec = torch.zeros(nf * ntracks * 32, dtype=torch.int64, device="cuda")
        plan.measure(x.data_ptr(), nf, counts.data_ptr(), cands.data_ptr())
        plan.run(counts.data_ptr(), cands.data_ptr(), nf, rec.data_ptr())
        _sync()
        return counts, cands.view(torch.int64), rec
    used, fresh = TrackPlan(H, W, ntracks, cap, ext), TrackPlan(H, W, ntracks, cap, ext)
    chain(used, A, 12)
    for x, y in zip(chain(used, B, 2), chain(fresh, B, 2)):
        assert torch.equal(x, y)
    used.close()
    fresh.close()
    rng = np.random.default_rng(13)
    big, small = _dev(_cplx(rng, 60000) * np.float32(50.0)), _dev(_cplx(rng, 500))

    def decimate(dec, x):
        y = torch.zeros(dec.out_len(x.numel()), dtype=torch.complex64, device="cuda")
        dec.decimate(x, x.numel(), y)
        xc = torch.zeros(dec.n_lags(x.numel(), x.numel(), 20), dtype=torch.float32, device="cuda")
        am, _ = dec.channel_offset(x, x.numel(), x, x.numel(), 20, xc)
        _sync()
        return torch.view_as_real(y).view(torch.int32), xc.view(torch.int32), am
    used, fresh = engine.IirDecimator(3), engine.IirDecimator(3)
    decimate(used, big)
    a, b = decimate(used, small), decimate(fresh, small)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
