"""LS_Filter_SVD on the GPU (passiveradar_amd/csrc/ls_svd.hip): the reference's goldens, the shapes at which the kernels take
another path, rank-revealing behaviour, batches and determinism, guard bands and the HipBackend mode, against the float64
restatement (tests/ls_svd_oracle.py).  Errors are peak-normalised (conftest.rel_err).  Bars: out 1e-4 (the project's parity
bar; the reference's own float32 distance to the restatement on the goldens is <= 3.0e-5, tools/gen_golden_ls_svd.py);
complex64 taps 2^-23 of the peak tap (one float32 rounding); device complex128 taps TAPS128_BAR (below)."""
import functools

import numpy as np
import pytest

from conftest import load_golden, rel_err
from ls_svd_oracle import data_matrix, ls_filter_svd

pytestmark = pytest.mark.gpu

GOLDENS = ("ls_svd_white", "ls_svd_white_peek0", "ls_svd_white_t74", "ls_svd_ar2", "ls_svd_periodic", "ls_svd_periodic_noise")

# device complex128 taps against the restatement on the goldens (cond of the kept directions <= 393), measured on MI355X:
# white 2.3e-15, white_peek0 1.1e-15, white_t74 1.3e-15, ar2 3.3e-13, periodic 1.8e-14, periodic_noise 2.24e-11.  The bar is
# 10x the largest; anything looser than 1e-8 would not be allowed.
TAPS128_BAR = 2.24e-10


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    yield


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(golden, restatement out, restatement taps, restatement info), computed once and shared"""
    g = load_golden(name)
    info = {}
    out, taps = ls_filter_svd(g["ref"], g["srv"], int(g["filterLen"]), int(g["peek"]), None, info)
    for a in (out, taps):
        a.setflags(write=False)
    return g, out, taps, info


def _run(ref, srv, L, peek, rcond=None):
    """one block through engine.ls_svd_execute: (out c64, taps c128, singular values, (kept, sweeps, converged))"""
    import torch
    from passiveradar_amd import engine
    n, T = ref.shape[0], L + peek
    r = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.complex64)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(srv, dtype=np.complex64)).cuda()
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    taps = torch.empty(T, dtype=torch.complex128, device="cuda")
    sv = torch.empty(T, dtype=torch.float64, device="cuda")
    info = torch.empty(3, dtype=torch.int32, device="cuda")
    ws = torch.empty(engine.ls_svd_workspace_bytes(n, L, peek, 1), dtype=torch.uint8, device="cuda")
    engine.ls_svd_execute(r, s, out, n, L, peek, rcond, 1, n, n, taps, sv, info, ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), taps.cpu().numpy(), sv.cpu().numpy(), tuple(int(v) for v in info.cpu().numpy())


def _cwhite(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def _surveillance(rng, ref, L, peek):
    """a decaying filter of T taps on the circular shifts of ref (by FFT), plus white noise at 0.05"""
    n, T = ref.shape[0], L + peek
    h0 = np.zeros(n, np.complex128)
    h0[:T] = _cwhite(rng, T) * np.exp(-np.arange(T) / 6.0)
    r = np.roll(ref.astype(np.complex128), -peek)
    clutter = np.fft.ifft(np.fft.fft(r) * np.fft.fft(h0))
    return (clutter + 0.05 * _cwhite(rng, n)).astype(np.complex64)


def _band_limited(rng, n, keep):
    """white noise with all but the lowest ``keep`` bins either side of zero frequency removed, unit power, complex64"""
    X = np.fft.fft(_cwhite(rng, n))
    X[keep:-keep] = 0
    x = np.fft.ifft(X)
    return (x / np.abs(x).std()).astype(np.complex64)


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(name):
    from passiveradar_amd.clutter_removal import LS_Filter_SVD
    g, eo, et, _ = _golden(name)
    L, peek = int(g["filterLen"]), int(g["peek"])
    out, taps = LS_Filter_SVD(g["ref"], g["srv"], L, peek, return_filter=True)
    assert out.dtype == taps.dtype == np.complex64 and out.shape == g["out"].shape and taps.shape == (L + peek,)
    e_out = rel_err(out, g["out"])
    e_taps = float(np.abs(taps - et).max() / np.abs(et).max())
    print(f"{name}: out {e_out:.2e} of the reference's peak, complex64 taps {e_taps:.2e} of the restatement's peak tap")
    assert e_out <= 1e-4, e_out
    assert e_taps <= 2.0 ** -23, e_taps
    assert LS_Filter_SVD(g["ref"], g["srv"], L, peek).dtype == np.complex64


def test_golden_zero_reference():
    from passiveradar_amd.clutter_removal import LS_Filter_SVD
    g = load_golden("ls_svd_zero_ref")
    out, taps, sv = LS_Filter_SVD(g["ref"], g["srv"], 16, 10, return_filter=True, return_singular_values=True)
    assert np.array_equal(out.view(np.uint32), g["srv"].view(np.uint32)) and np.array_equal(out, g["out"])
    assert not taps.any() and not sv.any() and np.isfinite(out).all()
    _, taps128, _, (kept, _, conv) = _run(g["ref"], g["srv"], 16, 10)
    assert kept == 0 and conv == 1 and not taps128.any()


@pytest.mark.parametrize("name", GOLDENS)
def test_device_complex128_taps(name):
    g, _, et, einfo = _golden(name)
    _, taps, sv, (kept, sweeps, conv) = _run(g["ref"], g["srv"], int(g["filterLen"]), int(g["peek"]))
    e = float(np.abs(taps - et).max() / np.abs(et).max())
    print(f"{name}: complex128 taps {e:.2e} of the peak tap, kept {kept}, sweeps {sweeps}")
    assert conv == 1 and kept == einfo["kept"]
    assert e <= TAPS128_BAR, e
    assert np.all(np.diff(sv) <= 0) and abs(sv[0] - einfo["sv"][0]) <= 1e-12 * einfo["sv"][0]


# (n, filterLen, peek): no pairs | one pair | odd, so a bye | more than one lag group | columns longer than a workgroup |
# config 3's length | n shorter than a tile, wrap-around on every lag
SHAPES = [(257, 1, 0), (257, 2, 0), (1021, 17, 10), (2048, 64, 10), (8192, 290, 10), (4099, 1034, 10), (63, 16, 10)]


@pytest.mark.parametrize("n,L,peek", SHAPES)
def test_shapes_against_restatement(n, L, peek):
    rng = np.random.default_rng(7000 + n + L)
    ref = _cwhite(rng, n)
    srv = _surveillance(rng, ref, L, peek)
    info = {}
    eo, et = ls_filter_svd(ref, srv, L, peek, None, info)
    out, taps, sv, (kept, sweeps, conv) = _run(ref, srv, L, peek)
    e_out, e_taps = rel_err(out, eo), rel_err(taps, et)
    print(f"n {n} T {L + peek}: out {e_out:.2e} taps {e_taps:.2e} kept {kept} sweeps {sweeps}")
    assert conv == 1 and kept == info["kept"] == L + peek
    assert e_out <= 1e-4, e_out
    assert np.abs(sv - info["sv"]).max() <= 1e-6 * info["sv"][0]


def test_periodic_reference_keeps_its_rank():
    """rank 8 of 26: eight directions kept at rcond = 1e-5 and the taps are the minimum-norm solution (the restatement's,
    and NumPy's lstsq at the same rcond)"""
    g = load_golden("ls_svd_periodic")
    info = {}
    eo, et = ls_filter_svd(g["ref"], g["srv"], 16, 10, 1e-5, info)
    out, taps, sv, (kept, _, conv) = _run(g["ref"], g["srv"], 16, 10, 1e-5)
    assert conv == 1 and kept == info["kept"] == 8
    lstsq = np.linalg.lstsq(data_matrix(g["ref"], 16, 10), g["srv"].astype(np.complex128), rcond=1e-5)[0]
    assert rel_err(taps, et) <= 1e-8 and rel_err(taps, lstsq) <= 1e-8, (rel_err(taps, et), rel_err(taps, lstsq))
    assert rel_err(out, eo) <= 1e-4
    assert np.abs(sv[:8] - info["sv"][:8]).max() <= 1e-6 * info["sv"][0]


def test_half_band_reference_cut_between_two_singular_values():
    """band-limited to 1/2 of the band, (4096, 64, 10): rcond at the geometric mean of two adjacent singular values of the
    restatement a factor >= 3 apart -- the same directions kept, the same output, the same singular values above the cut"""
    rng = np.random.default_rng(7100)
    ref = _band_limited(rng, 4096, 1024)
    srv = _surveillance(rng, ref, 64, 10)
    info = {}
    ls_filter_svd(ref, srv, 64, 10, 0.0, info)
    s = info["sv"] / info["sv"][0]
    steps = [i for i in range(len(s) - 1) if 1e-6 < s[i + 1] and s[i] < 1e-3 and s[i] >= 3 * s[i + 1]]
    assert steps, "the restatement's spectrum has no step of 3x between 1e-3 and 1e-6"      # the precondition
    i = steps[len(steps) // 2]
    rcond = float(np.sqrt(s[i] * s[i + 1]))
    eo, _ = ls_filter_svd(ref, srv, 64, 10, rcond, info)
    assert info["kept"] == i + 1
    out, _, sv, (kept, sweeps, conv) = _run(ref, srv, 64, 10, rcond)
    e_sv = float(np.abs(sv[:kept] - info["sv"][:kept]).max() / info["sv"][0])
    print(f"rcond {rcond:.2e} between sigma[{i}] and sigma[{i + 1}]: kept {kept}, out {rel_err(out, eo):.2e}, sigma {e_sv:.2e}, sweeps {sweeps}")
    assert conv == 1 and kept == info["kept"]
    assert rel_err(out, eo) <= 1e-4
    assert e_sv <= 1e-6


def test_eighth_band_reference_default_cut():
    """the case on which the reference returns noise 26 times the right answer: finite, no larger than its input, and the
    restatement's output at the same default cut"""
    rng = np.random.default_rng(7200)
    ref = _band_limited(rng, 4096, 256)
    srv = _surveillance(rng, ref, 16, 10)
    eo, _ = ls_filter_svd(ref, srv, 16, 10)
    out, taps, _, (kept, sweeps, conv) = _run(ref, srv, 16, 10)
    print(f"1/8 band, default cut: out {rel_err(out, eo):.2e}, kept {kept}, sweeps {sweeps}, peak tap {np.abs(taps).max():.3g}")
    assert conv == 1 and np.isfinite(out).all() and np.isfinite(taps).all()
    assert np.linalg.norm(out.astype(np.complex128)) <= np.linalg.norm(srv.astype(np.complex128))
    assert rel_err(out, eo) <= 1e-4


def _batch_call(refs, srvs, n, L, peek, stride, ostride):
    import torch
    from passiveradar_amd import engine
    nb, T = refs.shape[0], L + peek
    r, s = torch.from_numpy(refs).cuda(), torch.from_numpy(srvs).cuda()
    sentinel = complex(7.0, -3.0)
    out = torch.full((nb, ostride), sentinel, dtype=torch.complex64, device="cuda")
    taps = torch.empty((nb, T), dtype=torch.complex128, device="cuda")
    sv = torch.empty((nb, T), dtype=torch.float64, device="cuda")
    info = torch.empty((nb, 3), dtype=torch.int32, device="cuda")
    ws = torch.empty(engine.ls_svd_workspace_bytes(n, L, peek, nb), dtype=torch.uint8, device="cuda")
    engine.ls_svd_execute(r, s, out, n, L, peek, None, nb, stride, ostride, taps, sv, info, ws)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == sentinel)
    return out[:, :n], taps.cpu().numpy(), sv.cpu().numpy(), info.cpu().numpy()


def test_batch_equals_single_calls_and_repeats():
    """a silent, a periodic and a white block in one call (stride > n, a separate out_stride) == three single calls, bit for
    bit; the same call twice gives the same bits"""
    n, L, peek, stride, ostride = 4096, 16, 10, 4096 + 37, 4096 + 5
    rng = np.random.default_rng(7300)
    refs = np.zeros((3, stride), np.complex64)
    srvs = np.zeros((3, stride), np.complex64)
    refs[1, :n] = np.tile(_cwhite(rng, 8), n // 8)
    refs[2, :n] = _cwhite(rng, n)
    for b in range(3):
        srvs[b, :n] = _surveillance(rng, refs[b, :n], L, peek)
    first = _batch_call(refs, srvs, n, L, peek, stride, ostride)
    again = _batch_call(refs, srvs, n, L, peek, stride, ostride)
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert tuple(first[3][:, 0]) == (0, 8, 26) and first[3][:, 2].all()
    for b in range(3):
        out, taps, sv, info = _run(refs[b, :n], srvs[b, :n], L, peek)
        assert np.array_equal(first[0][b].view(np.uint8), out.view(np.uint8)), b
        assert np.array_equal(first[1][b].view(np.uint8), taps.view(np.uint8)), b
        assert np.array_equal(first[2][b].view(np.uint8), sv.view(np.uint8)), b
        assert tuple(first[3][b]) == info, b


@pytest.mark.parametrize("gap", [1, 4099])
def test_guard_bands(gap):
    """prc_ls_svd_execute: inputs poisoned outside their blocks; out, taps_out, sv_out, info_out and the workspace at its
    queried size guarded; two blocks"""
    import torch
    import guard
    from passiveradar_amd import engine
    NS, n, L, peek = 2, 1021, 27, 10
    T = L + peek
    rng = np.random.default_rng(7400)
    ref = np.stack([_cwhite(rng, n) for _ in range(NS)])
    srv = np.stack([_surveillance(rng, ref[b], L, peek) for b in range(NS)])
    wsb = engine.ls_svd_workspace_bytes(n, L, peek, NS)
    assert wsb % 16 == 0
    dev = lambda a: torch.from_numpy(a).cuda()
    ins = {"ref": guard.In(dev(ref), n + gap), "srv": guard.In(dev(srv), n + gap)}
    outs = {"out": guard.Out(NS, n, torch.complex64, n + gap + 5),
            "taps": guard.Out(1, NS * T, torch.complex128), "sv": guard.Out(1, NS * T, torch.float64),
            "info": guard.Out(1, NS * 3, torch.int32),
            # the workspace: 16-byte elements keep it aligned behind the guard's odd lead; nothing in it is promised
            "ws": guard.Out(1, wsb // 16, torch.complex128, promised=torch.zeros((1, wsb // 16), dtype=torch.bool), finite=False)}

    def run(a, s):
        engine.ls_svd_execute(a["ref"], a["srv"], a["out"], n, L, peek, None, NS, s["ref"], s["out"], a["taps"], a["sv"],
                              a["info"], a["ws"])
        torch.cuda.synchronize()
    got = guard.check(run, ins, outs)
    b = NS - 1
    eo, et = ls_filter_svd(ref[b], srv[b], L, peek)
    out = got.tight["out"].cpu().numpy()[b]
    taps = got.tight["taps"].cpu().numpy().reshape(NS, T)[b]
    assert rel_err(out, eo) <= 1e-4 and rel_err(taps, et) <= 1e-8
    assert tuple(got.tight["info"].cpu().numpy().reshape(NS, 3)[b, [0, 2]]) == (T, 1)


def test_entry_point_refuses_bad_sizes():
    from passiveradar_amd import engine
    for n, L, peek in ((26, 16, 10), (10, 16, 10), (8192, 4090, 10), (100, 0, 0)):
        with pytest.raises(ValueError):
            engine.ls_svd_workspace_bytes(n, L, peek, 1)
    assert engine.ls_svd_workspace_bytes(27, 16, 10, 1) > 0


def test_backend_equals_drop_in_and_oracle():
    """HipBackend(clutter='ls_svd'): chunk c of clean() == LS_Filter_SVD on that chunk, bit for bit; the maps through
    StreamProcessor == the oracle's fast_xambg of the restatement's cleaned chunks"""
    import torch
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    from passiveradar_amd.clutter_removal import LS_Filter_SVD
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    C, R, F, fs, nch = 16384, 24, 64, 1.0e5, 5
    ref, srv = scene.make_stream(nch, C, fs, R, 777)
    be = HipBackend(2 * C, R, F, fs, clutter="ls_svd", batch=4)
    got = StreamProcessor(be).process(ref, srv).cpu().numpy()
    ref_pad, srv_pad = be.padded(ref), be.padded(srv)
    cl = be.clean(ref_pad, srv_pad, nch)
    torch.cuda.synchronize()
    cl = cl.cpu().numpy()
    clean = np.concatenate([LS_Filter_SVD(ref[i * C:(i + 1) * C], srv[i * C:(i + 1) * C], R) for i in range(nch)])
    assert np.array_equal(cl[C // 2:C // 2 + nch * C], clean)
    exp_clean = np.concatenate([ls_filter_svd(ref[i * C:(i + 1) * C], srv[i * C:(i + 1) * C], R)[0] for i in range(nch)])
    assert rel_err(clean, exp_clean) < 1e-4
    pad = np.zeros(C // 2, np.complex64)
    rp, cp = np.concatenate((pad, ref, pad)), np.concatenate((pad, exp_clean.astype(np.complex64), pad))
    w = np.kaiser(2 * C, 5.0)
    for f in (0, 2, nch - 1):
        exp = O.fast_xambg(rp[f * C:f * C + 2 * C], cp[f * C:f * C + 2 * C], R, F, 2 * C, w)[:, :, 0]
        assert rel_err(got[f], exp) < 1e-4, f
