"""psd / csd / specgram / preview of passiveradar_amd/spectral.py and prc_welch on the MI355X against the float64 NumPy
restatement of the contract (tests/psd_oracle.py, itself held to matplotlib.mlab by tests/test_psd_host.py).

The two accuracy bars: max|P - P_ref| / max P_ref <= 2e-6 (the project's bar for small goldens) and, on EVERY bin,
|10 log10(P / P_ref)| <= 0.01 dB -- 16 times what a complex64 NumPy restatement of the same arithmetic (float32 window
and transform, float64 accumulation) shows on these inputs (6.3e-4 dB at worst, on the 100 dB deep floor of `tone60` at
nfft 8192).  The shapes are the smallest at which each thing can go wrong."""
import ctypes as C
import threading

import numpy as np
import pytest

import guard
import psd_oracle as P

pytestmark = pytest.mark.gpu

FS = 2.4e6
REL_BAR = 2e-6
DB_BAR = 0.01


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64)


def errors(got, ref):
    return float(np.abs(got - ref).max() / ref.max()), float(np.abs(10 * np.log10(got / ref)).max())


@pytest.mark.parametrize("nfft", [64, 256, 2048, 8192])
def test_psd_parity(gpu_ready, nfft):
    from passiveradar_amd.spectral import psd
    worst = {}
    for noverlap in P.overlaps(nfft):
        for name, x in P.cases(nfft, noverlap).items():
            for detrend in ("none", "mean"):
                got, f = psd(x, NFFT=nfft, Fs=FS, detrend=detrend, noverlap=noverlap)
                assert got.shape == (nfft,) and got.dtype == np.float64 and np.array_equal(f, P.freqs(nfft, FS))
                rel, db = errors(got, P.psd_ref(nfft, noverlap, name, detrend))
                print(f"psd parity nfft {nfft} noverlap {noverlap} {name} detrend {detrend}: rel {rel:.3g}, dB {db:.3g}")
                worst[name] = (max(worst.get(name, (0, 0))[0], rel), max(worst.get(name, (0, 0))[1], db))
                assert rel <= REL_BAR and db <= DB_BAR, (nfft, noverlap, name, detrend, rel, db)
    print(f"psd parity nfft {nfft} worst (rel, dB) per case: {worst}")


def periodic_hann(nfft):
    """np.hanning is the symmetric Hann, whose leakage from an on-bin tone is O(1/nfft) everywhere; the known answer
    (1/4, 1, 1/4 and nothing else) is the periodic Hann's"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft)


@pytest.mark.parametrize("nfft", [64, 256, 2048, 8192])
def test_known_answer_on_a_bin(gpu_ready, nfft):
    from passiveradar_amd.spectral import psd
    fc = 101.9e6
    for k0 in (0, 1, nfft // 2 - 1, nfft // 2, nfft - 1):
        p, f = psd(P.bin_tone(nfft, k0, 3 * nfft), NFFT=nfft, Fs=FS, window=periodic_hann(nfft), Fc=fc)
        c = (k0 + nfft // 2) % nfft
        assert int(np.argmax(p)) == c, (nfft, k0)
        for nb in ((c - 1) % nfft, (c + 1) % nfft):
            assert abs(p[nb] / p[c] - 0.25) <= 0.25 * 1e-5, (nfft, k0, nb, p[nb] / p[c])
        rest = np.delete(p, [(c - 1) % nfft, c, (c + 1) % nfft])
        assert rest.max() < 1e-9 * p[c], (nfft, k0, rest.max() / p[c])
        assert f[c] == pytest.approx(k0 * FS / nfft - (FS if k0 >= nfft // 2 else 0) + fc, rel=0, abs=1e-6), (nfft, k0)


def test_edge_cases_and_rows(gpu_ready):
    from passiveradar_amd.spectral import psd, specgram
    nfft = 256
    for n in (nfft, nfft - 5):
        x = P.dc(n, 21)
        for detrend in ("none", "mean"):
            got, _ = psd(x, NFFT=nfft, Fs=FS, detrend=detrend)
            rel, db = errors(got, P.psd(x, NFFT=nfft, Fs=FS, detrend=detrend))
            assert rel <= REL_BAR and db <= DB_BAR, (n, detrend, rel, db)
    x = P.white(7 * nfft + 100, 22)
    per_seg = np.abs(P.segments(x, nfft, 0, None, np.hanning(nfft))) ** 2 * P.scale(np.hanning(nfft), FS)
    per_seg = np.roll(per_seg, -nfft // 2, axis=1)                       # [7, nfft], centred
    for navg, rows in ((1, 7), (2, 3), (3, 2), (7, 1), (0, 1)):
        spec, f, t = specgram(x, NFFT=nfft, Fs=FS, noverlap=0, navg=navg)
        k = 7 if navg == 0 else navg
        assert spec.shape == (nfft, rows) and t.shape == (rows,)
        assert np.array_equal(t, P.times(x.shape[0], nfft, FS, 0, navg))
        for r in range(rows):
            rel, db = errors(spec[:, r], per_seg[r * k:(r + 1) * k].mean(axis=0))
            assert rel <= REL_BAR and db <= DB_BAR, (navg, r, rel, db)
    with pytest.raises(ValueError):
        specgram(x, NFFT=nfft, Fs=FS, noverlap=0, navg=8)
    # mlab's defaults (noverlap 128) and a device tensor in, device tensors out
    spec, f, t = specgram(dev(x), Fs=FS)
    assert spec.is_cuda and tuple(spec.shape) == (256, 13)
    rel, db = errors(spec.cpu().numpy(), P.specgram(x, NFFT=256, Fs=FS))
    assert rel <= REL_BAR and db <= DB_BAR and np.array_equal(t, P.times(x.shape[0], 256, FS, 128))


def test_csd(gpu_ready):
    from passiveradar_amd.spectral import csd, psd
    for nfft, noverlap in ((256, 37), (2048, 1024), (8192, 0)):
        x = P.cases(nfft, noverlap)["white"]
        y = (np.roll(x, 5) * (0.5 - 0.2j) + 0.1 * P.white(x.shape[0], 31)).astype(np.complex64)
        for detrend in ("none", "mean"):
            got, _ = csd(x, y, NFFT=nfft, Fs=FS, detrend=detrend, noverlap=noverlap)
            ref = P.csd(x, y, NFFT=nfft, Fs=FS, detrend=detrend, noverlap=noverlap)
            assert got.dtype == np.complex128 and got.shape == (nfft,)
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"csd nfft {nfft} noverlap {noverlap} detrend {detrend}: rel {err:.3g}")
            assert err <= REL_BAR, (nfft, noverlap, detrend, err)
        auto, _ = csd(x, x, NFFT=nfft, Fs=FS, noverlap=noverlap)
        p, _ = psd(x, NFFT=nfft, Fs=FS, noverlap=noverlap)
        assert np.array_equal(bits(auto.real), bits(p)) and not auto.imag.any()
        # device tensors: the same bits
        gd, _ = csd(dev(x), dev(y), NFFT=nfft, Fs=FS, detrend="mean", noverlap=noverlap)
        assert np.array_equal(bits(gd.cpu().numpy().view(np.float64)), bits(got.view(np.float64)))


def test_raw_input_step_and_batch(gpu_ready):
    from passiveradar_amd.signal_utils import deinterleave_IQ
    from passiveradar_amd.spectral import psd
    nfft, noverlap = 256, 37
    n = P.PARITY_N[nfft]
    raw, z = P.int8_raw(n, 14)
    kw = dict(NFFT=nfft, Fs=FS, detrend="mean", noverlap=noverlap)
    want, _ = psd(deinterleave_IQ(raw), **kw)
    assert np.array_equal(bits(psd(raw, raw=True, **kw)[0]), bits(want))
    assert np.array_equal(bits(psd(dev(raw), raw=True, **kw)[0]), bits(want))
    assert np.array_equal(bits(psd(dev(z), **kw)[0]), bits(want))
    for dt in (np.int16, np.float32):
        assert np.array_equal(bits(psd(raw.astype(dt), raw=True, **kw)[0]), bits(want)), dt
    u8 = (raw.astype(np.int16) + 128).astype(np.uint8)
    zu = (u8[0::2].astype(np.float32) + 1j * u8[1::2].astype(np.float32)).astype(np.complex64)
    assert np.array_equal(bits(psd(u8, raw=True, **kw)[0]), bits(psd(zu, **kw)[0]))
    # two channels interleaved sample by sample: step 2 at offsets 0 and 1
    a, b = z, P.white(n, 41)
    for other in (None, np.nan):
        both = np.empty(2 * n, np.complex64)
        both[0::2], both[1::2] = a, b
        pa, pb = psd(a, **kw)[0], psd(b, **kw)[0]
        first, second = both.copy(), both.copy()
        if other is not None:
            first[1::2], second[0::2] = other, other
        assert np.array_equal(bits(psd(first, step=2, **kw)[0]), bits(pa))
        assert np.array_equal(bits(psd(second[1:], step=2, **kw)[0]), bits(pb))
        assert np.array_equal(bits(psd(dev(second)[1:], step=2, **kw)[0]), bits(pb))
    raw2 = np.empty(4 * n, np.int8)                                      # the same for raw scalars: I,Q pairs alternate
    raw2.reshape(-1, 2, 2)[:, 0, :] = raw.reshape(-1, 2)
    raw2.reshape(-1, 2, 2)[:, 1, :] = 127
    assert np.array_equal(bits(psd(raw2, raw=True, step=2, **kw)[0]), bits(want))
    # a batch of three channels, longer than one workgroup's run, host and device (a strided view is read in place)
    x3 = np.stack([P.white(40 * nfft + 9, s) for s in (51, 52, 53)])
    singles = np.stack([psd(x3[c], NFFT=nfft, Fs=FS)[0] for c in range(3)])
    got = psd(x3, NFFT=nfft, Fs=FS)[0]
    assert got.shape == (3, nfft) and np.array_equal(bits(got), bits(singles))
    wide = dev(np.concatenate([x3, np.full((3, 77), np.nan, np.complex64)], axis=1))
    assert np.array_equal(bits(psd(wide[:, :x3.shape[1]], NFFT=nfft, Fs=FS)[0]), bits(singles))


def test_element_index_past_2_31(gpu_ready):
    """one 8192-point segment whose samples lie 2^18 complex elements apart in an int8 recording of 4.3 GB: the last one
    sits at scalar 2^32 - 2^19, so a 32-bit element or byte offset anywhere on the load path shows"""
    import torch
    from passiveradar_amd.spectral import psd
    nfft, step = 8192, 1 << 18
    raw, z = P.int8_raw(nfft, 81)
    big = torch.zeros(((nfft - 1) * step + 1) * 2, dtype=torch.int8, device="cuda")
    big.view(-1, 2)[::step] = dev(raw.reshape(-1, 2))
    want = psd(raw, NFFT=nfft, Fs=FS, raw=True)[0]
    got = psd(big, NFFT=nfft, Fs=FS, raw=True, step=step)[0]
    assert np.array_equal(bits(got), bits(want))


def test_determinism_also_from_four_threads(gpu_ready):
    import torch
    from passiveradar_amd.spectral import csd, psd
    nfft = 2048
    x = dev(P.white(40 * nfft + 5, 61))
    y = dev(P.white(40 * nfft + 5, 62))
    kw = dict(NFFT=nfft, Fs=FS, detrend="mean", noverlap=nfft // 2)
    p0, c0 = psd(x, **kw)[0], csd(x, y, **kw)[0]
    assert torch.equal(psd(x, **kw)[0], p0) and torch.equal(torch.view_as_real(csd(x, y, **kw)[0]), torch.view_as_real(c0))
    torch.cuda.synchronize()
    results, errors_ = [None] * 4, []

    def work(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                out = [(psd(x, **kw)[0], csd(x, y, **kw)[0]) for _ in range(3)]
            st.synchronize()
            results[i] = out
        except Exception as e:                                          # noqa: BLE001 -- reported by the main thread
            errors_.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors_, errors_
    for out in results:
        for p, c in out:
            assert torch.equal(p, p0) and torch.equal(torch.view_as_real(c), torch.view_as_real(c0))


@pytest.mark.parametrize("dtype", ["complex64", "int8"])
@pytest.mark.parametrize("cross", [False, True], ids=["psd", "csd"])
def test_guard_bands(gpu_ready, dtype, cross, nfft=256, gap=1001):
    """prc_welch on guarded x, y, out and workspace: two channels at stride > extent, nfft 256, noverlap 37 and a whole
    segment's worth of samples minus one after the last segment -- reading 'one more segment' lands in poison
    (``nfft``, ``gap``: tests/test_gpu_far_blocks.py runs 64-point segments with the channels 4 GiB apart)"""
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    noverlap, nch, nseg, navg = 37, 2, 6, 2
    hop = nfft - noverlap
    n = nfft + (nseg - 1) * hop + hop - 1
    rows = nseg // navg
    w = np.hanning(nfft)
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.step, d.scale = nfft, noverlap, navg, 1, 1, P.scale(w, FS)
    d.in_dtype = _lib.RAW_DTYPES[dtype]
    got_seg, got_rows, ws = C.c_int64(0), C.c_int64(0), C.c_size_t(0)
    _lib.check(lib.prc_welch_rows(C.byref(d), n, C.byref(got_seg), C.byref(got_rows)))
    assert (got_seg.value, got_rows.value) == (nseg, rows)
    _lib.check(lib.prc_welch_workspace_bytes(C.byref(d), n, nch, C.byref(ws)))
    assert ws.value % 8 == 0
    win = dev(w.astype(np.float32))
    st = _lib.torch_stream_ptr()
    if dtype == "int8":
        pairs = [P.int8_raw(n, s) for s in (71, 72, 73, 74)]
        xs, ys = np.stack([pairs[0][0], pairs[1][0]]), np.stack([pairs[2][0], pairs[3][0]])      # [2, 2 n] scalars
        zx, zy = [pairs[0][1], pairs[1][1]], [pairs[2][1], pairs[3][1]]
        per, stride = 2, 2 * n + 2 * gap
    else:
        zx, zy = [P.dc(n, 71), P.white(n, 72)], [P.white(n, 73), P.dc(n, 74)]
        xs, ys = np.stack(zx), np.stack(zy)
        per, stride = 1, n + gap

    def run(a, s):
        assert s["x"] % per == 0 and (not cross or s["y"] == s["x"])
        _lib.check(lib.prc_welch(C.byref(d), a["x"].data_ptr(), a["y"].data_ptr() if cross else None, n, s["x"] // per, nch,
                                 win.data_ptr(), a["out"].data_ptr(), a["workspace"].data_ptr(), st))
        torch.cuda.synchronize()

    inputs = {"x": guard.In(dev(xs), stride=stride)}
    if cross:
        inputs["y"] = guard.In(dev(ys), stride=stride)
    nws = ws.value // 8
    outputs = {"out": guard.Out(1, nch * rows * nfft, torch.complex128 if cross else torch.float64),
               "workspace": guard.Out(1, nws, torch.float64, promised=torch.zeros((1, nws), dtype=torch.bool), finite=False)}
    got = guard.check(run, inputs, outputs)
    out = got.tight["out"].cpu().numpy().reshape(nch, rows, nfft)
    for c in range(nch):
        ref = P.welch(zx[c], zy[c] if cross else None, NFFT=nfft, Fs=FS, detrend="mean", noverlap=noverlap, navg=navg)
        assert float(np.abs(out[c] - ref).max() / np.abs(ref).max()) <= REL_BAR, c


def test_bad_arguments_write_nothing(gpu_ready):
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    d = _lib.WelchDesc()
    d.nfft, d.noverlap, d.navg, d.detrend, d.in_dtype, d.step, d.scale = 256, 0, 0, 0, 4, 1, 1.0
    x = torch.ones(1024, dtype=torch.complex64, device="cuda")
    win = torch.ones(256, dtype=torch.float32, device="cuda")
    out = torch.full((256,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.full((4096,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    E = _lib.PRC_EINVAL
    assert lib.prc_welch(C.byref(d), None, None, 1024, 1024, 1, p(win), p(out), p(work), None) == E
    assert lib.prc_welch(C.byref(d), p(x), None, 0, 1024, 1, p(win), p(out), p(work), None) == E
    assert lib.prc_welch(C.byref(d), p(x), None, 1024, 1024, 0, p(win), p(out), p(work), None) == E
    assert lib.prc_welch(C.byref(d), p(x), None, 1024, 1024, 1, None, p(out), p(work), None) == E
    assert lib.prc_welch(C.byref(d), p(x), None, 1024, 1024, 1, p(win), p(out), None, None) == E
    d.navg = 5
    assert lib.prc_welch(C.byref(d), p(x), None, 1024, 1024, 1, p(win), p(out), p(work), None) == _lib.PRC_ESHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((work == 7.0).all())


@pytest.mark.parametrize("interleaved", [False, True])
def test_preview(gpu_ready, interleaved):
    from passiveradar_amd import scene
    from passiveradar_amd.signal_utils import deinterleave_IQ, find_channel_offset, frequency_shift, resample, xcorr
    from passiveradar_amd.spectral import preview
    icl, fs = 200000, 2.4e6
    cfg = dict(interleaved_input_channels=interleaved, input_chunk_length=icl, input_sample_rate=fs,
               input_center_freq=102.0e6, offset_freq=50000, resamp_up=13, resamp_dn=119, channel_bandwidth=fs * 13 / 119,
               channel_freq=101.95e6)
    raw_ref, raw_srv = scene.make_raw_stream(1, icl, fs, 50000, scene.scene_seed(7))
    raw_srv = np.roll(raw_srv.reshape(-1, 2), 24, axis=0).reshape(-1)                  # delayed by 24 samples
    if interleaved:
        data = np.empty(icl, np.int8)
        data.reshape(-1, 2, 2)[:, 0, :] = raw_ref.reshape(-1, 2)[:icl // 4]
        data.reshape(-1, 2, 2)[:, 1, :] = raw_srv.reshape(-1, 2)[:icl // 4]
        got = preview(cfg, data)
        iq = deinterleave_IQ(data)
        ref, srv = iq[0::2], iq[1::2]
    else:
        got = preview(cfg, raw_ref, raw_srv)
        ref, srv = deinterleave_IQ(raw_ref), deinterleave_IQ(raw_srv)
    assert got["offset"] == find_channel_offset(ref, srv, 4, 50000)
    assert np.array_equal(got["xcorr_lags"], np.arange(-2000, 2001))
    assert np.array_equal(got["xcorr_abs"], np.abs(xcorr(ref, srv, 2000, 2000)))
    assert got["input_psd"].shape == (2, 8192) and got["channel_psd"].shape == (2, 2048)
    assert np.array_equal(got["input_freqs"], P.freqs(8192, fs, 102.0e6))
    assert np.array_equal(got["channel_freqs"], P.freqs(2048, cfg["channel_bandwidth"], 101.95e6))
    for c, z in enumerate((ref, srv)):
        want = 10 * np.log10(P.psd(z, NFFT=8192, Fs=fs))
        assert np.abs(got["input_psd"][c] - want).max() <= DB_BAR, c
        zz = resample(frequency_shift(z, 50000, fs), 13, 119)
        want = 10 * np.log10(P.psd(zz, NFFT=2048, Fs=cfg["channel_bandwidth"]))
        assert np.abs(got["channel_psd"][c] - want).max() <= DB_BAR, c
