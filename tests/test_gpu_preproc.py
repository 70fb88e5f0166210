"""decimate, channel_preprocessing, shift, offset_compensation and normalize of passiveradar_amd/signal_utils.py and the
entry points under them (prc_fir_decimate, prc_shift, prc_normalize) on the MI355X, against goldens written by the
reference itself (tools/gen_golden_preproc.py; the inputs are regenerated from their seeds, tests/preproc_oracle.py).

Accuracy bar of the FIR decimator: 4e-6 of the peak.  A NumPy float32 emulation of the two kernels' own summation orders
(preproc_oracle.emulate_tile / emulate_direct, run on the CPU before any GPU run) differs from the same goldens by at most
8.2e-7 (tile form: n = 599, q = 59), 8.9e-7 (direct form: n = 3000, q = 97), 4.8e-7 on the channel_preprocessing cases and
5.4e-7 on the tail of the 2^24 + 70 000 sample recording; 4 x 8.9e-7 = 3.6e-6 (fused multiply-adds, the device's sincosf),
rounded up to one digit.  normalize is held to 2e-6; shift and offset_compensation are exact.
Measured on the MI355X: decimate at most 9.1e-7 (tile form, n = 599, q = 59; direct form 8.9e-7 at q = 97), the dtype cases
3.0e-7, channel_preprocessing 4.8e-7, the long recording's tail 5.4e-7, normalize 1.1e-7; fused against composed: no
difference in any bit.  The shapes are the smallest at which each thing can go wrong."""
import ctypes as C

import numpy as np
import pytest

import guard
import preproc_oracle as O
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

BAR = 4e-6
NORM_BAR = 2e-6


@pytest.fixture(scope="module")
def gold():
    return {k: load_golden("preproc_" + k) for k in ("decimate", "channel", "misc")}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n,q", O.DECIMATE_CASES)
def test_decimate_goldens(gpu_ready, gold, n, q):
    from passiveradar_amd.signal_utils import decimate
    x = O.decimate_input(n, q)
    want = gold["decimate"][f"y_{n}_{q}"]
    got = decimate(x, q)
    assert got.shape == want.shape and got.dtype == np.complex64
    err = rel_err(got, want)
    print(f"decimate n {n} q {q} ({'tile' if q <= O.TILE_MAX_Q else 'direct'}): {err:.3g}")
    assert err <= BAR, (n, q, err)
    gd = decimate(dev(x), q)
    assert gd.is_cuda and same_bits(gd, got)


def test_decimate_columns_and_dtypes(gpu_ready, gold):
    from passiveradar_amd.signal_utils import decimate
    x = O.decimate_input(300, 5, 3)
    got = decimate(x, 5)
    assert got.shape == (60, 3) and rel_err(got, gold["decimate"]["cols"]) <= BAR
    for c in range(3):
        assert same_bits(got[:, c], decimate(x[:, c], 5)), c
    gd = decimate(dev(x), 5)
    assert tuple(gd.shape) == (60, 3) and same_bits(gd, got)
    nan_between = np.full((300, 5), np.nan, np.complex64)             # a strided device view is made contiguous, not over-read
    nan_between[:, ::2] = x
    assert same_bits(decimate(dev(nan_between)[:, ::2], 5), got)
    for name in O.DECIMATE_DTYPES:
        want = gold["decimate"]["dt_" + name]
        y = decimate(O.dtype_input(name), 5)
        assert y.dtype == want.dtype and y.shape == want.shape, name
        err = rel_err(y, want)
        print(f"decimate dtype {name}: {err:.3g}")
        assert err <= BAR, (name, err)


@pytest.mark.parametrize("name", list(O.CHANNEL_CASES))
def test_channel_preprocessing_goldens(gpu_ready, gold, name):
    from passiveradar_amd.signal_utils import channel_preprocessing
    dtype, nscalars, dec, fc, Fs = O.CHANNEL_CASES[name]
    raw = O.channel_input(name)
    want = gold["channel"]["y_" + name]
    got = channel_preprocessing(raw, dec, fc, Fs)
    assert got.shape == want.shape and got.dtype == np.complex64
    err = rel_err(got, want)
    print(f"channel_preprocessing {name}: {err:.3g}")
    assert err <= BAR, (name, err)
    gd = channel_preprocessing(dev(raw), dec, fc, Fs)
    assert gd.is_cuda and same_bits(gd, got)


def test_long_recording_where_the_sample_index_rounds(gpu_ready, gold):
    from passiveradar_amd.signal_utils import channel_preprocessing
    g = gold["channel"]
    raw = O.long_input()
    assert np.array_equal(O.checksum(raw), g["long_raw"])
    got = channel_preprocessing(dev(raw), 10, 1e5, 2.4e6)
    assert tuple(got.shape) == (O.out_len(O.LONG_SAMPLES, 10),)
    tail = got[-O.LONG_KEEP:].cpu().numpy()
    err = float(np.abs(tail - g["long_tail"]).max() / g["long_peak"])
    print(f"channel_preprocessing, last {O.LONG_KEEP} outputs of {O.LONG_SAMPLES} samples: {err:.3g}")
    assert err <= BAR, err


@pytest.mark.parametrize("name,dec", [("i8_2001", 10), ("i16_odd", 7), ("f32_odd", 60), ("u8", 97)])
def test_fused_equals_composed(gpu_ready, name, dec):
    """the one launch against decimate(frequency_shift(deinterleave_IQ(raw), fc, Fs), dec) through the existing entry
    points: the same conversion, the same rotation (phase_rot, one complex product) and the same sums, so the same bits --
    in the tile form and in the direct form"""
    from passiveradar_amd.signal_utils import channel_preprocessing, decimate, deinterleave_IQ, frequency_shift
    _, _, _, fc, Fs = O.CHANNEL_CASES[name]
    raw = O.channel_input(name)
    fused = channel_preprocessing(raw, dec, fc, Fs)
    composed = decimate(frequency_shift(deinterleave_IQ(raw), fc, Fs), dec)
    diff = float(np.abs(fused - composed).max() / np.abs(composed).max())
    print(f"fused against composed {name} dec {dec}: {diff:.3g}")
    assert same_bits(fused, composed), (name, dec, diff)


def _response(h, f):
    """|H| of the float32 taps at f cycles per input sample, in float64"""
    k = np.arange(h.shape[0])
    return np.abs(np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), k)), axis=1))


def test_known_answer_tones(gpu_ready):
    from passiveradar_amd.signal_utils import decimate
    q, n = 10, 6000
    h = O.taps32(q)
    i = np.arange(n)
    interior = slice(20, n // q - 20)                                 # the filter is 10 outputs long on either side
    # inside the pass band (the cut-off is 0.05 cycles per sample, the Hamming transition starts near 0.042)
    ripple = float(np.abs(_response(h, np.linspace(0.0, 0.03, 301)) - 1.0).max())
    y = decimate(np.exp(2j * np.pi * 0.02 * i).astype(np.complex64), q)
    amp = np.abs(y[interior])
    print(f"pass-band tone: amplitude {amp.min():.7f} .. {amp.max():.7f}, design ripple {ripple:.3g}")
    assert ripple < 5e-3 and np.abs(amp - 1.0).max() <= ripple + BAR
    # at 0.9 of Nyquist: attenuated by what the taps' own response says, less 1 dB
    gain = float(_response(h, 0.45)[0])
    y = decimate(np.exp(2j * np.pi * 0.45 * i).astype(np.complex64), q)
    amp = float(np.abs(y[interior]).max())
    print(f"stop-band tone: amplitude {amp:.3g}, |H| {gain:.3g} ({20 * np.log10(gain):.1f} dB)")
    assert gain < 1e-2 and amp <= gain * 10 ** (1 / 20)


def test_shift(gpu_ready, gold):
    from passiveradar_amd.signal_utils import shift
    for name, x in O.shift_inputs().items():
        for k in O.SHIFTS:
            want = gold["misc"][f"shift_{name}_{k}"]
            got = shift(x, k)
            assert got.dtype == x.dtype and got.shape == x.shape and np.array_equal(got, want), (name, k)
            gd = shift(dev(x), k)
            assert gd.is_cuda and gd.dtype == dev(x).dtype and np.array_equal(gd.cpu().numpy(), want), (name, k)
        xd = dev(x)
        assert shift(xd, 0) is xd
    # every width of the copy: rows of 1, 2, 4, 8 and 16 bytes, and a base that is only byte-aligned
    for width in (1, 2, 4, 8, 16):
        x = O.raw_int8(37 * width, width).reshape(37, width)
        assert np.array_equal(shift(x, 5), O.shift(x, 5)) and np.array_equal(shift(x, -36), O.shift(x, -36))
    flat = dev(O.raw_int8(16 * 40 + 1, 7))
    odd = flat[1:].view(40, 16)
    assert np.array_equal(shift(odd, 3).cpu().numpy(), O.shift(odd.cpu().numpy(), 3))


def test_offset_compensation(gpu_ready, gold):
    from passiveradar_amd.signal_utils import offset_compensation, shift
    x1 = O.offset_input()
    for d in O.OFFSETS:
        x2 = shift(x1, d)
        out = offset_compensation(x1, x2, 20000, 4, 200)
        g = gold["misc"][f"off_{d}"]
        assert (out is x2) == bool(g[1]) == (d == 0)
        assert np.array_equal(O.checksum(out.view(np.float32).view(np.int8)), g[2:]), d      # the reference's result, bit for bit
        assert np.array_equal(out[12:-12], x1[12:-12])
        d1, d2 = dev(x1), dev(x2)
        od = offset_compensation(d1, d2, 20000, 4, 200)
        assert od.is_cuda and (od is d2) == (d == 0) and same_bits(od, out)


def test_normalize(gpu_ready, gold):
    from passiveradar_amd.signal_utils import normalize
    for shape in O.NORMALIZE_SHAPES:
        for dtype in ("float32", "complex64"):
            x = O.normalize_input(shape, dtype)
            want = gold["misc"][f"norm_{dtype}_" + "x".join(map(str, shape))]
            got = normalize(x)
            assert got.shape == shape and got.dtype == np.dtype(dtype)
            gd = normalize(dev(x))
            assert gd.is_cuda and tuple(gd.shape) == shape and same_bits(gd, got)
            sub = got.reshape(-1)[::O.NORMALIZE_STRIDE] if got.size >= 1000 else got
            err = rel_err(sub, want)
            print(f"normalize {dtype} {shape}: {err:.3g}")
            assert err <= NORM_BAR, (shape, dtype, err)
    for name, want in (("complex128", np.complex128), ("float64", np.float64), ("int16", np.float64)):
        x = O.dtype_input(name)
        y = normalize(x)
        assert y.dtype == want and rel_err(y, O.normalize(x)) <= NORM_BAR, name


def test_two_calls_give_the_same_bits(gpu_ready):
    import torch
    from passiveradar_amd.signal_utils import channel_preprocessing, decimate, normalize
    x = dev(O.white(30000, 91))
    raw = dev(O.raw_int8(60000, 92))
    for q in (10, O.TILE_MAX_Q, O.TILE_MAX_Q + 1, 97):
        a, b = decimate(x, q), decimate(x, q)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), q
        a, b = channel_preprocessing(raw, q, 1e5, 2.4e6), channel_preprocessing(raw, q, 1e5, 2.4e6)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), q
    a, b = normalize(x), normalize(x)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def _decimate_raw(lib, _lib, raw, q, n, mix=0, fc=0.0, fs=1.0, step=1, stride=0, nch=1):
    """prc_fir_decimate on an int8 device tensor, dense output [nch][ceil(n / q)]"""
    import torch
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix, d.fc, d.fs = q, 20 * q + 1, _lib.RAW_DTYPES["int8"], mix, fc, fs
    taps = dev(O.taps32(q))
    m = O.out_len(n, q)
    out = torch.empty((nch, m), dtype=torch.complex64, device="cuda")
    _lib.check(lib.prc_fir_decimate(C.byref(d), taps.data_ptr(), raw.data_ptr(), n, step, stride, nch, out.data_ptr(), 1, m,
                                    _lib.torch_stream_ptr()))
    torch.cuda.synchronize()
    return out


def test_addressing_past_2_31_bytes(gpu_ready):
    """an int8 recording of 2^31 + 2^16 scalars, rotation off: the last 64 outputs equal those of the same samples run as
    a short array, so no byte offset on the load path wraps at 2^31 (the sums of an output do not depend on where it is)"""
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    q = 10
    nscalars = 2 ** 31 + 2 ** 16
    n = nscalars // 2
    big = torch.zeros(nscalars, dtype=torch.int8, device="cuda")
    keep = 2 * q * 512                                               # the last 512 outputs' worth of samples, q-aligned
    start = (n - keep // 2) // q * q
    tail = dev(O.raw_int8(2 * (n - start), 93))
    big[2 * start:] = tail
    far = _decimate_raw(lib, _lib, big, q, n)[0]
    near = _decimate_raw(lib, _lib, tail, q, n - start)[0]
    assert far.shape[0] == O.out_len(n, q) and bool((far[-64:].abs() > 0).all())
    assert torch.equal(torch.view_as_real(far[-64:]), torch.view_as_real(near[-64:]))


@pytest.mark.parametrize("q", [10, O.TILE_MAX_Q + 1], ids=["tile", "direct"])
@pytest.mark.parametrize("mix", [0, 1])
def test_guard_bands_fir_decimate(gpu_ready, q, mix, gap=1001, far_in=0):
    """two int8 channels interleaved sample by sample (step 2, channel stride 1), a tile and a half of outputs: the input is
    ONE guarded block of both channels, the output two blocks at a stride longer than their extent (``gap``; with ``far_in``
    the channels are two input blocks of step 1 that many samples apart: tests/test_gpu_far_blocks.py passes 4 GiB)"""
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    n = 384 * q - 3
    m = O.out_len(n, q)
    fc, fs = 1e5, 2.4e6
    chans = [O.raw_int8(2 * n, 94 + c) for c in range(2)]
    both = np.empty(4 * n, np.int8)
    both.reshape(-1, 2, 2)[:, 0, :] = chans[0].reshape(-1, 2)
    both.reshape(-1, 2, 2)[:, 1, :] = chans[1].reshape(-1, 2)
    d = _lib.FirdecDesc()
    d.q, d.ntaps, d.raw_dtype, d.mix, d.fc, d.fs = q, 20 * q + 1, _lib.RAW_DTYPES["int8"], mix, fc, fs
    taps = guard.guarded_input(dev(O.taps32(q)).reshape(1, -1), 20 * q + 1)
    st = _lib.torch_stream_ptr()

    def run(a, s):
        step, stride = (1, s["x"] // 2) if far_in else (2, 1)
        _lib.check(lib.prc_fir_decimate(C.byref(d), taps.data_ptr(), a["x"].data_ptr(), n, step, stride, 2, a["out"].data_ptr(), 1,
                                        s["out"], st))
        torch.cuda.synchronize()

    x = guard.In(dev(np.stack(chans)), 2 * (n + far_in)) if far_in else guard.In(dev(both).reshape(1, -1))
    got = guard.check(run, {"x": x}, {"out": guard.Out(2, m, torch.complex64, stride=m + gap)})
    out = got.tight["out"].cpu().numpy()
    for c in range(2):
        z = O.tuned(chans[c], fc, fs) if mix else O.deinterleave(chans[c])
        assert rel_err(out[c], O.fir_decimate(z, q)) <= BAR, c


def test_guard_bands_shift_and_normalize(gpu_ready):
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    st = _lib.torch_stream_ptr()
    rows, width = 41, 6
    x = O.raw_int8(rows * width, 96).reshape(rows, width)
    x[x == -91] = 1                                                  # 0xA5 is the guard's own sentinel for bytes
    for k in (7, -7, rows + 2):
        def run(a, s):
            _lib.check(lib.prc_shift(a["x"].data_ptr(), a["y"].data_ptr(), rows, width, k, st))
            torch.cuda.synchronize()
        got = guard.check(run, {"x": guard.In(dev(x).reshape(1, -1))}, {"y": guard.Out(1, rows * width, torch.int8, finite=False)})
        assert np.array_equal(got.tight["y"].cpu().numpy().reshape(rows, width), O.shift(x, k)), k
    for dtype, tdt in (("float32", torch.float32), ("complex64", torch.complex64)):
        n = 3 * 8192 + 5                                             # four workgroups of partial sums, the last one ragged
        x = O.normalize_input((n,), dtype)
        ws = C.c_size_t(0)
        _lib.check(lib.prc_normalize_workspace_bytes(n, C.byref(ws)))
        assert ws.value == 32

        def run(a, s):
            _lib.check(lib.prc_normalize(a["x"].data_ptr(), a["y"].data_ptr(), n, int(dtype == "complex64"),
                                         a["workspace"].data_ptr(), st))
            torch.cuda.synchronize()
        got = guard.check(run, {"x": guard.In(dev(x).reshape(1, -1))},
                          {"y": guard.Out(1, n, tdt), "workspace": guard.Out(1, ws.value // 8, torch.float64)})
        assert rel_err(got.tight["y"].cpu().numpy().reshape(-1), O.normalize(x)) <= NORM_BAR, dtype


def test_device_tensors_stay_on_their_device_and_stream(gpu_ready):
    """the launches go to torch's CURRENT stream: on a side stream, behind a chain of kernels that is still producing the
    input, they see the finished input"""
    import torch
    from passiveradar_amd.signal_utils import channel_preprocessing, decimate, normalize, shift
    x = dev(O.white(200000, 97))
    raw = dev(O.raw_int8(400000, 98))
    want = [decimate(x, 10), channel_preprocessing(raw, 10, 1e5, 2.4e6), shift(x, 5), normalize(x)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xs, rs = torch.zeros_like(x), torch.zeros_like(raw)
        for _ in range(50):                                          # work the launches must wait behind
            xs = xs * 0.5 + x * 0.5
        xs = xs * 0 + x
        rs = rs + raw
        got = [decimate(xs, 10), channel_preprocessing(rs, 10, 1e5, 2.4e6), shift(xs, 5), normalize(xs)]
    side.synchronize()
    for a, b in zip(got, want):
        assert a.device == x.device and a.dtype == b.dtype
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
