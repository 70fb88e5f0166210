"""The polyphase filter bank without a GPU: tests/channelize_oracle.py against an independent statement of the definition,
streaming continuity, a tone's known answer, the float32 emulations of the two kernels' summation orders (their worst error
is the input of the GPU bar, tests/test_gpu_channelize.py), and the front door's argument checks, which all precede the first
device call.

Worst emulated error against the float64 definition, every case, int8 and complex64 inputs: tile order 4.4e-7 at
(4100, 100, 50), direct order 1.4e-7 at (600, 8, 74); so the GPU bar is 4 x 4.4e-7 = 1.8e-6, rounded up to 2e-6."""
import numpy as np
import pytest

import channelize_oracle as O
import preproc_oracle as P

def _starts(label):
    return (0, O.FAR_START) if label == "2000_12_12" else (0,)


@pytest.mark.parametrize("case", O.all_cases(), ids=lambda c: c[0])
def test_oracle_against_rotate_then_decimate(case):
    """row i is the FIR decimation of the stream rotated by exp(-2 pi i ((k_i (start + m)) mod M) / M): through
    preproc_oracle.fir_decimate with the default taps, through np.convolve with custom ones"""
    label, n, M, D, ch, taps = case
    for dtype in ("int8", "complex64"):
        x = O.case_input(n, M, D, dtype)
        for start in _starts(label):
            got = O.channelize(x, M, D, ch, taps, start)
            assert got.shape == (len(ch), O.out_len(n, D))
            for i, k in enumerate(ch):
                z = O.rotated(x, M, k, start)
                if taps is None:
                    want = P.fir_decimate(z, D)
                else:
                    want = np.convolve(z, taps.astype(np.float64))[(len(taps) - 1) // 2::D][:got.shape[1]]
                assert O.rel_err(got[i], want) <= 1e-12, (label, dtype, start, k)


def test_a_later_block_continues_the_stream():
    """the block x[s0:] with start = s0 gives the whole stream's outputs away from its edges, bit for bit in float64 (the same
    products in the same order) -- for s0 a multiple of D against the whole stream, for s0 = 1205 against the stream cut at 5"""
    M = D = 12
    ch = [0, 5, -1]
    raw = O.case_input(4800, M, D)
    edge = 11                                                         # c / D = 10 outputs either side see the block's edge
    for s0, base in ((1200, 0), (1205, 5)):
        whole = O.channelize(raw[2 * base:], M, D, ch, start=base)
        block = O.channelize(raw[2 * s0:], M, D, ch, start=s0)
        skip = (s0 - base) // D
        diff = np.abs(block[:, edge:-edge] - whole[:, skip + edge:-edge]).max()
        print(f"block from {s0} against the stream from {base}: {diff:.3g}")
        assert diff == 0.0, (s0, diff)
    # and it is the phase that does it: the same block taken as a stream of its own (start = 0) is another signal
    alone = O.channelize(raw[2 * 1205:], M, D, [5])
    assert O.rel_err(alone[:, edge:-edge], block[1:2, edge:-edge]) > 0.1


def test_tone_known_answer():
    """M = D = 12: a tone at (5/12 + 0.003) Fs comes out of channel 5 at the taps' own pass-band gain, 1.0025, and of its
    neighbours and of channel 0 below 4e-4"""
    M = D = 12
    x = np.exp(2j * np.pi * (5 / 12 + 0.003) * np.arange(6000)).astype(np.complex64)
    y = O.channelize(x, M, D, [5, 4, 6, 0])
    amp = np.abs(y[:, 20:-20])
    print(f"channel 5: {amp[0].min():.6f} .. {amp[0].max():.6f}; channels 4, 6, 0: {amp[1].max():.3g}, {amp[2].max():.3g}, {amp[3].max():.3g}")
    assert np.abs(amp[0] - 1.0025).max() <= 1e-4
    assert amp[1:].max() < 4e-4
    # the tone leaves channel 5 at 0.003 Fs = 0.036 cycles per output sample
    step = np.angle(y[0, 21:-20] * np.conj(y[0, 20:-21]))
    assert np.abs(step - 2 * np.pi * 0.003 * D).max() <= 1e-6


def test_emulated_orders_set_the_gpu_bar():
    """float32 in the kernels' own order against the float64 definition on every case: 4 x the worst, rounded up to one
    digit and capped at 1e-4, is the bar of the GPU tests (fused multiply-adds account for the factor)"""
    worst = {"tile": (0.0, None), "direct": (0.0, None)}
    for label, n, M, D, ch, taps in O.all_cases():
        for dtype in ("int8", "complex64"):
            x = O.case_input(n, M, D, dtype)
            for start in _starts(label):
                want = O.channelize(x, M, D, ch, taps, start)
                for name, emulate in (("tile", O.emulate_tile), ("direct", O.emulate_direct)):
                    e = O.rel_err(emulate(x, M, D, ch, taps, start), want)
                    if e > worst[name][0]:
                        worst[name] = (e, (label, dtype, start))
    print(f"worst emulated error: tile order {worst['tile'][0]:.3g} at {worst['tile'][1]}, direct order "
          f"{worst['direct'][0]:.3g} at {worst['direct'][1]}")
    w = 4 * max(worst["tile"][0], worst["direct"][0])
    digit = 10.0 ** np.floor(np.log10(w))
    bar = min(float(np.ceil(w / digit - 1e-9) * digit), 1e-4)
    assert np.isclose(bar, O.GPU_BAR, rtol=1e-9, atol=0), (worst, bar)


def test_emulations_do_not_depend_on_the_other_channels():
    """a row of either emulation is the row of the channel asked for alone: the orders sum every channel on its own"""
    n, M, D, ch = O.CASES[0]
    x = O.case_input(n, M, D)
    for emulate in (O.emulate_tile, O.emulate_direct):
        both = emulate(x, M, D, ch)
        for i, k in enumerate(ch):
            assert np.array_equal(both[i], emulate(x, M, D, [k])[0]), k
        assert np.array_equal(emulate(x, M, D, [-1])[0], emulate(x, M, D, [M - 1])[0])


def test_front_door_refuses_bad_arguments_before_any_device_call():
    from passiveradar_amd import signal_utils
    from passiveradar_amd.signal_utils import channelize
    assert "channelize" in signal_utils.__all__
    raw = np.zeros(64, np.int8)
    with pytest.raises(TypeError):
        channelize(raw, 12, 10.0)
    for bad_dec in (1, 0, -3):
        with pytest.raises(ValueError):
            channelize(raw, 12, bad_dec)                              # default taps need dec >= 2
    for bad_taps in (np.zeros(0, np.float32), np.ones(4, np.float32), np.ones((3, 3), np.float32)):
        with pytest.raises(ValueError):
            channelize(raw, 12, 2, taps=bad_taps)
    with pytest.raises(ValueError):
        channelize(raw, 12, 0, taps=np.ones(3, np.float32))
    for bad_m in (1, 0, 257):
        with pytest.raises(ValueError):
            channelize(raw, bad_m, 2)
    for bad_ch in ([12], [-7], [0, 1, 99], [0.5], [[0, 1]]):
        with pytest.raises(ValueError):
            channelize(raw, 12, 2, bad_ch)
    with pytest.raises(ValueError):
        channelize(raw, 5, 2, [-3])                                   # -M / 2 = -2.5: -2 is the lowest channel of five
    with pytest.raises(ValueError):
        channelize(raw.reshape(8, 8), 12, 2)
    # nothing to compute: no device is asked for it
    for empty in (np.zeros(0, np.int8), np.zeros(1, np.int8), np.zeros(0, np.complex64)):
        y = channelize(empty, 12, 2, [0, 5, -1])
        assert y.shape == (3, 0) and y.dtype == np.complex64
    assert channelize(np.zeros(0, np.int16), 4, 3).shape == (4, 0)


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    """prc_channelize's own checks, with their messages: they precede the launch, so fake (aligned, non-null) addresses do"""
    import ctypes as C
    from passiveradar_amd import _lib
    lib = _lib.lib()

    def call(n=100, out_stride=50, taps=64, tw=64, ch=64, x=64, out=64, **fields):
        d = _lib.ChannelizeDesc()
        d.nchan, d.dec, d.ntaps, d.raw_dtype, d.nsel, d.start = 12, 2, 41, 0, 2, 0
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib.prc_channelize(C.byref(d), taps, tw, ch, x, n, out, out_stride, None)
        return rc, lib.prc_last_error().decode()

    assert lib.prc_channelize(None, 64, 64, 64, 64, 1, 64, 1, None) == _lib.PRC_EINVAL
    for fields, code, word in (({"nchan": 1}, _lib.PRC_EINVAL, "nchan = 1"), ({"nchan": 257}, _lib.PRC_EINVAL, "nchan = 257"),
                               ({"dec": 0}, _lib.PRC_EINVAL, "dec = 0"), ({"ntaps": 40}, _lib.PRC_EINVAL, "ntaps = 40"),
                               ({"ntaps": 0}, _lib.PRC_EINVAL, "ntaps = 0"), ({"ntaps": 2 ** 24 + 1}, _lib.PRC_ESHAPE, "2^24"),
                               ({"raw_dtype": 5}, _lib.PRC_EINVAL, "raw_dtype = 5"), ({"nsel": 0}, _lib.PRC_EINVAL, "nsel = 0"),
                               ({"nsel": 65}, _lib.PRC_EINVAL, "nsel = 65"), ({"magic": 0}, _lib.PRC_EINVAL, "magic"),
                               ({"struct_size": 32}, _lib.PRC_EINVAL, "struct_size = 32")):
        rc, msg = call(**fields)
        assert rc == code and "prc_channelize" in msg and word in msg, (fields, rc, msg)
    for kw, word in (({"n": -1}, "n = -1"), ({"out_stride": 49}, "out_stride = 49"), ({"x": None}, "null"), ({"taps": None}, "null"),
                     ({"tw": None}, "null"), ({"ch": None}, "null"), ({"out": None}, "null"), ({"out": 68}, "alignment"),
                     ({"tw": 68}, "alignment"), ({"taps": 66}, "alignment"), ({"ch": 66}, "alignment")):
        rc, msg = call(**kw)
        assert rc == _lib.PRC_EINVAL and word in msg, (kw, rc, msg)
    assert call(n=0)[0] == _lib.PRC_OK                               # nothing to do, nothing launched
    assert call(n=0, out_stride=0, nsel=1)[0] == _lib.PRC_OK


def test_descriptor_and_constants_match_the_header(tmp_path):
    """prc_channelize_desc as gcc lays it out against the ctypes mirror, and the constants _lib.py and the oracle restate"""
    import ctypes
    import shutil
    import subprocess
    from conftest import REPO
    from passiveradar_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "cz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/prcore.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %u %d %d %d %d\\n", sizeof(prc_channelize_desc), offsetof(prc_channelize_desc, nchan),\n'
                   '         offsetof(prc_channelize_desc, nsel), offsetof(prc_channelize_desc, start), PRC_CHANNELIZE_DESC_SIZE_680,\n'
                   '         PRC_CHANNELIZE_MAX_CHAN, PRC_CHANNELIZE_MAX_SEL, PRC_CHANNELIZE_TILE_MAX_BYTES, (int)PRC_OPT_CHANNELIZE_FORM);\n'
                   '  return 0; }\n')
    exe = tmp_path / "cz"
    subprocess.check_call(["gcc", "-I", REPO, str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    D = _lib.ChannelizeDesc
    assert got == [ctypes.sizeof(D), D.nchan.offset, D.nsel.offset, D.start.offset, ctypes.sizeof(D), _lib.CHANNELIZE_MAX_CHAN,
                   _lib.CHANNELIZE_MAX_SEL, _lib.CHANNELIZE_TILE_MAX_BYTES, _lib.OPT_CHANNELIZE_FORM]
    assert (O.MAX_SEL, O.TILE_MAX_BYTES) == (_lib.CHANNELIZE_MAX_SEL, _lib.CHANNELIZE_TILE_MAX_BYTES)
    # the option that forces the direct form: default, round trip, range -- no device needed
    assert _lib.get_option(_lib.OPT_CHANNELIZE_FORM) == 0
    old = _lib.set_option(_lib.OPT_CHANNELIZE_FORM, 1)
    try:
        assert old == 0 and _lib.get_option(_lib.OPT_CHANNELIZE_FORM) == 1
    finally:
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, old)
    with pytest.raises(ValueError):
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, 2)
