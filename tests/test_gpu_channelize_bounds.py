"""Guard bands around every device argument of prc_channelize (tests/guard.py, as tests/test_gpu_echo_bounds.py uses it): x
in every raw dtype, taps, twiddles, channels, and out at a stride above its rows -- n = 1, n below the filter length, n one
sample past a tile of 256 outputs -- in the tile form and in the direct form.  The NaN poison around the floating arguments
reaches the result through any over-read; channels is an integer argument, so every case runs with the gaps of the integer
arguments filled with 0 and with the type's maximum (for the integer raw types that is x as well), and the two fills must
agree bit for bit; an over-write shows as a changed sentinel.  The tight call is held to the oracle."""
import ctypes as C

import numpy as np
import pytest

import channelize_oracle as O
import guard

pytestmark = pytest.mark.gpu

M, D, CH = 12, 10, [1, -5, 7]
L = 20 * D + 1
SIZES = [1, L - 60, O.TILE_OUTPUTS * D + 1]


@pytest.mark.parametrize("form", ["tile", "direct"])
@pytest.mark.parametrize("dtype", O.DTYPES)
def test_channelize_guard_bands(gpu_ready, dtype, form):
    import torch
    from passiveradar_amd import _lib
    lib = _lib.lib()
    st = _lib.torch_stream_ptr()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cs, sn = O.twiddles32(M)
    tw = (cs + 1j * sn).astype(np.complex64)
    old = _lib.set_option(_lib.OPT_CHANNELIZE_FORM, int(form == "direct"))
    try:
        for n in SIZES:
            x = O.case_input(n, M, D, dtype)
            m = O.out_len(n, D)
            d = _lib.ChannelizeDesc()
            d.nchan, d.dec, d.ntaps, d.raw_dtype, d.nsel, d.start = M, D, L, _lib.RAW_DTYPES[dtype], len(CH), 7

            def run(a, s):
                _lib.check(lib.prc_channelize(C.byref(d), a["taps"].data_ptr(), a["twiddles"].data_ptr(), a["channels"].data_ptr(),
                                              a["x"].data_ptr(), n, a["out"].data_ptr(), s["out"], st))
                torch.cuda.synchronize()

            ins = {"x": guard.In(dev(x).reshape(1, -1)), "taps": guard.In(dev(O.taps32(D)).reshape(1, -1)),
                   "twiddles": guard.In(dev(tw).reshape(1, -1)), "channels": guard.In(dev(np.array(CH, np.int32)).reshape(1, -1))}
            got = guard.check(run, ins, {"out": guard.Out(len(CH), m, torch.complex64, stride=m + 37)})
            err = O.rel_err(got.tight["out"].cpu().numpy(), O.channelize(x, M, D, CH, start=7))
            print(f"prc_channelize {dtype} n = {n} ({form}): {err:.3g}")
            assert err <= O.GPU_BAR, (dtype, n, form, err)
    finally:
        _lib.set_option(_lib.OPT_CHANNELIZE_FORM, old)
