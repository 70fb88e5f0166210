"""Guard bands around every device argument of prc_batch_xambg and prc_ofdm_timing (tests/guard.py, as
tests/test_gpu_channelize_bounds.py uses it): ref and srv as three frames at a stride above their length, each frame ending
exactly at start + (F - 1) hop + L and its first `start` samples, which no batch covers, poisoned as well; the window; the
workspace (an output whose padding columns need not be written); out; metric_out and start_out.  Both batch lengths, both
filters.  The NaN poison reaches the result through any over-read, an over-write shows as a changed sentinel, and the tight
call is held to the oracle."""
import numpy as np
import pytest

import batch_xambg_oracle as O
import guard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_resident(gpu_ready):
    yield
    O.release_device_leftovers()


@pytest.mark.parametrize("filt", [O.RECIPROCAL, O.MATCHED])
@pytest.mark.parametrize("L,F,R,hop,start", [(1024, 256, 40, 1100, 5), (1024, 512, 16, 1024, 0), (4096, 256, 70, 4100, 3),
                                            (4096, 256, 4095, 4096, 1)])
def test_batch_xambg_guard_bands(gpu_ready, L, F, R, hop, start, filt):
    import torch
    from passiveradar_amd import _lib, engine
    nf = 3
    n = start + (F - 1) * hop + L                                                # the last batch ends with the frame
    refs = np.stack([O.white(n, 10 + b) for b in range(nf)])
    srvs = np.stack([(0.7 * np.roll(refs[b], 9) + 0.1 * O.white(n, 20 + b)).astype(np.complex64) for b in range(nf)])
    w = np.hanning(F + 2)[1:-1].astype(np.float32)
    want = O.stack(refs, srvs, L, F, R, hop, start, filt, 0.1, w)
    poisoned = lambda a: torch.from_numpy(np.concatenate([np.full((nf, start), np.nan + 1j * np.nan, np.complex64), a[:, start:]], axis=1)).cuda()
    d = engine.batch_xambg_desc(n, L, R, F, hop, start, _lib.BATCH_FILTERS[filt], 0.1)
    nws = engine.batch_xambg_workspace_bytes(d, nf) // 8
    st = _lib.torch_stream_ptr()

    def run(a, s):
        assert s["ref"] == s["srv"]
        engine.batch_xambg_execute(d, a["ref"], a["srv"], s["ref"], a["window"], a["out"], nf, a["workspace"], st)
        torch.cuda.synchronize()

    ins = {"ref": guard.In(poisoned(refs), stride=n + 37), "srv": guard.In(poisoned(srvs), stride=n + 37),
           "window": guard.In(torch.from_numpy(w).cuda().reshape(1, -1))}
    outs = {"out": guard.Out(1, nf * F * (R + 1), torch.complex64),
            "workspace": guard.Out(1, nws, torch.complex64, promised=torch.zeros((1, nws), dtype=torch.bool), finite=False)}
    got = guard.check(run, ins, outs)
    err = O.rel_err(got.tight["out"].cpu().numpy().reshape(nf, F, R + 1), want)
    print(f"prc_batch_xambg L = {L} F = {F} R = {R} {filt}: {err:.3g}")
    assert err <= O.GPU_BAR, (L, F, R, filt, err)


@pytest.mark.parametrize("nfft,cp,nsym", [(1024, 128, 4), (100, 7, 3)])
def test_ofdm_timing_guard_bands(gpu_ready, nfft, cp, nsym):
    import torch
    from passiveradar_amd import _lib, engine
    sym = nfft + cp
    n = (nsym + 1) * sym + nfft                                                  # the shortest legal length
    body = O.white((nsym + 3) * nfft, 5).reshape(nsym + 3, nfft)
    x = np.roll(np.concatenate([body[:, nfft - cp:], body], axis=1).reshape(-1), 41)[:n].astype(np.complex64)
    wm = O.timing_metric(x, nfft, cp, nsym)
    st = _lib.torch_stream_ptr()

    def run(a, s):
        engine.ofdm_timing(a["ref"], n, nfft, cp, nsym, a["metric_out"], a["start_out"], st)
        torch.cuda.synchronize()

    got = guard.check(run, {"ref": guard.In(torch.from_numpy(x).cuda().reshape(1, -1))},
                      {"metric_out": guard.Out(1, sym, torch.float64), "start_out": guard.Out(1, 1, torch.int32)})
    m = got.tight["metric_out"].cpu().numpy()[0]
    assert float(np.abs(m - wm).max() / wm.max()) <= O.TIMING_BAR
    assert int(got.tight["start_out"].cpu().numpy()[0, 0]) == int(np.argmax(wm)) == 41
