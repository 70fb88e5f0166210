"""Guard bands around every device argument of prc_echo_cancel (tests/guard.py, as tests/test_gpu_tbd_bounds.py uses it): ref,
srv, atoms, counts, out, fit and info over a three-frame stack with strides above n.  The guard's NaN poison propagates through
the definition (a NaN that reaches a Gram sum breaks the frame's solve down or ends in out), so an over-read of ref or srv shows
as a flagged frame, a non-finite result or a difference from the tight call; an over-read of the integer arguments as a
difference between the two fills; an over-write as a changed sentinel.  The tight call is held to the oracle."""
import numpy as np
import pytest

import echo_oracle as EO
import guard

pytestmark = pytest.mark.gpu

NF, N, M, FS = 3, 1100, 4, 1100.0
STRIDE, OUT_STRIDE = N + 29, N + 13


def scene(wrap):
    rng = np.random.default_rng(51)
    white = lambda: ((rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2)).astype(np.complex64)
    ref = np.stack([white() for _ in range(NF)])
    # (without wrap an atom at lag n - 1 is one sample long and its slope column is a multiple of it: a breakdown, not this test)
    lags = [[0, 17], [N - 1 if wrap else 40, 5, -3], []]
    dops = [[2.2, -4.4], [1.1, 7.3, -6.6], []]
    srv = np.stack([sum((EO.echo(ref[b], l, f, FS, 1.0 / (1 + k), True) for k, (l, f) in enumerate(zip(lags[b], dops[b]))),
                        1e-3 * white().astype(np.complex128)) for b in range(NF)]).astype(np.complex64)
    return ref, srv, lags, [[f + 0.2 for f in d] for d in dops]


@pytest.mark.parametrize("wrap", [True, False])
def test_echo_cancel_guard_bands(gpu_ready, wrap, NF=NF, STRIDE=STRIDE, OUT_STRIDE=OUT_STRIDE):
    """``NF``, ``STRIDE``, ``OUT_STRIDE``: tests/test_gpu_far_blocks.py runs the first two frames 4 GiB apart"""
    import torch
    from passiveradar_amd import _lib, engine
    ref, srv, lags, dops = scene(wrap)
    ref, srv = ref[:NF], srv[:NF]
    rec = np.zeros((NF, M), _lib.ECHO_ATOM_DTYPE)
    rec["lag"], rec["doppler"] = 2 ** 31 - 1, np.nan           # what the slots beyond a count hold: never read
    counts = np.zeros(NF, np.int32)
    for b in range(NF):
        k = len(lags[b])
        rec["lag"][b, :k], rec["doppler"][b, :k], counts[b] = lags[b], dops[b], k
    st = _lib.torch_stream_ptr()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def run(args, s):
        d = engine.echo_desc(N, FS, M, NF, wrap, True, 2, 0.0, s["ref"], s["out"])
        assert s["ref"] == s["srv"]
        ws = torch.full((engine.echo_workspace_bytes(d) + 16,), 0xFF, dtype=torch.uint8, device="cuda")
        ws = ws[(-ws.data_ptr()) % 16:]
        engine.echo_execute(d, args["ref"], args["srv"], args["atoms"], args["counts"], args["out"], args["fit"], args["info"], ws, st)
        torch.cuda.synchronize()

    ins = {"ref": guard.In(dev(ref), STRIDE), "srv": guard.In(dev(srv), STRIDE),
           "atoms": guard.In(dev(rec.view(np.int64).reshape(1, -1))), "counts": guard.In(dev(counts).reshape(1, -1))}
    outs = {"out": guard.Out(NF, N, torch.complex64, OUT_STRIDE), "fit": guard.Out(1, NF * M * 6, torch.int64, finite=False),
            "info": guard.Out(1, NF, torch.int32)}
    got = guard.check(run, ins, outs)
    out = got.tight["out"].cpu().numpy()
    fit = got.tight["fit"].cpu().numpy().view(_lib.ECHO_FIT_DTYPE).reshape(NF, M)
    info = got.tight["info"].cpu().numpy().reshape(-1)
    for b in range(NF):
        want, wfit, winfo = EO.cancel(ref[b], srv[b], FS, lags[b], dops[b], wrap=wrap)
        k = len(lags[b])
        assert info[b] == winfo == 0
        assert np.abs(out[b] - want).max() <= 2e-6 * np.abs(srv[b]).max()
        assert np.abs(fit[b]["doppler"][:k] - wfit["doppler"]).max(initial=0) <= 1e-6 * FS / N
        assert not fit[b][k:].view(np.uint8).any()
    if NF > 2:
        assert np.array_equal(out[2].view(np.uint32), srv[2].view(np.uint32))
