"""Guard bands around every device argument of prc_cfar_os (tests/guard.py, as tests/test_gpu_patch_bounds.py uses it):
NaN-poisoned lead and tail around X, sentinels around out, the noise map and the workspace.  Nothing outside the documented
extents is read (the results are those of tight, exactly-sized arguments, bit for bit, and finite) or written -- at a
frame smaller than the window (every index wraps more than once) and at one a cell larger than a tile, stacks of three."""
import numpy as np
import pytest

import cfar_os_oracle as OS
import guard

pytestmark = pytest.mark.gpu

NF = 3


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("scale", ["reference", "plain"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shape", [(5, 7), (17, 65)])
def test_guard_bands(gpu_ready, shape, cplx, scale, with_noise):
    import torch
    from passiveradar_amd import _lib, engine
    H, W = shape
    rng = np.random.default_rng(H)
    x = (rng.standard_normal((NF, H, W)) + 1j * rng.standard_normal((NF, H, W))).astype(np.complex64)
    xin = x if cplx else np.abs(x)
    d = engine.cfar_os_desc(H, W, 18, 4, None, scale, cplx)
    nws = engine.cfar_os_workspace_bytes(d, NF)
    assert nws == (0 if scale == "plain" else 4 * 64 * NF)
    st = _lib.torch_stream_ptr()

    def run(args, s):
        engine.cfar_os_execute(d, args["X"], args["out"], args.get("noise"), NF, args.get("workspace"), st)
        torch.cuda.synchronize()

    outs = {"out": guard.Out(NF, H * W, torch.float32)}
    if with_noise:
        outs["noise"] = guard.Out(NF, H * W, torch.float32)
    if nws:
        outs["workspace"] = guard.Out(1, nws // 4, torch.float32)
    got = guard.check(run, {"X": guard.In(dev(xin).reshape(1, -1))}, outs)
    # the tight call against the unguarded front end, bit for bit, and against the oracle
    from passiveradar_amd.target_detection import CFAR_2D_OS
    r, z = CFAR_2D_OS(dev(xin), 18, 4, scale=scale, return_noise=True)
    assert torch.equal(got.tight["out"].reshape(NF, H, W), r)
    if with_noise:
        assert torch.equal(got.tight["noise"].reshape(NF, H, W), z)
    if not cplx:
        for f in range(NF):
            assert np.array_equal(z[f].cpu().numpy(), OS.noise(xin[f], 18, 4))
