"""Guard bands around the device arguments of prc_fuse (tests/guard.py, as tests/test_gpu_tbd_bounds.py uses it): the
K x nframes maps lie at a stride larger than a map inside one allocation whose every other element is NaN, best and vel in
allocations filled with a sentinel, every base only element-aligned.  A sample read outside a map is a NaN: under sum it makes
its hypothesis NaN, which is never chosen, under min it is passed over or stays -- either way a cell that should have chosen
that hypothesis changes its best or its vel, and the payload differs from the tight call's and from the oracle.  The geometry
sends columns and rows off the map at both ends, so the range tests are what keeps every index inside."""
import numpy as np
import pytest

import fuse_oracle as FO
import guard

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("form", [None, 1, 2])
@pytest.mark.parametrize("combine", [FO.SUM, FO.MIN])
@pytest.mark.parametrize("with_vel", [True, False])
def test_fuse_guard_bands(gpu_ready, with_vel, combine, form):
    import torch
    from passiveradar_amd import _lib, engine
    stat, il, rx, grid, vels, z = FO.random_case(61, 3, 33, 19, 13, 9, 5, 7, 3)
    K, nf, H, W = stat.shape
    ny, nx = grid[5], grid[2]
    rows = FO.illum_rows(il, rx)
    r, c = FO.cells(rows, rx, grid, vels, z)
    assert (c < 0).any() and (c > W - 1).any() and (r < 0).any() and (r > H - 1).any()
    d = engine.fuse_desc(K, H, W, grid, vels, rx, z, combine, form)
    st = _lib.torch_stream_ptr()

    def run(args, strides):
        s = strides["stat"]                          # map (k, f) is block k nf + f
        engine.fuse_execute(d, rows, args["stat"], nf * s, s, nf, args["best"], args.get("vel"), st)
        torch.cuda.synchronize()

    ins = {"stat": guard.In(dev(stat).reshape(K * nf, H * W), stride=H * W + 37)}
    outs = {"best": guard.Out(1, nf * ny * nx, torch.float32)}
    if with_vel:
        outs["vel"] = guard.Out(1, nf * ny * nx, torch.int32)
    got = guard.check(run, ins, outs)
    want = FO.fuse(stat, rows, rx, grid, vels, z, combine)
    assert np.array_equal(got.tight["best"].cpu().numpy().reshape(nf, ny, nx), want[0])
    if with_vel:
        assert np.array_equal(got.tight["vel"].cpu().numpy().reshape(nf, ny, nx), want[1])


def test_same_result_after_other_uses_of_the_device(gpu_ready):
    """the LDS image, the band table and the copy of the illuminator rows are rebuilt by every workgroup: a call between two
    equal calls (another shape, more illuminators, the other form; then another entry point that fills the LDS) changes nothing"""
    import torch
    from passiveradar_amd.target_detection import fuse_maps, track_before_detect
    a = FO.random_case(62, 3, 33, 19, 17, 13, 9, 9, 2)
    b = FO.random_case(63, 8, 5, 130, 5, 7, 3, 5, 1)
    xa, xb = dev(a[0]), dev(b[0])
    first = fuse_maps(xa, *a[1:], form=2)
    fuse_maps(xb, *b[1:], form=2)
    fuse_maps(xb, *b[1:], form=1)
    track_before_detect(torch.rand((4, 64, 96), device="cuda"))
    again = fuse_maps(xa, *a[1:], form=2)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    want = FO.fuse(a[0], FO.illum_rows(a[1], a[2]), *a[2:])
    assert np.array_equal(again[0].cpu().numpy(), want[0]) and np.array_equal(again[1].cpu().numpy(), want[1])
