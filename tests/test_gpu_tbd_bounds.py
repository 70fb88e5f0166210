"""Guard bands around every device argument of prc_tbd and prc_tbd_trace (tests/guard.py, as tests/test_gpu_plots_bounds.py uses
it): stat, row_shift, prev, score, back, ends and paths at (33, 130) x 5 frames, with prev and back present and absent, in the
time-blocked form (one launch of five frames, and launches of two) and in the one-frame-per-launch form.  The guard's NaN
poison propagates through the definition (a NaN input stays in its cell's score; a NaN predecessor is never chosen, so a cell
that should have chosen the element it displaced changes its score or its code), so an over-read of stat, prev or an earlier
score frame shows as a non-finite result or as a difference from the tight call; an over-write as a changed sentinel."""
import numpy as np
import pytest

import guard
import tbd_oracle as TO

pytestmark = pytest.mark.gpu

NF, H, W = 5, 33, 130
I32 = np.iinfo(np.int32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene():
    rng = np.random.default_rng(41)
    stat = rng.rayleigh(1.0, (NF, H, W)).astype(np.float32)
    prev = rng.rayleigh(1.0, (H, W)).astype(np.float32)
    shifts = rng.integers(-6, 7, H).astype(np.int32)
    shifts[0], shifts[H - 1], shifts[7], shifts[8] = 3, -3, W + 1, -(W + 1)       # the edge rows reach across the edge columns
    return stat, prev, shifts


@pytest.mark.parametrize("form", [None, 2, 1])
@pytest.mark.parametrize("with_back", [True, False])
@pytest.mark.parametrize("with_prev", [True, False])
def test_tbd_guard_bands(gpu_ready, with_prev, with_back, form):
    import torch
    from passiveradar_amd import _lib, engine
    stat, prev, shifts = scene()
    d = engine.tbd_desc(H, W, 0.9, 2, 3, None, 0, 0)
    st = _lib.torch_stream_ptr()

    def run(args, s):
        engine.tbd_execute(d, args["stat"], args["row_shift"], args.get("prev"), NF, args["score"], args.get("back"), st, form)
        torch.cuda.synchronize()

    ins = {"stat": guard.In(dev(stat).reshape(1, -1)), "row_shift": guard.In(dev(shifts).reshape(1, -1))}
    if with_prev:
        ins["prev"] = guard.In(dev(prev).reshape(1, -1))
    outs = {"score": guard.Out(1, NF * H * W, torch.float32)}
    if with_back:
        outs["back"] = guard.Out(1, NF * H * W, torch.uint8)
    got = guard.check(run, ins, outs)
    want = TO.tbd(stat, 2, 3, 0.9, range_guard=0, doppler_guard=0, row_shift=shifts, prev=prev if with_prev else None)
    assert TO.same_bits(got.tight["score"].cpu().numpy().reshape(NF, H, W), want[0])
    if with_back:
        assert np.array_equal(got.tight["back"].cpu().numpy().reshape(NF, H, W), want[1])


@pytest.mark.parametrize("with_shifts", [True, False])
def test_trace_guard_bands(gpu_ready, with_shifts):
    import torch
    from passiveradar_amd import _lib, engine
    stat, prev, shifts = scene()
    _, back = TO.tbd(stat, 2, 3, 0.9, range_guard=0, doppler_guard=0, row_shift=shifts if with_shifts else None)
    back[2, ::4, ::5] = 200                                   # codes prc_tbd never writes ...
    back[3, 1::4, ::7] = 3                                    # ... and codes that point across an edge
    rng = np.random.default_rng(43)
    cells = np.concatenate((rng.choice(H * W, 60, replace=False), [0, W - 1, (H - 1) * W, H * W - 1]))
    ends = np.array([[f, c] for f in range(NF) for c in cells] + [[-1, 0], [NF, 0], [0, -1], [0, H * W], [I32.max, I32.max],
                                                                  [I32.min, I32.min]], dtype=np.int32)
    depth = NF + 2
    d = engine.tbd_desc(H, W, 0.9, 2, 3, None, 0, 0)
    st = _lib.torch_stream_ptr()

    def run(args, s):
        engine.tbd_trace(d, args["back"], args.get("row_shift"), NF, args["ends"], ends.shape[0], depth, args["paths"], st)
        torch.cuda.synchronize()

    ins = {"back": guard.In(dev(back).reshape(1, -1)), "ends": guard.In(dev(ends).reshape(1, -1))}
    if with_shifts:
        ins["row_shift"] = guard.In(dev(shifts).reshape(1, -1))
    got = guard.check(run, ins, {"paths": guard.Out(1, ends.shape[0] * depth, torch.int32)})
    want = TO.trace(back, ends, depth, 2, 3, shifts if with_shifts else None)
    assert np.array_equal(got.tight["paths"].cpu().numpy().reshape(-1, depth), want)
