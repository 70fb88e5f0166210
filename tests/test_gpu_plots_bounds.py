"""Guard bands around every device argument of prc_plots (tests/guard.py, as tests/test_gpu_cfar_os_bounds.py uses it), on
both storage paths, with info and weight NULL and non-NULL.  A stack of three (33, 130) frames: a sparse one, one over
max_cells (counts = 0: none of its slots may change) and one with more plots than capacity (only the first `capacity`
slots are written).  Nothing outside the documented extents is read (the results are those of tight, exactly-sized
arguments, bit for bit) or written: cands / info slots at or beyond min(counts[f], capacity) keep their bytes, as does
everything around the workspace; and the result does not depend on what the workspace held before."""
import numpy as np
import pytest

import guard
import plots_oracle as PO

pytestmark = pytest.mark.gpu

NF, H, W, CAP = 3, 33, 130, 8
EXT = [250.0, 300.0]
SENTINEL64 = 0x7FF80000DEADBEEF


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(path):
    rng = np.random.default_rng(17)
    stat = rng.random((NF, H, W)).astype(np.float32)
    stat[0] *= 0.5                                         # nothing at the threshold 0.9 but three planted blobs
    stat[0, 4:6, 7:10] = [[1.5, 2.5, 1.25], [1.0, 1.75, 2.0]]
    stat[0, 20, 100] = 3.0
    stat[0, 32, 127:130] = [1.0, 1.5, 1.0]
    if path == "workspace":
        stat[1] += 1.0                                     # every cell detects: 4290 > max_cells
    else:
        stat[1] += 0.3
    weight = (rng.standard_normal((NF, H, W)) + 1j * rng.standard_normal((NF, H, W))).astype(np.complex64)
    return stat, weight


@pytest.mark.parametrize("with_weight", [False, True])
@pytest.mark.parametrize("with_info", [False, True])
@pytest.mark.parametrize("path", ["lds", "workspace"])
def test_guard_bands(gpu_ready, path, with_info, with_weight):
    import torch
    from passiveradar_amd import _lib, engine
    stat, weight = scene(path)
    want = [PO.plots(stat[f], 0.9, EXT, weight[f] if with_weight else None, range_guard=0, doppler_guard=0) for f in range(NF)]
    mc = 4200 if path == "workspace" else max(want[0]["ncells_total"], want[2]["ncells_total"])
    assert want[1]["ncells_total"] > mc >= want[2]["ncells_total"] and want[2]["count"] > CAP > want[0]["count"] > 0
    d = engine.plots_desc(H, W, 0.9, EXT, 8, 0, 0, mc, CAP, with_weight)
    nws = engine.plots_workspace_bytes(d, NF)
    assert nws == (NF * 20 * 8192 if path == "workspace" else 0)
    st = _lib.torch_stream_ptr()
    stored = [min(w["count"], CAP) if f != 1 else 0 for f, w in enumerate(want)]

    def run(args, s):
        # the workspace is scratch, not a result (a frame over max_cells leaves its appends there in arrival order): it gets
        # its own guard bands, and only what lies around it is looked at
        ws = guard.GuardedOutput(1, nws // 8, nws // 8, torch.int64, "cuda") if nws else None
        engine.plots_execute(d, args["stat"], args.get("weight"), NF, args["counts"], args["ncells"], args["cands"],
                             args.get("info"), ws.view if ws else None, st)
        torch.cuda.synchronize()
        if ws:
            outside, unwritten, _ = ws.report()
            assert outside.numel() == 0, f"workspace: {outside.numel()} element(s) outside its {nws} bytes were overwritten"
            assert not bool(unwritten.all())

    def promised(per_slot):
        m = torch.zeros((NF, CAP * per_slot), dtype=torch.bool)
        for f, k in enumerate(stored):
            m[f, :k * per_slot] = True
        return m

    ins = {"stat": guard.In(dev(stat).reshape(1, -1))}
    if with_weight:
        ins["weight"] = guard.In(dev(weight).reshape(1, -1))
    outs = {"counts": guard.Out(1, NF, torch.int32), "ncells": guard.Out(1, NF, torch.int32),
            "cands": guard.Out(NF, CAP * 4, torch.int64, promised=promised(4), finite=False)}
    if with_info:
        outs["info"] = guard.Out(NF, CAP * 6, torch.int64, promised=promised(6), finite=False)
    got = guard.check(run, ins, outs)
    # slots nobody promised keep their bytes, in the guarded and in the tight call
    for res in (got.guarded, got.tight):
        for name, per_slot in (("cands", 4), ("info", 6)):
            if name in res:
                keep = ~promised(per_slot).to(res[name].device)
                assert bool((res[name][keep] == SENTINEL64).all()), name
    # the tight call against the oracle
    assert got.tight["counts"].cpu().numpy().tolist() == [[want[0]["count"], 0, want[2]["count"]]]
    assert got.tight["ncells"].cpu().numpy().tolist() == [[w["ncells_total"] for w in want]]
    cands = got.tight["cands"].cpu().numpy().view(_lib.TRACK_CAND_DTYPE).reshape(NF, CAP)
    for f in (0, 2):
        k = stored[f]
        assert np.array_equal(cands[f]["index"][:k], want[f]["index"][:k])
        assert np.array_equal(cands[f]["strength"][:k], want[f]["strength"][:k])
        assert np.abs(cands[f]["range"][:k] - want[f]["range"][:k]).max() <= 1e-12 * (4200 / 4096) * EXT[1]
    if with_info:
        info = got.tight["info"].cpu().numpy().view(_lib.PLOT_INFO_DTYPE).reshape(NF, CAP)
        for f in (0, 2):
            assert np.array_equal(info[f]["peak"][:stored[f]], want[f]["peak"][:stored[f]])
            assert np.array_equal(info[f]["ncells"][:stored[f]], want[f]["ncells"][:stored[f]])


def test_result_is_independent_of_the_workspace_contents(gpu_ready):
    import torch
    from passiveradar_amd import _lib, engine
    stat, weight = scene("workspace")
    d = engine.plots_desc(H, W, 0.9, EXT, 8, 0, 0, 4290, 64, True)
    nws = engine.plots_workspace_bytes(d, NF)
    assert nws > 0
    x, w = dev(stat), dev(weight)
    res = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for fill in ("zeros", "ones", "random"):
        if fill == "random":
            ws = torch.randint(0, 256, (nws,), dtype=torch.uint8, device="cuda", generator=gen)
        else:
            ws = torch.full((nws,), 0 if fill == "zeros" else 255, dtype=torch.uint8, device="cuda")
        o = (torch.zeros(NF, dtype=torch.int32, device="cuda"), torch.zeros(NF, dtype=torch.int32, device="cuda"),
             torch.zeros(NF * 64 * 32, dtype=torch.uint8, device="cuda"), torch.zeros(NF * 64 * 48, dtype=torch.uint8, device="cuda"))
        engine.plots_execute(d, x, w, NF, o[0], o[1], o[2], o[3], ws, _lib.torch_stream_ptr())
        torch.cuda.synchronize()
        res.append([t.cpu().numpy().tobytes() for t in o])
    assert res[0] == res[1] == res[2]
    assert np.frombuffer(res[0][0], np.int32)[1] == 1          # the all-detecting frame: one plot of 4290 cells
