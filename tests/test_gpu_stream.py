"""The block pipeline of main.py:169-194 on the GPU (batched LS chunks + overlapped CAF frames)
against the golden built from the reference's own functions, plus size-independent properties at
BASELINE sizes."""
import os

import numpy as np
import pytest

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(gpu_ready):
    yield


@pytest.mark.parametrize("batch", [1, 4, 16])
def test_stream_golden(batch):
    import torch
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("stream")
    C, R, F = int(g["C"]), int(g["R"]), int(g["F"])
    sp = StreamProcessor(HipBackend(2 * C, R, F, float(g["fs"]), batch=batch))
    frames = sp.process(g["ref"], g["srv"])
    torch.cuda.synchronize()
    out = StreamProcessor.to_reference_layout(frames).cpu().numpy()
    assert out.shape == g["out"].shape
    assert rel_err(out, g["out"]) < 1e-4
    # the cleaned stream itself (LS stage) against the reference's
    be = sp.backend
    clean = be.clean(be.padded(g["ref"]), be.padded(g["srv"]), 6)[C // 2:C // 2 + 6 * C].cpu().numpy()
    assert rel_err(clean, g["cleaned"]) < 1e-4


def test_sharded_result_equals_unsharded():
    """frames computed rank by rank (world=3, no collective here) == the single-GPU frames"""
    import torch
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("stream")
    C, R, F = int(g["C"]), int(g["R"]), int(g["F"])
    be = HipBackend(2 * C, R, F, float(g["fs"]), batch=4)
    full = StreamProcessor(be).process(g["ref"], g["srv"]).cpu().numpy()
    parts = [StreamProcessor(be, r, 3).process_local(g["ref"], g["srv"])[0].cpu().numpy() for r in range(3)]
    assert rel_err(np.concatenate(parts), full) < 1e-6


def test_cfg2_pipeline_properties():
    """BASELINE config 2 sizes: targets survive the canceller and peak where the scene put them;
    the direct path is gone; two identical halves of a batch give identical frames."""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    n, R, F, fs = 2400000, 256, 512, 2.4e6
    C = n // 2
    ref, srv = scene.make_stream(3, C, fs, R, scene.scene_seed(4))
    be = HipBackend(n, R, F, fs, batch=3)
    fr = StreamProcessor(be).process(ref, srv)
    torch.cuda.synchronize()
    mid = np.abs(fr[1].cpu().numpy())                  # a frame with both neighbours present
    for d, fd, _ in scene.default_targets(R):
        r, c = scene.expected_peak_cell(d, fd, n, fs, R, F)
        win = mid[max(r - 3, 0):r + 4, max(c - 3, 0):c + 4]
        assert np.unravel_index(win.argmax(), win.shape) == (min(r, 3), min(c, 3))
        assert win.max() > 8 * np.median(mid)
    # zero-Doppler clutter ridge (delays 2, 9, 40) is cancelled well below the strongest target
    ridge = mid[F // 2, [R - 2, R - 9, R - 40]]
    tgt = mid[scene.expected_peak_cell(60, 80.0, n, fs, R, F)]
    assert ridge.max() < 0.1 * tgt


def test_raw_to_frames_small_config():
    """front end + LS + CAF from raw int8 recordings against the oracle's restatement of main.py:105-194"""
    import torch
    from oracle import np_oracle as O
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    rng = np.random.default_rng(12)
    cfg = dict(input_chunk_length=2 * 37490, offset_freq=100000, input_sample_rate=2400000,
               resamp_up=13, resamp_dn=119, cpi_samples=8192, num_range_cells=16, num_doppler_cells=32,
               IF_sample_rate=2400000 * 13 / 119)
    nblk = 4
    n_raw = cfg["input_chunk_length"] * nblk
    base = rng.standard_normal(n_raw // 2 + 64) + 1j * rng.standard_normal(n_raw // 2 + 64)
    refc = base[64:]
    srvc = 0.9 * base[62:-2] + 0.2 * base[40:-24] + 0.05 * (rng.standard_normal(n_raw // 2) + 0j)
    def to_raw(z):
        r = np.empty(n_raw, np.int8)
        r[0::2] = np.clip(np.round(z.real * 25), -127, 127)
        r[1::2] = np.clip(np.round(z.imag * 25), -127, 127)
        return r
    raw_ref, raw_srv = to_raw(refc), to_raw(srvc)
    # ceil(37490 complex samples * 13/119) = 4096 IF samples per block = cpi/2
    fe = lambda r: O.front_end(r, cfg["input_chunk_length"], cfg["offset_freq"], cfg["input_sample_rate"], 13, 119)
    ref_if, srv_if = fe(raw_ref), fe(raw_srv)
    assert ref_if.shape[0] == nblk * 4096
    exp = O.process_stream(ref_if.astype(np.complex64), srv_if.astype(np.complex64), cfg["cpi_samples"], 16, 32,
                           cfg["IF_sample_rate"])
    sp = StreamProcessor(HipBackend(cfg["cpi_samples"], 16, 32, cfg["IF_sample_rate"], batch=4))
    got = sp.process_raw(raw_ref, raw_srv, cfg)
    torch.cuda.synchronize()
    got = StreamProcessor.to_reference_layout(got).cpu().numpy()
    assert got.shape == exp.shape
    assert rel_err(got, exp) < 1e-4


def test_pipeline_is_deterministic():
    """no atomics anywhere: two passes over the same resident batch give bit-identical frames, with the
    LS and CAF stages pipelined on two streams or back to back on one"""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend
    C, R, F, fs = 65536, 32, 64, 262144.0
    ref, srv = scene.make_stream(8, C, fs, R, 4711)
    outs = []
    for overlap in (True, False, True):
        be = HipBackend(2 * C, R, F, fs, batch=8, overlap=overlap)
        be.overlap = overlap and True          # force the two-stream path even for this small batch
        if overlap:
            be.sub = 4
            be.nls = 2                                     # two LS chains in flight on two streams
            be.s_ls_all = [torch.cuda.Stream(), torch.cuda.Stream()]
            be.s_caf = torch.cuda.Stream()
            be.ls_plans = [be.engine.LsPlan(C, R, 10, False, 4) for _ in range(2)]
            be.ls = be.ls_plans[0]
        rp, sp_ = be.padded(ref), be.padded(srv)
        outs.append(be.run(rp, sp_, 8, 0, 8).cpu().numpy())
        torch.cuda.synchronize()
    assert np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], outs[1])


def test_cfg2_pipeline_against_reference_output():
    """BASELINE config 2 end to end at full size (3 hop chunks -> LS x5 bins -> the middle overlapped frame)
    against the map the reference itself produced (tests/golden/pipeline_cfg2.npz).

    The reference's LS correlations are float32 sums over 1.2 M samples (scipy.signal.correlate on complex64),
    which leaves ~2e-5 of tap noise; on the cancelled direct-path ridge (zero Doppler +-1 row) that noise
    integrates coherently to 2.3e-4 of the map's peak.  The device path sums in float64 where it matters and agrees
    with a float64 evaluation of the same algorithm to 1e-6, so: <1e-4 everywhere off that ridge, <5e-4 on
    it, <1e-5 against the float64 oracle."""
    import scipy.signal as sg
    import torch
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("pipeline_cfg2")
    n, R, F, fs = int(g["N"]), int(g["R"]), int(g["F"]), float(g["fs"])
    C = n // 2
    a, s = scene.make_stream(3, C, fs, R, int(g["seed"]))
    be = HipBackend(n, R, F, fs, batch=3)
    X = StreamProcessor(be).process(a, s)[int(g["frame_index"])].cpu().numpy()
    ref = g["out"]
    d = np.abs(X - ref) / np.abs(ref).max()
    off_ridge = np.ones(F, bool)
    off_ridge[F // 2 - 1:F // 2 + 2] = False
    assert d[off_ridge].max() < 1e-4
    assert d.max() < 5e-4
    clean = be.clean(be.padded(a), be.padded(s), 3)[C // 2:C // 2 + 3 * C].cpu().numpy()
    assert rel_err(clean[::101], g["cleaned_sub"]) < 1e-4
    # float64 evaluation of the same algorithm
    exact = np.concatenate([O.LS_Filter_Multiple(a[i * C:(i + 1) * C], s[i * C:(i + 1) * C], R, fs, [0, 1, -1, 2, -2])
                            for i in range(3)])
    assert rel_err(clean, exact) < 5e-6
    w = sg.get_window(("kaiser", 5.0), n)
    pad = np.zeros(n // 4)
    Xo = O.fast_xambg_libcalls(np.concatenate((pad, a, pad))[C:C + n].astype(np.complex64),
                               np.concatenate((pad, exact, pad))[C:C + n].astype(np.complex64), R, F, w)[:, :, 0]
    assert rel_err(X, Xo) < 1e-5


def test_cfg2_pipeline_against_complex128_reference_output():
    """BASELINE config 2 end to end at full size against the map the reference produces when its own functions are
    fed complex128 inputs (tests/golden/pipeline_cfg2_c128.npz: scipy.signal.correlate then sums the 1.2 M-term
    correlations in double, clutter_removal.py:142-155).  This is the north-star statement without caveat:
    max|X - X_ref| / max|X_ref| < 1e-4 on EVERY cell, zero-Doppler ridge included; measured ~1e-6."""
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("pipeline_cfg2_c128")
    n, R, F, fs = int(g["N"]), int(g["R"]), int(g["F"]), float(g["fs"])
    C = n // 2
    a, s = scene.make_stream(3, C, fs, R, int(g["seed"]))
    be = HipBackend(n, R, F, fs, batch=3)
    X = StreamProcessor(be).process(a, s)[int(g["frame_index"])].cpu().numpy()
    e = rel_err(X, g["out"])
    print("cfg2 pipeline vs complex128-input reference:", e)
    assert e < 1e-4
    clean = be.clean(be.padded(a), be.padded(s), 3)[C // 2:C // 2 + 3 * C].cpu().numpy()
    assert rel_err(clean[::101], g["cleaned_sub"]) < 1e-5


def test_stream_with_nlms_canceller():
    """HipBackend(clutter='nlms'): every hop chunk is an independent NLMS stream (batched launch), frames from the
    cleaned stream -- against per-chunk NLMS (C twin of the oracle) + the oracle's CAF on the overlapped frames"""
    import torch
    from oracle import c_oracle, np_oracle as O
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    C, R, F, nch, fs = 4096, 20, 32, 7, 2.6e5
    a, b = scene.make_stream(nch, C, fs, R, 424242)
    be = HipBackend(2 * C, R, F, fs, clutter="nlms", batch=4, nlms_mu=0.05)
    got = StreamProcessor(be).process(a, b)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    cleaned = np.concatenate([c_oracle.nlms(a[i * C:(i + 1) * C], b[i * C:(i + 1) * C], R, 0.05, 10)[0] for i in range(nch)])
    from scipy.signal import get_window
    w = get_window(("kaiser", 5.0), 2 * C)
    rf, sf = O.overlap_frames(a, C, C // 2), O.overlap_frames(cleaned, C, C // 2)
    exp = np.stack([O.fast_xambg(x, y, R, F, 2 * C, w)[:, :, 0] for x, y in zip(rf, sf)])
    assert got.shape == exp.shape and rel_err(got, exp) < 1e-4


def test_cfg1_pipeline_against_reference_output():
    """BASELINE config 1 (the reference's own CPU-runnable case) end to end: three 131 072-sample chunks -> LS x5
    bins -> the middle overlapped 256 x 257 frame, against the map the reference itself produced.  At this length
    the reference's float32 correlation noise stays below the 1e-4 bar on every cell."""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("pipeline_cfg1")
    n, R, F, fs = int(g["N"]), int(g["R"]), int(g["F"]), float(g["fs"])
    a, s = scene.make_stream(3, n // 2, fs, R, int(g["seed"]))
    X = StreamProcessor(HipBackend(n, R, F, fs, batch=3)).process(a, s)[int(g["frame_index"])].cpu().numpy()
    assert X.shape == g["out"].shape and rel_err(X, g["out"]) < 1e-4


def test_prc_gather_frames_single_rank():
    """prc_comm_* / prc_gather_frames through the C ABI on one GPU: a world of one (RCCL is loaded, the
    communicator is created, the root's own block is a device copy into its slot); ragged and empty blocks
    are accepted.  The multi-rank pattern (one ncclRecv per peer) is covered on CPU by the gloo tests of the
    same Shard arithmetic."""
    import ctypes
    import torch
    from passiveradar_amd.stream import FrameComm
    comm = FrameComm(0, 1, FrameComm.unique_id())
    F, cols = 16, 9
    blk = torch.randn((5, F, cols), dtype=torch.complex64, device="cuda")
    out = torch.zeros((5, F, cols), dtype=torch.complex64, device="cuda")
    st = torch.cuda.current_stream()
    comm.gather(blk, [5], F * cols, out, 0, ctypes.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, blk)
    # in place: the block already sits in its slot of the receive buffer
    comm.gather(out, [5], F * cols, out, 0, ctypes.c_void_p(st.cuda_stream))
    # an empty block
    comm.gather(None, [0], F * cols, out, 0, ctypes.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, blk)
    comm.close()


def test_prc_comm_loopback_moves_data_through_rccl_on_one_gpu():
    """prc_comm_loopback: the calls prc_gather_frames makes between ranks -- ncclGroupStart, ncclSend, ncclRecv, ncclGroupEnd
    through the run-time binding, float32 counts, one stream -- executed on a one-GPU box with the rank as its own peer: a
    wrong signature, datatype code or count unit in the binding shows here and not on the first multi-GPU run.  Sizes from
    one float to one config-2 map and a non-default stream; a complex64 block travels as float pairs."""
    import torch
    from passiveradar_amd.stream import FrameComm
    comm = FrameComm(0, 1, FrameComm.unique_id())
    assert comm.count() == (1, 0)
    g = torch.Generator(device="cuda").manual_seed(3)
    for shape, dt in (((1,), torch.float32), ((1000, 3), torch.float32), ((3, 512, 257), torch.complex64)):
        src = torch.randn(shape, dtype=torch.float32, device="cuda", generator=g) if dt == torch.float32 else \
            torch.view_as_complex(torch.randn(shape + (2,), dtype=torch.float32, device="cuda", generator=g))
        dst = torch.zeros_like(src)
        comm.loopback(src, dst)
        torch.cuda.synchronize()
        assert torch.equal(src, dst), shape
    st = torch.cuda.Stream()
    src = torch.randn((1 << 20,), device="cuda", generator=g)
    dst = torch.zeros_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        src2 = src * 2.0                                   # produced on the stream the transfer is enqueued on
        comm.loopback(src2, dst, stream=st)
        back = dst + 1.0                                   # consumed on it
    st.synchronize()
    assert torch.equal(back, src * 2.0 + 1.0)
    with pytest.raises(ValueError):
        comm.loopback(src, dst[:10])
    comm.close()


def test_four_illuminator_step_equals_four_single_cafs():
    """BASELINE config 5's structure (q = 4096, R = 2048: the same segment / lag-block shape as the full-size
    2048 x 2048 surface, fewer Doppler rows): four reference channels against ONE surveillance channel over a
    batch of overlapped frames == four separate fast_xambg calls per frame (oracle-checked on one of them)."""
    import torch
    from scipy.signal import get_window
    from passiveradar_amd.range_doppler_processing import fast_xambg
    from passiveradar_amd.stream import HipBackend
    n, R, F, fs, nfr = 1 << 17, 2048, 32, 2.0e7, 3
    C = n // 2
    rng = np.random.default_rng(55)
    refs = [(rng.standard_normal(nfr * C) + 1j * rng.standard_normal(nfr * C)).astype(np.complex64) for _ in range(4)]
    srv = sum(np.roll(r, 100 * (i + 1)) * (0.5 + 0.1 * i) for i, r in enumerate(refs)).astype(np.complex64)
    be = HipBackend(n, R, F, fs, clutter=None, batch=nfr)
    srv_pad = be.padded(srv)
    w = get_window(("kaiser", 5.0), n)
    pad = np.zeros(C // 2, np.complex64)
    sp = np.concatenate((pad, srv, pad))
    for i, r in enumerate(refs):
        got = be.run(be.padded(r), srv_pad, nfr, 0, nfr).cpu().numpy()
        rp = np.concatenate((pad, r, pad))
        for f in range(nfr):
            one = fast_xambg(rp[f * C:f * C + n], sp[f * C:f * C + n], R, F, n, w)[:, :, 0]
            assert rel_err(got[f], one) < 1e-6
        # the echo of illuminator i sits at delay 100 (i+1), zero Doppler
        mid = np.abs(got[1])
        assert np.unravel_index(mid.argmax(), mid.shape) == (F // 2, R - 100 * (i + 1))
    from oracle import np_oracle as O
    exp = O.fast_xambg(rp[C:C + n], sp[C:C + n], R, F, n, w)[:, :, 0]
    assert rel_err(got[1], exp) < 1e-4


@pytest.mark.parametrize("args,frames", [(["--workload", "cfg4", "--frames", "21"], 21),
                                          (["--workload", "cfg5", "--frames", "1"], 1),
                                          (["--frames", "300"], 300)])
def test_bench_workload_modes_run(args, frames):
    """bench.py's workload modes at toy sizes (one GPU): the 600 s-stream mode on a 21-frame stream, the
    four-illuminator mode, the default with a ragged last sub-batch -- one JSON line each with the contract's fields"""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--no-cpu", "--steps", "2", "--warmup", "1"] + args,
                       capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0 and d["unit"] == "frames/s"
    assert d["config"]["frames_per_step_total"] == frames
    assert d["scaling"] == ("strong" if "cfg4" in args else "weak")
    assert d["roofline"]["bound"] in ("hbm", "valu") and 0 < d["roofline"]["frac"] < 1.5
    assert abs(d["value"] - frames * d["steps"] / d["timed_seconds"]) / d["value"] < 1e-6


def test_plain_bench_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full, CPU leg not switched off) times exactly --steps steps and measures nothing else; its
    --dump-outputs sample of the last step's maps (float32 values, float64 flat indices, under 64 MB) holds the same
    cells as the maps --dump writes of that step"""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out, dump = tmp_path / "outputs", str(tmp_path / "cfg2.npz")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--steps", "3", "--warmup", "1", "--frames", "300",
                        "--dump-outputs", str(out), "--dump", dump], capture_output=True, text=True, timeout=600, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 3 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] - d["timed_seconds"] / 3 * 1e3) < 1e-9 * d["ms_per_step"]
    assert not [k for k in ("roofline", "kernels", "cpu_baseline", "secondary") if k in d], d.keys()
    files = sorted(os.listdir(out))
    assert files == ["maps.npy", "sample_index.npy"] and sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    vals, idx = np.load(out / "maps.npy"), np.load(out / "sample_index.npy").astype(np.int64)
    assert vals.dtype == np.float32 and vals.shape == (1, idx.size, 2) and np.all(np.diff(idx) > 0)
    g = np.load(dump)
    cells = g["ill0_frames"][0].size
    assert idx[-1] < 300 * cells
    for j, f in enumerate(g["frame_index"]):
        sel = idx // cells == f
        assert sel.any()
        got = vals[0, sel, 0] + 1j * vals[0, sel, 1]
        assert np.array_equal(got, g["ill0_frames"][j].reshape(-1)[idx[sel] - f * cells]), int(f)


def test_bench_cfg4_maps_against_an_independent_pass(tmp_path):
    """what bench.py --workload cfg4 computes IS the stream pipeline: its maps (dumped from the last timed step of a
    21-frame stream at full config-2 frame size) equal an independent pass over the regenerated stream -- other
    sub-batch size, LS and CAF back to back on one stream -- and one frame equals the CPU oracle end to end"""
    import subprocess
    import sys
    import torch
    from scipy.signal import get_window
    from oracle import np_oracle as O
    from passiveradar_amd.stream import HipBackend
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    import bench
    dump = str(tmp_path / "cfg4.npz")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--no-cpu", "--steps", "2", "--warmup", "1",
                        "--workload", "cfg4", "--frames", "21", "--dump", dump],
                       capture_output=True, text=True, timeout=900, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(dump)
    fs, n, R, F, _, _ = bench.WORKLOADS["cfg4"]
    C, nfr = n // 2, int(d["nframes"])
    assert nfr == 21
    # the stream as bench.py builds it in strong-scaling mode: 64-chunk segments keyed by the global chunk index
    a, s_ = bench.synth_segment(torch, 64, C, fs, R, int(d["seed0"]) * 1000003 + 0, torch.device("cuda", 0), t0=0.0)
    ref, srv = a[:nfr * C], s_[:nfr * C]
    be = HipBackend(n, R, F, fs, batch=5, overlap=False)
    maps = be.run(be.padded(ref), be.padded(srv), nfr, 0, nfr)
    torch.cuda.synchronize()
    got = d["ill0_frames"]
    for j, fi in enumerate(d["frame_index"]):
        assert rel_err(got[j], maps[int(fi)].cpu().numpy()) < 1e-6, int(fi)
    assert rel_err(d["ill0_sums"], maps.sum(dim=(1, 2)).cpu().numpy()) < 1e-5
    # one frame end to end on the CPU: LS_Filter_Multiple on its three chunks, overlapped CPI, fast_xambg
    fi = 1
    rh, sh = ref[:3 * C].cpu().numpy(), srv[:3 * C].cpu().numpy()
    clean = np.concatenate([O.LS_Filter_Multiple(rh[i * C:(i + 1) * C], sh[i * C:(i + 1) * C], R, fs, [0, 1, -1, 2, -2])
                            for i in range(3)]).astype(np.complex64)
    pad = np.zeros(C // 2, np.complex64)
    rp, cp = np.concatenate((pad, rh, pad)), np.concatenate((pad, clean, pad))
    exp = O.fast_xambg(rp[fi * C:fi * C + n], cp[fi * C:fi * C + n], R, F, n, get_window(("kaiser", 5.0), n))[:, :, 0]
    assert rel_err(got[list(d["frame_index"]).index(fi)], exp) < 1e-4


@pytest.mark.parametrize("gather", ["none", "prc"])
def test_bench_default_workload_maps_against_an_independent_pass(tmp_path, gather):
    """The HEADLINE path itself: bench.py's default workload at 600 frames -- three sub-batches of 256 (the
    last one ragged) alternating over the three LS plans / streams, the CAF on a fourth -- dumps the first, second, middle
    and last map and every frame's sum of its last timed step; an independent pass over the regenerated stream (batches of
    five, LS and CAF back to back on one stream, one plan) must give the same maps.  gather = "prc": the same step with the
    N > 1 gather plumbing switched on through a communicator of ONE rank -- CAF launches cut at the sub-batch boundaries,
    every block handed to prc_gather_frames on the communication stream behind its launch's event, four receive buffers in
    turn -- which must not change a map (the multi-rank transfers themselves need more than one GPU)"""
    import subprocess
    import sys
    import torch
    from passiveradar_amd.stream import HipBackend
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    import bench
    dump = str(tmp_path / "cfg2.npz")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--no-cpu", "--steps", "2", "--warmup", "1",
                        "--frames", "600", "--dump", dump, "--gather", gather], capture_output=True, text=True, timeout=900,
                       cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(dump)
    fs, n, R, F, _, _ = bench.WORKLOADS["cfg2"]
    C, nfr = n // 2, int(d["nframes"])
    assert nfr == 600 and list(d["frame_index"]) == [0, 1, 300, 599]
    dev = torch.device("cuda", 0)
    ref_pad, srv_pad = bench.synth_padded(torch, nfr, C, fs, R, int(d["seed0"]), dev)     # the stream as bench.py builds it
    be = HipBackend(n, R, F, fs, batch=5, overlap=False)
    maps = be.run(ref_pad, srv_pad, nfr, 0, nfr)
    torch.cuda.synchronize()
    got = d["ill0_frames"]
    # not bit-equal by construction: a plan of 258 blocks cuts a chunk into 9 teams of ~35 pieces, a plan of 7 blocks into
    # 78 teams of 4, so the float32 partial sums of the correlations group differently (measured: 1.0e-6 on frame 300)
    for j, fi in enumerate(d["frame_index"]):
        assert rel_err(got[j], maps[int(fi)].cpu().numpy()) < 5e-6, int(fi)
    # every frame's sum (a coarse check that each of the 600 maps came from the right chunks): 131 584 cells whose 1e-6
    # differences add incoherently while the sum itself mostly cancels -- measured 1.2e-5 of the largest sum
    assert rel_err(d["ill0_sums"], maps.sum(dim=(1, 2)).cpu().numpy()) < 1e-4
    if gather == "prc":
        # the block the last prc_gather_frames call of the step delivered into its receive buffer IS those frames
        f0, blk = int(d["gathered_first_frame"]), d["gathered_block"]
        assert f0 + blk.shape[0] == nfr and int(d["gathers_per_step"]) >= 3
        assert rel_err(blk, maps[f0:f0 + blk.shape[0]].cpu().numpy()) < 5e-6


def test_stream_with_the_ls_filter_variant():
    """SURVEY 8's config-2 "LS_Filter variant": the stream backend with clutter="ls_direct" runs LS_Filter
    (clutter_removal.py:6-56: circular data matrix, reg = 1 on the Gram diagonal) per hop chunk, then the overlapped
    CAF -- equal to the drop-in called chunk by chunk and to the oracle end to end"""
    from oracle import np_oracle as O
    from passiveradar_amd import scene
    from passiveradar_amd.clutter_removal import LS_Filter
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    C, R, F, fs, nch = 16384, 24, 64, 1.0e5, 5
    ref, srv = scene.make_stream(nch, C, fs, R, 777)
    be = HipBackend(2 * C, R, F, fs, clutter="ls_direct", batch=4)
    got = StreamProcessor(be).process(ref, srv).cpu().numpy()
    clean = np.concatenate([LS_Filter(ref[i * C:(i + 1) * C], srv[i * C:(i + 1) * C], R) for i in range(nch)])
    exp_clean = np.concatenate([O.LS_Filter(ref[i * C:(i + 1) * C], srv[i * C:(i + 1) * C], R) for i in range(nch)])
    assert rel_err(clean, exp_clean) < 1e-4
    pad = np.zeros(C // 2, np.complex64)
    rp, cp = np.concatenate((pad, ref, pad)), np.concatenate((pad, exp_clean.astype(np.complex64), pad))
    w = np.kaiser(2 * C, 5.0)
    for f in (0, 2, nch - 1):
        exp = O.fast_xambg(rp[f * C:f * C + 2 * C], cp[f * C:f * C + 2 * C], R, F, 2 * C, w)[:, :, 0]
        assert rel_err(got[f], exp) < 1e-4, f
    with pytest.raises(ValueError):
        HipBackend(2 * C, R, F, fs, clutter="svd")


def test_bench_cfg5_maps_against_single_calls(tmp_path):
    """bench.py --workload cfg5 (four illuminators against one surveillance channel, full 2048 x 2048 size, one frame):
    the dumped surfaces equal one fast_xambg call per (reference, surveillance) pair on the regenerated channels --
    range_doppler_processing.py:12-90 once per pair, which is what a multi-illuminator frame means"""
    import subprocess
    import sys
    import torch
    from passiveradar_amd.range_doppler_processing import fast_xambg
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    import bench
    dump = str(tmp_path / "cfg5.npz")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--no-cpu", "--steps", "2", "--warmup", "1",
                        "--workload", "cfg5", "--frames", "1", "--dump", dump],
                       capture_output=True, text=True, timeout=900, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = np.load(dump)
    fs, n, R, F, _, _ = bench.WORKLOADS["cfg5"]
    C = n // 2
    dev = torch.device("cuda", 0)
    srv_pad, refs = None, []
    for i in range(4):                                   # as bench.py builds them (rank 0, frame group 0)
        r_i, srv_pad = bench.synth_padded(torch, 1, C, fs, R, 777 + 13 * i, dev, add_to=srv_pad)
        refs.append(r_i)
    win = torch.from_numpy(np.kaiser(n, 5.0).astype(np.float32)).to(dev)
    from scipy.signal import get_window
    win = torch.from_numpy(get_window(("kaiser", 5.0), n).astype(np.float32)).to(dev)
    for i in range(4):
        one = fast_xambg(refs[i][:n], srv_pad[:n], R, F, n, win)[:, :, 0].cpu().numpy()
        assert rel_err(d[f"ill{i}_frames"][0], one) < 1e-6, i


def test_prconfig_raw_to_frame_against_reference_output():
    """The reference's published workload end to end at the shipped sizes (PRconfig.yaml unmodified): three raw int8
    blocks of 4 799 250 scalars per channel -> device front end (deinterleave, tune with block phases, 13:119) ->
    LS_Filter_Multiple x 5 bins (T = 185) on 262 144-sample chunks -> the middle overlapped 1024 x 176 frame
    (main.py:105-194), against what the reference's own functions produced (golden pipeline_prconfig_raw, made by
    oracle/gen_golden.py pipeline_prconfig_raw_case): IF streams, cleaned stream and the map, each within 1e-4."""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("pipeline_prconfig_raw")
    cfg = {k[4:]: (float(g[k]) if k == "cfg_IF_sample_rate" else int(g[k])) for k in g if k.startswith("cfg_")}
    raw_ref, raw_srv = scene.make_raw_stream(int(g["nblk"]), cfg["input_chunk_length"], cfg["input_sample_rate"],
                                             cfg["offset_freq"], int(g["seed"]))
    if (list(scene.raw_checksum(raw_ref)) != [int(v) for v in g["raw_ref_checksum"]] or
            list(scene.raw_checksum(raw_srv)) != [int(v) for v in g["raw_srv_checksum"]]):
        pytest.skip("the regenerated raw stream differs from the golden's (another libm / NumPy build)")
    be = HipBackend(cfg["cpi_samples"], cfg["num_range_cells"], cfg["num_doppler_cells"], cfg["IF_sample_rate"], batch=3)
    args = (cfg["input_chunk_length"], cfg["offset_freq"], cfg["input_sample_rate"], cfg["resamp_up"], cfg["resamp_dn"])
    a, s = be.front_end(raw_ref, *args), be.front_end(raw_srv, *args)
    assert a.shape[0] == int(g["nblk"]) * cfg["output_chunk_length"]
    assert rel_err(a[::61].cpu().numpy(), g["if_ref_sub"]) < 1e-4 and rel_err(s[::61].cpu().numpy(), g["if_srv_sub"]) < 1e-4
    sp = StreamProcessor(be)
    frames = sp.process_raw(raw_ref, raw_srv, cfg)
    torch.cuda.synchronize()
    X = frames[int(g["frame_index"])].cpu().numpy()
    assert X.shape == g["out"].shape and rel_err(X, g["out"]) < 1e-4
    # the cleaned stream the frames were made of (clutter 40 dB down: normalised by the level of what went in)
    ref_pad, srv_pad = be.padded(a), be.padded(s)
    clean = be.clean(ref_pad, srv_pad, int(g["nblk"]))
    C = cfg["output_chunk_length"]
    got = clean[C // 2:C // 2 + int(g["nblk"]) * C][::61].cpu().numpy()
    assert np.abs(got - g["cleaned_sub"]).max() / float(g["if_srv_rms"]) < 1e-4


@pytest.mark.gpu
def test_front_end_in_pieces_continues_the_block_phases():
    """front_end(block0=, out=): a recording converted piece by piece (bench.py --workload prconfig overlaps the host
    link with the device this way) is the recording converted in one call, bit for bit -- the per-block phase of
    main.py:125-131 is a function of the block's index in the recording, not in the call."""
    import json
    import torch
    from passiveradar_amd import scene, stream as prstream
    cfg = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "config_prconfig.json")))
    icl = 2 * 4096 * 3
    rr, _ = scene.make_raw_stream(7, icl, cfg["input_sample_rate"], cfg["offset_freq"], scene.scene_seed(5))
    be = prstream.HipBackend(4096, 16, 32, cfg["IF_sample_rate"], batch=8, device=torch.device("cuda", 0), clutter=None)
    args = (icl, cfg["offset_freq"], cfg["input_sample_rate"], cfg["resamp_up"], cfg["resamp_dn"])
    whole = be.front_end(rr, *args, max_blocks=4)
    n_out = whole.shape[0] // 7
    out = torch.zeros(7 * n_out + 10, dtype=torch.complex64, device="cuda")
    for b0, m in ((0, 3), (3, 1), (4, 3)):
        got = be.front_end(rr[b0 * icl:(b0 + m) * icl], *args, max_blocks=4, block0=b0, out=out[5 + b0 * n_out:5 + (b0 + m) * n_out])
        assert got.data_ptr() == out[5 + b0 * n_out:].data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(out[5:5 + 7 * n_out], whole)
    assert float(out[:5].abs().max()) == 0.0 and float(out[-5:].abs().max()) == 0.0


@pytest.mark.parametrize("nframes,batch", [(7, 4), (8, 8), (3, 2)])
def test_multi_illuminator_frames_in_two_lanes(nframes, batch):
    """HipBackend(caf_lanes=2).frames_multi: alternate half-batches of frames on two plans / two streams (so that one
    piece's Doppler launch runs under the next piece's segment launch, bench.py --workload cfg5) give the maps of the
    one-plan path bit for bit, joined to the calling stream or not, call after call into the same buffers"""
    import torch
    from passiveradar_amd import scene
    from passiveradar_amd.stream import HipBackend
    C, R, F, fs, nref = 16384, 600, 256, 1.0e6, 3
    refs, srv = scene.make_multi_scene((nframes + 1) * C, fs, 200, [11, 12, 13])
    one = HipBackend(2 * C, R, F, fs, clutter=None, batch=batch, nref=nref)
    two = HipBackend(2 * C, R, F, fs, clutter=None, batch=batch, nref=nref, caf_lanes=2)
    assert two.caf_lanes == 2 and one.caf_lanes == 1
    rp = [one.padded(r) for r in refs]
    sp = one.padded(srv)
    want = one.frames_multi(rp, sp, 0, nframes)
    got = two.frames_multi(rp, sp, 0, nframes)
    torch.cuda.synchronize()
    for w, g in zip(want, got):
        assert torch.equal(w, g)
    outs = [torch.zeros_like(w) for w in want]
    for _ in range(3):                                  # a resident pipeline: no join between the calls
        two.frames_multi(rp, sp, 0, nframes, outs, join=False)
    torch.cuda.synchronize()
    for w, g in zip(want, outs):
        assert torch.equal(w, g)


def test_bench_measures_its_own_traffic(tmp_path):
    """roofline.traffic used to be a constant from a file.  bench.py --traffic measure runs itself twice under
    `rocprofv3 --pmc` (FETCH_SIZE, then WRITE_SIZE: separate passes, counters only) on one launch's worth of frames and
    reports 2 x FETCH + WRITE of the dominant kernel -- the line says so, and the figure is the fused LS pass's 28-30 MB per
    chunk-bin (a --full line takes this path whenever its CPU leg runs: `--traffic auto`)."""
    import json
    import shutil
    import subprocess
    import sys
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 is not on PATH")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--no-cpu", "--steps", "2", "--warmup", "1", "--frames", "300",
                        "--traffic", "measure"], capture_output=True, text=True, timeout=900, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    roof = d["roofline"]
    assert roof["kernel"] == "ls_fir_subtract" and roof["traffic_source"]["how"].startswith("measured by this run"), roof
    per_chunk_bin = roof["traffic"] / 256.0            # an LS launch of the 300-frame step covers 256 hop chunks
    assert 26e6 < per_chunk_bin < 32e6, per_chunk_bin
    # `frac` is the rate on the bytes MOVED; SURVEY 8d's two-pass accounting credits the fused kernel with
    # bytes it never moves and is reported under its own name
    assert abs(roof["frac"] - roof["traffic"] / (roof["solo_ms_per_launch"] * 1e-3) / 8e12) < 1e-9
    assert 0.3 < roof["frac"] < roof["frac_two_pass_accounting"] < 1.2
    assert roof["frac_of_copy_ceiling"] < 1.0
    # every family's launch was counted, and the whole step's bytes per frame are the sum the kernels{} table implies
    k = d["kernels"]
    assert all(k[f]["moved_bytes_per_launch"] for f in ("caf_segments", "caf_doppler", "ls_correlate", "ls_fir_subtract"))
    assert 180e6 < d["hbm_moved_bytes_per_frame"] < 230e6, d["hbm_moved_bytes_per_frame"]
    assert d["hbm_frac_of_copy_ceiling"] < 1.0 < d["hbm_two_pass_accounting"]["bytes_per_frame"] / d["hbm_moved_bytes_per_frame"]


def test_bench_reports_in_step_kernel_durations():
    """the kernels{} table held solo times whose sum exceeds the step.  `--in-step measure` adds every
    kernel's duration inside the overlapped step (one rocprofv3 --kernel-trace child pass) and the mean concurrency."""
    import json
    import shutil
    import subprocess
    import sys
    if shutil.which("rocprofv3") is None:
        pytest.skip("rocprofv3 is not on PATH")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--no-cpu", "--steps", "2", "--warmup", "1", "--frames", "1024",
                        "--traffic", "file", "--in-step", "measure"], capture_output=True, text=True, timeout=900, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    acc = d["kernel_time_accounting"]
    assert acc["child_frames_per_step"] == 1024 and acc["in_step_mean_concurrency"] > 1.0, acc
    fused = d["kernels"]["ls_fir_subtract"]
    assert fused["in_step_ms_per_launch"] > fused["avg_ms_per_launch"] * 0.95, fused   # sharing the chip never makes it faster
    assert d["roofline"]["frac_in_step"] <= d["roofline"]["frac"] * 1.05


def test_bench_gpus_n_starts_n_ranks():
    """`python bench.py --gpus N` without a launcher used to benchmark ONE GPU and print n_gpus 1.  It now
    starts the N ranks itself (torch.distributed.run on 127.0.0.1) -- and the line says how many RCCL saw."""
    import json
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--frames", "512"],
                       capture_output=True, text=True, timeout=1500, cwd=repo, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["rccl_nranks"] == 2 and len(d["rank_ms_per_step"]) == 2, d


def test_device_maps_through_the_output_stores(tmp_path):
    """SURVEY 8 row f4 (main.py:200-224), device side: the maps of a small stream computed on the GPU go through BOTH
    stores -- the zarr v2 directory store (frame by frame through ZarrFrameWriter, in two blocks out of order, as the
    pipelined host-to-host step writes them) and the HDF5 dataset '/xambg' -- and come back, through the spec-driven zarr
    reader and libhdf5, as the (F, R+1, nframes) array of the reference: equal to the device maps moved to axis 2, bit for
    bit, and to the reference's own output of the same stream (golden `stream`) within the parity bar.  The .npz axes
    follow main.py:200-206's formulas.  (No zarr / h5py consumer exists in this image: README, "Output stores".)"""
    import json
    import torch
    from passiveradar_amd import output
    from passiveradar_amd.stream import HipBackend, StreamProcessor
    g = load_golden("stream")
    C, R, F, fs = int(g["C"]), int(g["R"]), int(g["F"]), float(g["fs"])
    sp = StreamProcessor(HipBackend(2 * C, R, F, fs, batch=4))
    frames = sp.process(g["ref"], g["srv"])                       # device tensor [nframes][F][R+1]
    assert frames.is_cuda and frames.dtype == torch.complex64
    nframes = int(frames.shape[0])
    want = np.ascontiguousarray(StreamProcessor.to_reference_layout(frames).cpu().numpy())
    assert want.shape == (F, R + 1, nframes) == g["out"].shape
    cfg = dict(num_doppler_cells=F, num_range_cells=R, frame_interval=C / fs, range_cell_width=299792458.0 / fs / 1000.0,
               doppler_cell_width=fs / (2 * C), range_doppler_map_ftype="zarr",
               range_doppler_map_fname=str(tmp_path / "XAMBG.zarr"), meta_fname=str(tmp_path / "XAMBG.npz"))
    # zarr, as bench.py --workload prconfig stores: blocks of frames as they leave the device, here the second block first
    zw = output.ZarrFrameWriter(cfg["range_doppler_map_fname"], F, R + 1, nframes)
    cut = nframes // 2
    host = torch.empty((nframes, F, R + 1), dtype=torch.complex64).pin_memory()
    host[cut:].copy_(frames[cut:], non_blocking=True)
    host[:cut].copy_(frames[:cut], non_blocking=True)
    torch.cuda.synchronize()
    zw.write(cut, host.numpy()[cut:])
    zw.write(0, host.numpy()[:cut])
    back = output.read_zarr_v2(cfg["range_doppler_map_fname"])
    assert back.dtype == np.complex64 and np.array_equal(back, want)
    assert rel_err(back, g["out"]) < 1e-4                          # what the reference itself stored for this stream
    # the one-call form takes the device tensor directly
    p2 = output.save_range_doppler(dict(cfg, range_doppler_map_fname=str(tmp_path / "again.zarr")), frames)
    assert np.array_equal(output.load_range_doppler_zarr(p2), want)
    meta = json.load(open(os.path.join(p2, ".zarray")))
    assert meta["shape"] == [F, R + 1, nframes] and meta["chunks"] == [F, R + 1, 1] and meta["dtype"] == "<c8"
    # HDF5 through the HDF5 C library
    if output.hdf5_available():
        ph = output.save_range_doppler(dict(cfg, range_doppler_map_ftype="hdf5", range_doppler_map_fname=str(tmp_path / "XAMBG.hdf5")),
                                       frames.cpu().numpy())
        got = output.load_range_doppler_hdf5(ph)
        assert got.dtype == np.complex64 and np.array_equal(got, want)
    # the .npz axes: main.py:200-206
    m = np.load(output.save_metadata(cfg, nframes))
    assert np.array_equal(m["frame_timestamps"], np.arange(nframes) * cfg["frame_interval"])
    assert np.array_equal(m["range_bins"], np.arange(R + 1) * cfg["range_cell_width"])
    assert np.array_equal(m["doppler_bins"], np.arange(-F, F) * cfg["doppler_cell_width"])


def test_front_end_phases_may_die_when_the_call_returns():
    """Round 6 (found by tests/fuzz_parity.py under eight caller threads: a block tuned with another call's phases):
    prc_frontend_execute's `phases_host` is a HOST array the caller may free the moment the call returns -- the ctypes
    array of engine.FrontendPlan.execute is such a temporary -- while the stream may reach the copy much later.  Here
    the stream is kept busy (a long sleep kernel queued first), the call is made through the C ABI with phases in a buffer
    that is overwritten right after it returns, and the blocks must come out tuned with the phases that were passed
    (main.py:125-149).  The phases now ride inside the kernel arguments (up to 32 blocks per launch) or, for longer
    launches, inside the arguments of small kernels that fill the plan's device array -- both forms are run here (4 and
    70 blocks per launch).  (Single-threaded the HIP runtime stages a small pageable copy at enqueue, so this contract
    test also passes on the old direct copy -- measured; the load that made it fail is in
    tests/test_gpu_zz_fuzz.py::test_fuzz_two_channel_front_end_eight_threads.)"""
    import ctypes as C
    import torch
    from passiveradar_amd import _lib, engine
    from passiveradar_amd import scene
    for n_in, nb in ((6000, 4), (1500, 70)):
        _phases_case(C, torch, _lib, engine, scene, n_in, nb)


def _phases_case(C, torch, _lib, engine, scene, n_in, nb):
    up, dn = 13, 119
    raw = scene.make_raw_stream(nb, 2 * n_in, 2400000, 100000, scene.scene_seed(77))[0]
    raw_d = torch.from_numpy(raw).cuda()
    plan = engine.FrontendPlan(n_in, "int8", up, dn, nb)
    lib, s = _lib.lib(), _lib.torch_stream_ptr()
    good = [0.3 + 1.7 * b for b in range(nb)]

    def run(phases_buf, out):
        _lib.check(lib.prc_frontend_execute(plan._h, raw_d.data_ptr(), 2 * n_in, 1, 100000.0, 2400000.0, phases_buf, out.data_ptr(),
                                            plan.n_out, nb, s))
    want = torch.empty(nb * plan.n_out, dtype=torch.complex64, device="cuda")
    keep = (C.c_double * nb)(*good)
    run(keep, want)
    torch.cuda.synchronize()
    # the blocks really are tuned per block: with all phases equal to the first one the other blocks differ
    flat = torch.empty_like(want)
    run((C.c_double * nb)(*([good[0]] * nb)), flat)
    torch.cuda.synchronize()
    assert torch.equal(flat[:plan.n_out], want[:plan.n_out]) and not torch.equal(flat[plan.n_out:], want[plan.n_out:])
    for rounds in range(3):
        got = torch.zeros_like(want)
        torch.cuda._sleep(400_000_000)                       # ~0.2 s of stream time before the launch can run
        buf = (C.c_double * nb)(*good)
        run(buf, got)
        for b in range(nb):
            buf[b] = 1e9 + b                                   # the caller's memory is reused at once
        torch.cuda.synchronize()
        assert torch.equal(got, want), rounds


def _bench_two_ranks_one_gpu(tmp_path, extra, name):
    import json
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dump = str(tmp_path / f"{name}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(repo, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--share-gpu",
           "--no-cpu", "--steps", "2", "--warmup", "1", "--dump", dump] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=repo, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and len(line["rank_ms_per_step"]) == 2 and line["gather_path"] == "torch", line
    assert "not a number of record" in line["rehearsal"] and line["rccl_nranks"] is None
    assert all(b > 0 for b in line["gathered_bytes_per_rank_per_step"])
    return line, np.load(dump)


def test_bench_two_ranks_rehearsal_strong_scaling_equals_one_rank(tmp_path):
    """The multi-rank control flow of bench.py has never run on hardware (one GPU per box).  REHEARSAL: two ranks share the
    one GPU over gloo (`--dist-backend gloo --share-gpu`; RCCL refuses two ranks on one device, so the gather takes the
    torch path with the maps staged through the host): config 4's stream sharded over the two ranks -- contiguous frame
    ranges, one halo chunk re-filtered locally, four part gathers per pass overlapped with compute -- must assemble on rank 0
    into the maps one rank computes alone (main.py:169-194, 213-224): every frame's sum and four picked maps."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames = 301
    line, two = _bench_two_ranks_one_gpu(tmp_path, ["--workload", "cfg4", "--frames", str(frames)], "two")
    assert line["scaling"] == "strong" and line["config"]["frames_per_step_total"] == frames
    one_dump = str(tmp_path / "one.npz")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--workload", "cfg4", "--frames", str(frames), "--no-cpu",
                        "--steps", "2", "--warmup", "1", "--dump", one_dump], capture_output=True, text=True, timeout=1500, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    one = np.load(one_dump)
    assert list(two["frame_index"]) == list(one["frame_index"]) and int(two["nframes"]) == frames
    scale = np.abs(one["ill0_frames"]).max()
    assert np.abs(two["ill0_frames"] - one["ill0_frames"]).max() < 5e-6 * scale      # other LS plan sizes: float32 sums group differently
    assert rel_err(two["ill0_sums"], one["ill0_sums"]) < 1e-4


def test_bench_two_ranks_rehearsal_weak_scaling_gathers_every_sub_batch(tmp_path):
    """the default workload's N > 1 form: every rank its own frames, one gather per sub-batch issued behind the launch that
    completes it; the last gathered block on rank 0 is [rank 0's frames | rank 1's frames] of that sub-batch"""
    line, d = _bench_two_ranks_one_gpu(tmp_path, ["--frames", "600"], "weak")
    assert line["scaling"] == "weak" and line["config"]["frames_per_step_total"] == 1200
    m = int(d["m"])
    blk = d["gathered_block"]
    assert blk.shape[0] == 2 * m and m == 600 - 512                      # the ragged last sub-batch of 600 = 256 + 256 + 88
    assert np.array_equal(blk[:m], d["own_frames"])                       # rank 0's block landed first, bit for bit
    assert np.abs(blk[m:]).max() > 0 and not np.array_equal(blk[m:], blk[:m])   # rank 1's frames (another stream) behind it
