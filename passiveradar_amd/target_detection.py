"""Drop-ins for the reference's ``passiveRadar/target_detection.py``: ``CFAR_2D`` (:683-703), applied per frame to
``|xambg|`` by range_doppler_plot.py:56-57 (SURVEY 8f "next" #3), the multi-target Kalman tracker of
multitarget_kalman_tracker.py: ``get_measurements`` (:164-229) and ``multitarget_tracker`` (:455-537), plus
``track_maps``, that script's CFAR -> measure -> track chain (:44-63) in one device pass, and the single-target tracker
of simple_kalman_tracker.py: ``simple_target_tracker`` (:626-681), plus ``simple_track_maps``, its CFAR -> track
chain (:46-61).  Beyond the reference: ``CFAR_2D_OS``, the order-statistic CFAR on CFAR_2D's window (with
``cfar_training_cells`` and ``os_cfar_threshold``), which the chains take with ``cfar="os"``, and ``refine_peaks``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, engine
from ._lib import check, lib

__all__ = ["CFAR_2D", "CFAR_2D_abs", "CFAR_2D_OS", "cfar_training_cells", "os_cfar_threshold", "get_measurements",
           "multitarget_tracker", "track_maps",
           "kalman_filter_dtype", "target_track_dtype", "simple_target_tracker", "simple_track_maps",
           "target_track_dtype_simple", "refine_peaks"]


def CFAR_2D(X, fw, gw, thresh=None):
    """Constant false alarm rate filter (same contract as target_detection.py:683-703): X is a 2-D
    (Doppler x range) magnitude map -- or a stack [nframes, H, W] / torch device tensor for batches;
    returns the CFAR ratio in float64 (boolean if ``thresh`` is given), like the reference."""
    if _lib.is_device_tensor(X):
        import torch
        x = X.to(torch.float32).contiguous()
        frames = 1 if x.dim() == 2 else x.shape[0]
        H, W = x.shape[-2], x.shape[-1]
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):          # launch on the tensor's device and torch's stream there
            check(lib().prc_cfar2d(x.data_ptr(), H, W, int(fw), int(gw), int(thresh is not None),
                                   float(thresh or 0.0), out.data_ptr(), frames, _lib.torch_stream_ptr(x.device)))
        return out.bool() if thresh is not None else out
    x = np.ascontiguousarray(X, dtype=np.float32)
    frames = 1 if x.ndim == 2 else x.shape[0]
    H, W = x.shape[-2], x.shape[-1]
    st = engine.staging()
    dx = st.get("cfar_x", x.nbytes)
    do = st.get("cfar_o", x.nbytes)
    dx.upload(x)
    check(lib().prc_cfar2d(dx.ptr, H, W, int(fw), int(gw), int(thresh is not None), float(thresh or 0.0),
                           do.ptr, frames, None))
    out = do.download(x.shape, np.float32)
    return out > 0.5 if thresh is not None else out.astype(np.float64)


def CFAR_2D_abs(xambg, fw, gw, thresh=None):
    """``CFAR_2D(np.abs(xambg), fw, gw, thresh)`` -- the call of range_doppler_plot.py:56-57 -- in ONE kernel: the
    complex64 range-Doppler map (2-D, a stack [nframes, H, W], or torch device tensors of those shapes) goes in as it
    is and |X| is taken while the CFAR tiles are loaded, so the complex map is read once and no magnitude map is written.  Same return convention as
    CFAR_2D."""
    if _lib.is_device_tensor(xambg):
        import torch
        x = xambg.to(torch.complex64).contiguous()
        if x.dim() not in (2, 3):
            raise ValueError("CFAR_2D_abs takes a 2-D map or a stack [nframes, H, W]")
        frames = 1 if x.dim() == 2 else x.shape[0]
        H, W = x.shape[-2], x.shape[-1]
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib().prc_cfar2d_c64(x.data_ptr(), H, W, int(fw), int(gw), int(thresh is not None),
                                       float(thresh or 0.0), out.data_ptr(), frames, _lib.torch_stream_ptr(x.device)))
        return out.bool() if thresh is not None else out
    x = np.ascontiguousarray(xambg, dtype=np.complex64)
    if x.ndim not in (2, 3):
        raise ValueError("CFAR_2D_abs takes a 2-D map or a stack [nframes, H, W]")
    frames = 1 if x.ndim == 2 else x.shape[0]
    H, W = x.shape[-2], x.shape[-1]
    st = engine.staging()
    dx = st.get("cfar_xc", x.nbytes)
    do = st.get("cfar_o", x.nbytes // 2)
    dx.upload(x)
    check(lib().prc_cfar2d_c64(dx.ptr, H, W, int(fw), int(gw), int(thresh is not None), float(thresh or 0.0),
                               do.ptr, frames, None))
    out = do.download(x.shape, np.float32)
    return out > 0.5 if thresh is not None else out.astype(np.float64)


# ---- order-statistic CFAR on CFAR_2D's window ----------------------------------------------------
def cfar_training_cells(fw, gw):
    """Training cells Nt of the (fw, gw) window: fw^2 - (e2 - e1)^2 with CFAR_2D's guard block [e1, e2)^2 -- 299 at (18, 4),
    not the fw^2 - gw^2 of the reference's gain."""
    return engine.cfar_training_cells(fw, gw)


def os_cfar_threshold(pfa, ncells, rank, law="magnitude"):
    """The multiplier of an order-statistic CFAR for a false-alarm probability: for square-law cells in exponential noise
    Pfa(T) = prod_{i=0}^{rank-1} (N - i) / (N - i + T) (Rohling), solved for T by bisection in float64.
    ``law="magnitude"`` (Rayleigh cells, what |xambg| is) returns sqrt(T), ``law="square"`` T itself.  The result is a
    threshold for the ``plain`` scale of CFAR_2D_OS.  N = 299, rank = 225, Pfa = 1e-3: T = 5.055, sqrt(T) = 2.248."""
    N, k, pfa = int(ncells), int(rank), float(pfa)
    if law not in ("magnitude", "square"):
        raise ValueError("law is 'magnitude' or 'square'")
    if not 1 <= k <= N:
        raise ValueError(f"rank = {k} outside 1 .. {N} cells")
    if not 0.0 < pfa < 1.0:
        raise ValueError("pfa is a probability inside (0, 1)")
    m = N - np.arange(k, dtype=np.float64)

    def log_pfa(T):
        return float(np.sum(np.log(m) - np.log(m + T)))

    target, lo, hi = np.log(pfa), 0.0, 1.0
    while log_pfa(hi) > target:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if log_pfa(mid) > target:
            lo = mid
        else:
            hi = mid
    T = 0.5 * (lo + hi)
    return float(np.sqrt(T)) if law == "magnitude" else float(T)


def CFAR_2D_OS(X, fw, gw, thresh=None, *, rank=None, scale="reference", return_noise=False):
    """Order-statistic CFAR on CFAR_2D's window: the noise estimate z of a cell is the ``rank``-th smallest (1-based,
    default ceil(0.75 Nt)) of its Nt = cfar_training_cells(fw, gw) training cells, selected exactly, instead of their mean
    -- a few strong cells in the window (a second target, the clutter ridge, a sidelobe) leave it untouched.
    ``scale="reference"``: (X / mean|X|) / (z + 1e-10), CFAR_2D's own form, which the trackers and the render chain take
    unchanged; ``scale="plain"``: X / z, the ratio os_cfar_threshold's multiplier applies to.
    X is a 2-D map or a stack [nframes, H, W], NumPy or a torch device tensor, real or complex (|X| is taken on load, as
    CFAR_2D_abs does).  Returns as CFAR_2D: float64 from NumPy (bool with ``thresh``), float32 / bool tensors on the caller's
    device and stream for torch; with ``return_noise=True`` also the z map (float64 / float32)."""
    dev = _lib.is_device_tensor(X)
    if dev:
        import torch
        x = X.to(torch.complex64 if X.is_complex() else torch.float32).contiguous()
        cplx, ndim = x.is_complex(), x.dim()
    else:
        x = np.asarray(X)
        cplx, ndim = np.iscomplexobj(x), x.ndim
        x = np.ascontiguousarray(x, dtype=np.complex64 if cplx else np.float32)
    if ndim not in (2, 3):
        raise ValueError("CFAR_2D_OS takes a 2-D map or a stack [nframes, H, W]")
    frames = 1 if ndim == 2 else int(x.shape[0])
    H, W = int(x.shape[-2]), int(x.shape[-1])
    desc = engine.cfar_os_desc(H, W, fw, gw, rank, scale, cplx, thresh)
    nws = engine.cfar_os_workspace_bytes(desc, max(frames, 1))     # every argument check, on the host
    if dev:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        z = torch.empty_like(out) if return_noise else None
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws else None
        if frames:
            with torch.cuda.device(x.device):          # launch on the tensor's device and torch's stream there
                engine.cfar_os_execute(desc, x, out, z, frames, ws, _lib.torch_stream_ptr(x.device))
        out = out.bool() if thresh is not None else out
        return (out, z) if return_noise else out
    _lib.require_gpu()
    if frames == 0:
        out = np.zeros(x.shape, dtype=bool if thresh is not None else np.float64)
        return (out, np.zeros(x.shape, dtype=np.float64)) if return_noise else out
    st = engine.staging()
    nb = frames * H * W * 4
    dx = st.get("cfar_xc" if cplx else "cfar_x", x.nbytes)
    do = st.get("cfar_o", nb)
    dz = st.get("cfar_z", nb) if return_noise else None
    ws = st.get("cfar_ws", nws) if nws else None
    dx.upload(x)
    engine.cfar_os_execute(desc, dx, do, dz, frames, ws)
    out = do.download(x.shape, np.float32)
    out = out > 0.5 if thresh is not None else out.astype(np.float64)
    return (out, dz.download(x.shape, np.float32).astype(np.float64)) if return_noise else out


def _chain_cfar(x, fw, gw, cfar, cfar_rank):
    """the CFAR stage of the device chains on a torch stack: "mean" = CFAR_2D / CFAR_2D_abs, "os" = CFAR_2D_OS"""
    if cfar == "os":
        return CFAR_2D_OS(x, fw, gw, rank=cfar_rank)
    if cfar != "mean":
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")
    return CFAR_2D_abs(x, fw, gw) if x.is_complex() else CFAR_2D(x, fw, gw)


def _chain_cfar_staged(x, fw, gw, cfar, cfar_rank):
    """the same stage for a host stack [nframes, H, W] on buffers the chain owns (null stream): returns
    (maps buffer, nframes, H, W, what must stay alive)"""
    if cfar not in ("mean", "os"):
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")
    cplx = np.iscomplexobj(x)
    xs = np.ascontiguousarray(x, dtype=np.complex64 if cplx else np.float32)
    nframes, H, W = xs.shape
    dx = _lib.DeviceBuffer(xs.nbytes)
    dx.upload(xs)
    do = _lib.DeviceBuffer(nframes * H * W * 4)
    ws = None
    if cfar == "os":
        desc = engine.cfar_os_desc(H, W, fw, gw, cfar_rank, "reference", cplx)
        ws = _lib.DeviceBuffer(engine.cfar_os_workspace_bytes(desc, nframes))
        engine.cfar_os_execute(desc, dx, do, None, nframes, ws)
    else:
        fn = lib().prc_cfar2d_c64 if cplx else lib().prc_cfar2d
        check(fn(dx.ptr, H, W, int(fw), int(gw), 0, 0.0, do.ptr, nframes, None))
    return do, nframes, H, W, (dx, ws)


# ---- multi-target tracker (target_detection.py:164-537) ---------------------------------------------------------------
# the reference's record types (np.float -> float64, np.int -> int64)
kalman_filter_dtype = np.dtype([("x", np.float64, (4,)), ("P", np.float64, (4, 4)), ("F1", np.float64, (4, 4)),
                                ("F2", np.float64, (4, 4)), ("Q", np.float64, (4, 4)), ("H", np.float64, (2, 4)),
                                ("R", np.float64, (2, 2)), ("S", np.float64, (2, 2))])
target_track_dtype = np.dtype([("status", np.int64), ("lifetime", np.int64), ("measurement", np.float64, (2,)),
                               ("estimate", np.float64, (2,)), ("measurement_history", np.float64, (20,)),
                               ("kalman_state", kalman_filter_dtype)])
# the constants of initialize_track (:375-382)
_F1 = np.array([[1, 0, -0.003, 0], [0, 0, -0.003, -0.003], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
_F2 = np.array([[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
_Q = np.diag([4.0, 0.03, 0.2, 0.08])
_H = np.array([[1, 0, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
_R = np.diag([5.0, 2.0])
TRACK_PERCENTILE = 99.8        # get_measurements ignores its `p` and always takes the 99.8th percentile (:211)


class TrackPlan:
    """Owner of a prc_track_plan (frame shape, track count, candidate capacity, extents).  Any capacity >= 1 works:
    above 2^19 candidates per frame (a threshold on a long run of ties in a frame of more than 2^19 cells) the plan
    allocates a device workspace of capacity / 8 bytes for the tracker's per-candidate bits, which otherwise sit in LDS."""

    def __init__(self, H, W, ntracks, capacity, frame_extent, percentile=TRACK_PERCENTILE):
        d = _lib.TrackDesc()
        d.H, d.W, d.ntracks, d.capacity = int(H), int(W), int(ntracks), int(capacity)
        d.percentile = float(percentile)
        d.doppler_extent, d.range_extent = float(frame_extent[0]), float(frame_extent[1])
        self.H, self.W, self.ntracks, self.capacity = d.H, d.W, d.ntracks, d.capacity
        h = C.c_void_p()
        check(lib().prc_track_plan_create(C.byref(h), C.byref(d)))
        self.handle = h.value

    def measure(self, frames, nframes, counts, cands, stream=None):
        check(lib().prc_track_measure(self.handle, frames, int(nframes), counts, cands, stream))

    def run(self, counts, cands, nframes, records, stream=None):
        check(lib().prc_track_run(self.handle, counts, cands, int(nframes), records, stream))

    def close(self):
        if getattr(self, "handle", None):
            lib().prc_track_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def expected_capacity(H, W, percentile=TRACK_PERCENTILE):
    """candidates a tie-free frame has at the percentile (n - 1 - k), plus a margin"""
    n = int(H) * int(W)
    k = int(np.floor(np.float64(n - 1) * np.true_divide(np.float64(percentile), 100)))
    return max(1, n - 1 - k) + 64


def _frames_shape(x):
    if x.ndim == 2:
        return 1, x.shape[0], x.shape[1]
    if x.ndim == 3:
        return x.shape[0], x.shape[1], x.shape[2]
    raise ValueError("expected a frame [H, W] or a stack [nframes, H, W]")


class _Measured:
    """counts + candidate records of a stack of frames on the device, measured with a plan whose capacity holds every
    frame's candidates: after one measure the counts are read, and if any exceeds the capacity the plan is rebuilt at
    the exact maximum and the stack measured again (a deterministic sizing step).  ``capacity`` pins the capacity (no
    rebuild: frames over it keep their first `capacity` candidates and the tracker flags them); ``start_capacity`` only
    replaces the first guess (default: expected_capacity)."""

    def __init__(self, frames_ptr, nframes, H, W, frame_extent, ntracks, alloc, stream, percentile=TRACK_PERCENTILE,
                 capacity=None, start_capacity=None):
        self.alloc, self.stream = alloc, stream
        self.nframes = nframes
        self.rebuilt = False
        cap = int(capacity or start_capacity or expected_capacity(H, W, percentile))
        self.counts_buf = alloc("counts", 4 * max(nframes, 1))
        for attempt in range(2):
            self.plan = TrackPlan(H, W, ntracks, cap, frame_extent, percentile)
            self.cands_buf = alloc("cands", 32 * max(nframes, 1) * cap)
            self.plan.measure(frames_ptr, nframes, self.counts_buf.ptr, self.cands_buf.ptr, stream)
            self.counts = self.counts_buf.download(nframes, np.int32, stream=stream)
            need = int(self.counts.max()) if nframes else 0
            if need <= cap or capacity:
                break
            cap = need
            self.rebuilt = True
        self.capacity = cap

    def candidates(self):
        raw = self.cands_buf.download(self.nframes * self.capacity, _lib.TRACK_CAND_DTYPE, stream=self.stream)
        return raw.reshape(self.nframes, self.capacity)

    def run(self):
        rec = self.alloc("records", 256 * max(self.nframes, 1) * self.plan.ntracks)
        self.plan.run(self.counts_buf.ptr, self.cands_buf.ptr, self.nframes, rec.ptr, self.stream)
        out = rec.download(self.nframes * self.plan.ntracks, _lib.TRACK_RECORD_DTYPE, stream=self.stream)
        return out.reshape(self.nframes, self.plan.ntracks)


class _TorchBuf:
    """a device byte buffer from torch's allocator with DeviceBuffer's download()"""

    def __init__(self, nbytes, device):
        import torch
        self.t = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)
        self.ptr = self.t.data_ptr()

    def download(self, shape, dtype, stream=None):
        out = np.empty(shape, dtype=dtype)
        check(lib().prc_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream))
        check(lib().prc_stream_sync(stream))
        return out


def _device_measure(x, frame_extent, ntracks=1, capacity=None, percentile=TRACK_PERCENTILE, start_capacity=None):
    """measure a 2-D frame or [nframes, H, W] stack: numpy (staged) or a torch device tensor (on its stream)"""
    if _lib.is_device_tensor(x):
        import torch
        t = x.to(torch.float32).contiguous()
        nframes, H, W = _frames_shape(t)
        stream = _lib.torch_stream_ptr(t.device)
        with torch.cuda.device(t.device):
            m = _Measured(t.data_ptr(), nframes, H, W, frame_extent, ntracks, lambda name, nb: _TorchBuf(nb, t.device),
                          stream, percentile, capacity, start_capacity)
        m.keep = t
        return m
    f = np.ascontiguousarray(x, dtype=np.float32)
    nframes, H, W = _frames_shape(f)
    _lib.require_gpu()
    dx = _lib.DeviceBuffer(f.nbytes)
    dx.upload(f)
    m = _Measured(dx.ptr, nframes, H, W, frame_extent, ntracks, lambda name, nb: _lib.DeviceBuffer(nb), None,
                  percentile, capacity, start_capacity)
    m.keep = dx
    return m


def _cands_to_meas(c, count):
    c = c[:count]
    return np.stack((c["range"], c["doppler"], c["strength"]))


def get_measurements(dataFrame, p, frame_extent):
    """get_measurements (target_detection.py:164-229): candidate measurements of one range-Doppler frame (H Doppler rows
    x W range columns) as (3, M) float64 -- range, Doppler, strength, strongest first (ties: the later cell of the
    reference's fliplr(frame.T) order first).  ``p`` is ignored, as in the reference (always the 99.8th percentile).
    A torch device stack [N, H, W] returns ``(counts, meas, index)`` on the device instead: int32 [N], float64
    [N, 3, capacity] (range, Doppler, strength; entries past counts[i] unused) and int64 [N, capacity] flat indices."""
    if _lib.is_device_tensor(dataFrame):
        import torch
        m = _device_measure(dataFrame, frame_extent)
        raw = m.cands_buf.t[:32 * m.nframes * m.capacity].view(torch.float64).view(m.nframes, m.capacity, 4)
        meas = raw[:, :, [1, 2, 0]].permute(0, 2, 1).contiguous()
        index = m.cands_buf.t[:32 * m.nframes * m.capacity].view(torch.int64).view(m.nframes, m.capacity, 4)[:, :, 3]
        counts = m.counts_buf.t[:4 * m.nframes].view(torch.int32).clone()
        return counts, meas, index.contiguous()
    x = np.asarray(dataFrame)
    if x.ndim != 2:
        raise ValueError("get_measurements takes one 2-D frame (a torch device stack for batches)")
    m = _device_measure(x, frame_extent)
    return _cands_to_meas(m.candidates()[0], int(m.counts[0]))


def _records_to_history(rec, ntracks):
    out = np.zeros(rec.shape, dtype=target_track_dtype)
    out["status"] = rec["status"]
    out["lifetime"] = rec["lifetime"]
    out["measurement"] = rec["measurement"]
    out["estimate"] = rec["estimate"]
    out["measurement_history"] = rec["history"].astype(np.float64)
    ks = out["kalman_state"]
    ks["x"] = rec["x"]
    ks["P"] = rec["P"].reshape(rec.shape + (4, 4))
    ks["S"] = rec["S"].reshape(rec.shape + (2, 2))
    ks["F1"], ks["F2"], ks["Q"], ks["H"], ks["R"] = _F1, _F2, _Q, _H, _R
    out["kalman_state"] = ks
    if rec["overflow"].any():
        raise _lib.PrcoreError(_lib.PRC_EINVAL, "multitarget_tracker: a frame's candidates exceeded the plan's capacity")
    return out


def multitarget_tracker(data, frame_extent, N_TRACKS):
    """multitarget_tracker (target_detection.py:455-537): ``data`` is numpy (H, W, Nframes) as the reference takes it
    (converted to float32), or a torch device tensor [N, H, W]; frame_extent = [max Doppler, max range].  Returns the
    reference's (Nframes, N_TRACKS) array of target_track_dtype."""
    if _lib.is_device_tensor(data):
        x = data
    else:
        d = np.asarray(data)
        if d.ndim != 3:
            raise ValueError("multitarget_tracker takes (H, W, Nframes) frames")
        x = np.moveaxis(d, 2, 0)
    m = _device_measure(x, frame_extent, int(N_TRACKS))
    return _records_to_history(m.run(), int(N_TRACKS))


def track_maps(xambg, frame_extent, N_TRACKS=10, fw=18, gw=4, cfar="mean", cfar_rank=None):
    """multitarget_kalman_tracker.py:44-63 as one device chain on the caller's stream: CFAR_2D(|xambg|, fw, gw) per
    frame (CFAR_2D_abs; CFAR_2D for a real magnitude stack) -> get_measurements -> multitarget_tracker.  ``xambg`` is a
    torch device tensor [N, H, W] or numpy (H, W, Nframes) as the script loads it.  ``cfar="os"`` puts CFAR_2D_OS
    (reference scale, rank ``cfar_rank``, default ceil(0.75 Nt)) in the cell average's place."""
    if _lib.is_device_tensor(xambg):
        cf = _chain_cfar(xambg, fw, gw, cfar, cfar_rank)
        if cf.dim() == 2:
            cf = cf.unsqueeze(0)
        return multitarget_tracker(cf, frame_extent, N_TRACKS)
    x = np.moveaxis(np.asarray(xambg), 2, 0)
    _lib.require_gpu()
    do, nframes, H, W, keep = _chain_cfar_staged(x, fw, gw, cfar, cfar_rank)
    m = _Measured(do.ptr, nframes, H, W, frame_extent, int(N_TRACKS), lambda name, nb: _lib.DeviceBuffer(nb), None)
    return _records_to_history(m.run(), int(N_TRACKS))


# ---- single-target tracker (target_detection.py:530-681) ---------------------------------------------------------------
target_track_dtype_simple = np.dtype([("lock_mode", np.float64, (4,)), ("measurement", np.float64, (2,)),
                                      ("measurement_idx", np.int64, (2,)), ("estimate", np.float64, (2,)),
                                      ("range_extent", np.float64), ("doppler_extent", np.float64),
                                      ("kalman_state", kalman_filter_dtype)])
# the constants of simple_target_tracker (:640-647) -- F1[1] and Q, R differ from multitarget_tracker's
_SF1 = np.array([[1, 0, -0.003, 0], [0, 0, -0.003, -0.03], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64)
_SQ = np.diag([2.0, 0.02, 0.2, 0.05])
_SR = np.diag([5.0, 5.0])


def _strack_records_to_history(rec, range_extent, doppler_extent):
    out = np.zeros(rec.shape, dtype=target_track_dtype_simple)
    for k in ("lock_mode", "measurement", "measurement_idx", "estimate"):
        out[k] = rec[k]
    out["range_extent"] = range_extent
    out["doppler_extent"] = doppler_extent
    ks = out["kalman_state"]
    ks["x"] = rec["x"]
    ks["P"] = rec["P"].reshape(rec.shape + (4, 4))
    ks["S"] = rec["S"].reshape(rec.shape + (2, 2))
    ks["F1"], ks["F2"], ks["Q"], ks["H"], ks["R"] = _SF1, _F2, _SQ, _H, _SR
    out["kalman_state"] = ks
    return out


def _strack_state_record(state):
    """a history row (target_track_dtype_simple) as a prc_strack_record"""
    row = np.asarray(state).reshape(-1)
    if row.size != 1 or row.dtype.names is None:
        raise ValueError("state= takes one row of a simple_target_tracker history")
    row = row[0]
    rec = np.zeros(1, dtype=_lib.STRACK_RECORD_DTYPE)
    for k in ("lock_mode", "measurement", "measurement_idx", "estimate"):
        rec[k] = row[k]
    ks = row["kalman_state"]
    rec["x"] = np.asarray(ks["x"]).reshape(4)
    rec["P"] = np.asarray(ks["P"]).reshape(16)
    rec["S"] = np.asarray(ks["S"]).reshape(4)
    return rec


def _strack_desc(H, W, dtype, range_extent, doppler_extent):
    d = _lib.StrackDesc()
    d.H, d.W, d.dtype = int(H), int(W), int(dtype)
    d.range_extent, d.doppler_extent = float(range_extent), float(doppler_extent)
    return d


def _strack_run(frames_ptr, nframes, H, W, dtype, range_extent, doppler_extent, state, alloc, stream):
    """prc_strack_run on device frames [nframes][H][W]; returns the records as STRACK_RECORD_DTYPE"""
    d = _strack_desc(H, W, dtype, range_extent, doppler_extent)
    nb = C.c_size_t(0)
    check(lib().prc_strack_workspace_bytes(C.byref(d), int(nframes), C.byref(nb)))
    ws = alloc(nb.value)
    rec = alloc(_lib.STRACK_RECORD_DTYPE.itemsize * max(nframes, 1))
    st_ptr = None
    if state is not None:
        st = _lib.DeviceBuffer(_lib.STRACK_RECORD_DTYPE.itemsize)
        st.upload(_strack_state_record(state))
        st_ptr = st.ptr
    check(lib().prc_strack_run(C.byref(d), frames_ptr, int(nframes), st_ptr, rec.ptr, ws.ptr, stream))
    out = rec.download(nframes, _lib.STRACK_RECORD_DTYPE, stream=stream)
    return out


def simple_target_tracker(data, rangeExtent, dopplerExtent, *, state=None):
    """simple_target_tracker (target_detection.py:626-681): ``data`` is numpy (H Doppler, W range, Nframes) as the
    reference takes it (float32 stays float32, anything else becomes float64), or a torch device tensor [N, H, W] of
    float32 / float64.  Returns the reference's (Nframes,) history of target_track_dtype_simple, computed as the
    reference does on the frames as float64 (a float64 frame may differ only where the reference's own division by the
    frame mean merges two values within about one ulp).  ``state=`` (the one extension) is a history row -- the last
    one of an earlier call -- to resume from; without it the track starts from the reference's initial state."""
    if _lib.is_device_tensor(data):
        import torch
        t = data if data.dtype in (torch.float32, torch.float64) else data.to(torch.float64)
        t = t.contiguous()
        if t.dim() != 3:
            raise ValueError("simple_target_tracker takes a device stack [N, H, W]")
        N, H, W = t.shape
        dt = _lib.REAL_F32 if t.dtype == torch.float32 else _lib.REAL_F64
        with torch.cuda.device(t.device):
            rec = _strack_run(t.data_ptr(), N, H, W, dt, rangeExtent, dopplerExtent, state,
                              lambda nb: _TorchBuf(nb, t.device), _lib.torch_stream_ptr(t.device))
        return _strack_records_to_history(rec, rangeExtent, dopplerExtent)
    d = np.asarray(data)
    if d.ndim != 3:
        raise ValueError("simple_target_tracker takes (H, W, Nframes) frames")
    f = np.ascontiguousarray(np.moveaxis(d, 2, 0), dtype=np.float32 if d.dtype == np.float32 else np.float64)
    N, H, W = f.shape
    _lib.require_gpu()
    dx = _lib.DeviceBuffer(f.nbytes)
    dx.upload(f)
    rec = _strack_run(dx.ptr, N, H, W, _lib.REAL_F32 if f.dtype == np.float32 else _lib.REAL_F64, rangeExtent,
                      dopplerExtent, state, lambda nb: _lib.DeviceBuffer(nb), None)
    return _strack_records_to_history(rec, rangeExtent, dopplerExtent)


def simple_track_maps(xambg, rangeExtent, dopplerExtent, fw=18, gw=4, cfar="mean", cfar_rank=None):
    """simple_kalman_tracker.py:46-61 as one device chain on the caller's stream: CFAR_2D(|xambg|, fw, gw) per frame
    (CFAR_2D_abs; CFAR_2D for a real magnitude stack) -> simple_target_tracker on the float32 CFAR maps.  ``xambg`` is
    a torch device tensor [N, H, W] or numpy (H, W, Nframes) as the script loads it.  ``cfar="os"`` puts CFAR_2D_OS
    (reference scale, rank ``cfar_rank``) in the cell average's place."""
    if _lib.is_device_tensor(xambg):
        cf = _chain_cfar(xambg, fw, gw, cfar, cfar_rank)
        if cf.dim() == 2:
            cf = cf.unsqueeze(0)
        return simple_target_tracker(cf, rangeExtent, dopplerExtent)
    x = np.moveaxis(np.asarray(xambg), 2, 0)
    _lib.require_gpu()
    do, nframes, H, W, keep = _chain_cfar_staged(x, fw, gw, cfar, cfar_rank)
    rec = _strack_run(do.ptr, nframes, H, W, _lib.REAL_F32, rangeExtent, dopplerExtent, None,
                      lambda nb: _lib.DeviceBuffer(nb), None)
    return _strack_records_to_history(rec, rangeExtent, dopplerExtent)


# ---- sub-cell peak refinement of exact ambiguity patches (range_doppler_processing.xambg_patch) ------------------------
def refine_peaks(X, lags, dopplers, doppler_step):
    """Per patch of ``X`` (complex64 [npatches, ndoppler, nlags], from ``xambg_patch`` with origins ``lags`` / ``dopplers``
    and spacing ``doppler_step``): the argmax of |X|^2 (the first cell in [d][l] order wins ties) and a 3-point parabola on
    |X| along each axis, off = (y- - y+) / (2 (y- - 2 y0 + y+)) clamped to +-1/2 (prc_xambg_patch_peaks of
    include/prcore.h, one wavefront per patch).  Fields: ``lag`` (samples), ``doppler`` (Hz), ``amplitude`` (|X| at the
    argmax cell), ``d``, ``l`` (the cell), ``flags`` (bit 0: the argmax is on a Doppler edge, that axis is not interpolated;
    bit 1: the same for lag; bit 2: a flat patch, dead air included: cell (0, 0), offsets 0).
    Returns a structured array (_lib.PATCH_PEAK_DTYPE) for NumPy input; for a torch device tensor a dict of device tensors
    by field name (nothing returns to the host)."""
    if len(X.shape) != 3:
        raise ValueError("refine_peaks takes patches [npatches, ndoppler, nlags]")
    npatches, ndoppler, nlags = (int(v) for v in X.shape)
    rec = engine.patch_list(lags, dopplers)
    if rec.shape[0] != npatches:
        raise ValueError(f"{npatches} patches but {rec.shape[0]} origins")
    desc = engine.patch_desc(1, nlags, ndoppler, 1.0, doppler_step)
    if _lib.is_device_tensor(X):
        import torch
        with torch.cuda.device(X.device):
            x = X.to(torch.complex64).contiguous()
            raw = torch.empty((npatches, _lib.PATCH_PEAK_DTYPE.itemsize), dtype=torch.uint8, device=x.device)
            d_rec = torch.from_numpy(rec.view(np.uint8)).to(x.device)
            if npatches:
                engine.xambg_patch_peaks(desc, d_rec, npatches, x, raw, _lib.torch_stream_ptr(x.device))
        f64, f32, i32 = raw.view(torch.float64), raw.view(torch.float32), raw.view(torch.int32)
        return {"lag": f64[:, 0], "doppler": f64[:, 1], "amplitude": f32[:, 4], "d": i32[:, 5], "l": i32[:, 6],
                "flags": i32[:, 7]}
    x = np.ascontiguousarray(X, dtype=np.complex64)
    if npatches == 0:
        return np.zeros(0, dtype=_lib.PATCH_PEAK_DTYPE)
    _lib.require_gpu()
    st = engine.staging()
    d_x = st.get("xp_out", x.nbytes)
    d_rec = st.get("xp_rec", rec.nbytes)
    d_pk = st.get("xp_peaks", npatches * _lib.PATCH_PEAK_DTYPE.itemsize)
    d_x.upload(x)
    d_rec.upload(rec.view(np.uint8))
    engine.xambg_patch_peaks(desc, d_rec, npatches, d_x, d_pk)
    return d_pk.download((npatches,), _lib.PATCH_PEAK_DTYPE)
