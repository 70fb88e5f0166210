"""Drop-ins for the reference's ``passiveRadar/target_detection.py``: ``CFAR_2D`` (:683-703), applied per frame to
``|xambg|`` by range_doppler_plot.py:56-57 (SURVEY 8f "next" #3), the multi-target Kalman tracker of
multitarget_kalman_tracker.py: ``get_measurements`` (:164-229) and ``multitarget_tracker`` (:455-537), plus
``track_maps``, that script's CFAR -> measure -> track chain (:44-63) in one device pass, and the single-target tracker
of simple_kalman_tracker.py: ``simple_target_tracker`` (:626-681), plus ``simple_track_maps``, its CFAR -> track
chain (:46-61).  Beyond the reference: ``CFAR_2D_OS``, the order-statistic CFAR on CFAR_2D's window (with
``cfar_training_cells`` and ``os_cfar_threshold``), which the chains take with ``cfar="os"``, ``refine_peaks``, and
``extract_plots``, the plot extractor between a CFAR map and the tracker (``track_maps(..., measure="plots")``), and
track-before-detect: ``track_before_detect`` (the Viterbi integration of a stack of CFAR maps along the paths the Doppler
rows allow, ``tbd_row_shifts``), ``tbd_paths`` and the chain ``tbd_maps``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, engine
from ._lib import check, lib

__all__ = ["CFAR_2D", "CFAR_2D_abs", "CFAR_2D_OS", "cfar_training_cells", "os_cfar_threshold", "get_measurements",
           "multitarget_tracker", "track_maps",
           "kalman_filter_dtype", "target_track_dtype", "simple_target_tracker", "simple_track_maps",
           "target_track_dtype_simple", "refine_peaks", "extract_plots", "tbd_row_shifts", "track_before_detect", "tbd_paths",
           "tbd_maps"]


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


def _chain_cfar(x, fw, gw, cfar, cfar_rank, scale="reference"):
    """the CFAR stage of the device chains on a torch stack: "mean" = CFAR_2D / CFAR_2D_abs, "os" = CFAR_2D_OS (``scale``
    applies to it alone)"""
    if cfar == "os":
        return CFAR_2D_OS(x, fw, gw, rank=cfar_rank, scale=scale)
    if cfar != "mean":
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")
    return CFAR_2D_abs(x, fw, gw) if x.is_complex() else CFAR_2D(x, fw, gw)


def _chain_cfar_staged(x, fw, gw, cfar, cfar_rank, scale="reference"):
    """the same stage for a host stack [nframes, H, W] on buffers the chain owns (null stream): returns
    (maps buffer, nframes, H, W, what must stay alive: the uploaded input first)"""
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
        desc = engine.cfar_os_desc(H, W, fw, gw, cfar_rank, scale, cplx)
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


def track_maps(xambg, frame_extent, N_TRACKS=10, fw=18, gw=4, cfar="mean", cfar_rank=None, measure="percentile",
               plot_thresh=None, plot_connectivity=8, plot_max_cells=None, plot_capacity=None):
    """multitarget_kalman_tracker.py:44-63 as one device chain on the caller's stream: CFAR_2D(|xambg|, fw, gw) per
    frame (CFAR_2D_abs; CFAR_2D for a real magnitude stack) -> get_measurements -> multitarget_tracker.  ``xambg`` is a
    torch device tensor [N, H, W] or numpy (H, W, Nframes) as the script loads it.  ``cfar="os"`` puts CFAR_2D_OS
    (reference scale, rank ``cfar_rank``, default ceil(0.75 Nt)) in the cell average's place.
    ``measure="plots"`` (beyond the reference) puts the plot extractor in get_measurements' place: the CFAR map is
    thresholded at ``plot_thresh`` (required) and every connected cluster (``plot_connectivity``) is one measurement at its
    centroid, weighted by |xambg| (extract_plots).  With ``cfar="os"`` the CFAR then runs on the ``plain`` scale, the one
    os_cfar_threshold's multiplier applies to; with ``cfar="mean"`` on CFAR_2D's ratio.  ``plot_max_cells`` /
    ``plot_capacity`` pin the extractor's bounds (default: sized from the counts); a frame over a pinned bound raises
    PrcoreError, as the tracker's overflow does."""
    if measure not in ("percentile", "plots"):
        raise ValueError(f"measure is 'percentile' or 'plots', not {measure!r}")
    if measure == "plots":
        if plot_thresh is None:
            raise ValueError("measure='plots' needs plot_thresh")
        return _track_plots(xambg, frame_extent, int(N_TRACKS), fw, gw, cfar, cfar_rank, float(plot_thresh),
                            plot_connectivity, plot_max_cells, plot_capacity)
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


# ---- plot extraction (beyond the reference) -------------------------------------------------------
PLOTS_DEFAULT_CAPACITY = 512


class _Plots:
    """counts + one prc_track_cand per plot of a stack of statistic frames on the device (prc_plots).  A bound left at
    None is sized from what the call reports, as _Measured sizes its capacity: after a run ncells / counts are read, and if
    a frame exceeded ``max_cells`` the stack is run again at the exact maximum (the workspace path if that is above
    PRC_PLOTS_LDS_CELLS); if then, or at first, a frame has more plots than ``capacity``, once more at that exact maximum
    (the plot count of a frame over max_cells is only known after the first re-run).  A pinned bound is never changed: the
    caller sees the overflow in ncells / counts.  ``start_max_cells`` / ``start_capacity`` only replace the first guesses."""

    def __init__(self, stat_ptr, weight_ptr, complex_weight, nframes, H, W, thresh, frame_extent, alloc, stream,
                 connectivity=8, range_guard=8, doppler_guard=4, max_cells=None, capacity=None, want_info=False,
                 start_max_cells=None, start_capacity=None):
        self.alloc, self.stream, self.nframes = alloc, stream, nframes
        mc = int(max_cells or start_max_cells or _lib.PLOTS_LDS_CELLS)
        cap = int(capacity or start_capacity or PLOTS_DEFAULT_CAPACITY)
        nf = max(nframes, 1)
        self.counts_buf = alloc("plot_counts", 4 * nf)
        self.ncells_buf = alloc("plot_ncells", 4 * nf)
        self.runs = 0
        while True:
            desc = engine.plots_desc(H, W, thresh, frame_extent, connectivity, range_guard, doppler_guard, mc, cap,
                                     complex_weight)
            nws = engine.plots_workspace_bytes(desc, nframes)
            self.cands_buf = alloc("plot_cands", 32 * nf * cap)
            self.info_buf = alloc("plot_info", _lib.PLOT_INFO_DTYPE.itemsize * nf * cap) if want_info else None
            ws = alloc("plot_ws", nws) if nws else None
            check(lib().prc_memset(self.cands_buf.ptr, 0, 32 * nf * cap, stream))        # slots past a count read as zeros
            if want_info:
                check(lib().prc_memset(self.info_buf.ptr, 0, _lib.PLOT_INFO_DTYPE.itemsize * nf * cap, stream))
            engine.plots_execute(desc, stat_ptr, weight_ptr, nframes, self.counts_buf.ptr, self.ncells_buf.ptr,
                                 self.cands_buf.ptr, self.info_buf.ptr if want_info else None, ws.ptr if ws else None, stream)
            self.runs += 1
            self.counts = self.counts_buf.download(nframes, np.int32, stream=stream)
            self.ncells = self.ncells_buf.download(nframes, np.int32, stream=stream)
            need_mc = int(self.ncells.max()) if nframes else 0
            need_cap = int(self.counts.max()) if nframes else 0
            grow_mc = max_cells is None and need_mc > mc
            grow_cap = capacity is None and need_cap > cap
            if not (grow_mc or grow_cap) or self.runs == 3:
                break
            mc = need_mc if grow_mc else mc
            cap = need_cap if grow_cap else cap
        self.max_cells, self.capacity = mc, cap

    def stored(self):
        """plots written per frame"""
        return np.minimum(self.counts, self.capacity)

    def overflowed(self):
        return bool((self.ncells > self.max_cells).any() or (self.counts > self.capacity).any())

    def candidates(self):
        raw = self.cands_buf.download(self.nframes * self.capacity, _lib.TRACK_CAND_DTYPE, stream=self.stream)
        return raw.reshape(self.nframes, self.capacity)

    def info(self):
        raw = self.info_buf.download(self.nframes * self.capacity, _lib.PLOT_INFO_DTYPE, stream=self.stream)
        return raw.reshape(self.nframes, self.capacity)


def _plots_check_host(H, W, thresh, frame_extent, connectivity, range_guard, doppler_guard, max_cells, capacity, nframes):
    """every argument check of prc_plots, on the host (ValueError), before a device is touched"""
    for name, v in (("max_cells", max_cells), ("capacity", capacity)):
        if v is not None and int(v) < 1:
            raise ValueError(f"{name} = {v}, not >= 1")
    desc = engine.plots_desc(H, W, thresh, frame_extent, connectivity, range_guard, doppler_guard, max_cells,
                             PLOTS_DEFAULT_CAPACITY if capacity is None else capacity)
    engine.plots_workspace_bytes(desc, nframes)


def _device_plots(stat, thresh, frame_extent, weight, **kw):
    """_Plots of a 2-D frame or [nframes, H, W] stack: numpy (staged, null stream) or a torch device tensor (its stream)"""
    dev = _lib.is_device_tensor(stat)
    if weight is not None and _lib.is_device_tensor(weight) != dev:
        raise ValueError("stat and weight are both NumPy arrays or both device tensors")
    if dev:
        import torch
        t = stat.to(torch.float32).contiguous()
        w = None if weight is None else weight.to(torch.complex64 if weight.is_complex() else torch.float32).contiguous()
        shape, wshape, cplx = tuple(t.shape), None if w is None else tuple(w.shape), w is not None and w.is_complex()
    else:
        t = np.ascontiguousarray(stat, dtype=np.float32)
        w = None
        if weight is not None:
            w = np.asarray(weight)
            w = np.ascontiguousarray(w, dtype=np.complex64 if np.iscomplexobj(w) else np.float32)
        shape, wshape, cplx = t.shape, None if w is None else w.shape, w is not None and np.iscomplexobj(w)
    if len(shape) not in (2, 3):
        raise ValueError("extract_plots takes a frame [H, W] or a stack [nframes, H, W]")
    if wshape is not None and wshape != shape:
        raise ValueError(f"weight has shape {wshape}, stat {shape}")
    nframes, H, W = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    _plots_check_host(H, W, thresh, frame_extent, kw.get("connectivity", 8), kw.get("range_guard", 8),
                      kw.get("doppler_guard", 4), kw.get("max_cells"), kw.get("capacity"), nframes)
    if dev:
        stream = _lib.torch_stream_ptr(t.device)
        with torch.cuda.device(t.device):
            m = _Plots(t.data_ptr(), None if w is None else w.data_ptr(), cplx, nframes, H, W, thresh, frame_extent,
                       lambda name, nb: _TorchBuf(nb, t.device), stream, **kw)
        m.keep = (t, w)
        return m
    _lib.require_gpu()
    dx = _lib.DeviceBuffer(t.nbytes)
    dx.upload(t)
    dw = None
    if w is not None:
        dw = _lib.DeviceBuffer(w.nbytes)
        dw.upload(w)
    m = _Plots(dx.ptr, None if dw is None else dw.ptr, cplx, nframes, H, W, thresh, frame_extent,
               lambda name, nb: _lib.DeviceBuffer(nb), None, **kw)
    m.keep = (dx, dw)
    return m


def extract_plots(stat, thresh, frame_extent, *, weight=None, connectivity=8, range_guard=8, doppler_guard=4,
                  max_cells=None, capacity=None, return_info=False, start_max_cells=None, start_capacity=None):
    """Plot extraction (prc_plots of include/prcore.h): the cells of a CFAR statistic with ``stat > thresh`` outside
    get_measurements' excluded zones (``range_guard`` range columns at either end, ``doppler_guard`` Doppler columns either
    side of zero; 0 switches a zone off), grouped into connected clusters (``connectivity`` 4 or 8), one measurement per
    cluster: range and Doppler of the centroid weighted by ``weight`` (same shape; complex: its magnitude; default: stat
    itself) and the cluster's largest stat as strength -- strongest first, ties as get_measurements breaks them.
    A NumPy 2-D frame (H Doppler rows x W range columns) returns (3, M) float64 -- range, Doppler, strength --
    get_measurements' shape.  A NumPy stack [N, H, W] or a torch device stack returns ``(counts, meas, index)`` as
    get_measurements does for device stacks (int32 [N]; float64 [N, 3, capacity]; int64 [N, capacity]; entries past
    counts[i] are zero), arrays for NumPy, tensors on the caller's device and torch's current stream for torch.
    ``return_info=True`` appends the prc_plot_info records (a structured array of _lib.PLOT_INFO_DTYPE, [N, capacity] /
    [M]; a uint8 tensor [N, capacity, 48] for torch) and ncells, the detecting cells per frame.
    ``max_cells`` (detections held per frame, default PRC_PLOTS_LDS_CELLS) and ``capacity`` (plots stored per frame, default
    512) left at None are sized from the counts: a frame over either makes the call run again at the exact maximum.  A
    pinned bound is kept: counts[i] > capacity means only the first ``capacity`` plots were stored, ncells[i] > max_cells
    that frame i was not extracted (counts[i] = 0).  ``start_max_cells`` / ``start_capacity`` replace the first guesses."""
    thresh = float(thresh)
    m = _device_plots(stat, thresh, frame_extent, weight, connectivity=connectivity, range_guard=range_guard,
                      doppler_guard=doppler_guard, max_cells=max_cells, capacity=capacity, want_info=return_info,
                      start_max_cells=start_max_cells, start_capacity=start_capacity)
    N, cap = m.nframes, m.capacity
    if _lib.is_device_tensor(stat):
        import torch
        raw = m.cands_buf.t[:32 * N * cap]
        meas = raw.view(torch.float64).view(N, cap, 4)[:, :, [1, 2, 0]].permute(0, 2, 1).contiguous()
        index = raw.view(torch.int64).view(N, cap, 4)[:, :, 3].contiguous()
        counts = m.counts_buf.t[:4 * N].view(torch.int32).clone()
        if not return_info:
            return counts, meas, index
        nb = _lib.PLOT_INFO_DTYPE.itemsize
        return counts, meas, index, m.info_buf.t[:nb * N * cap].view(N, cap, nb).clone(), m.ncells_buf.t[:4 * N].view(torch.int32).clone()
    c = m.candidates()
    if len(np.shape(stat)) == 2:
        k = int(m.stored()[0])
        meas = _cands_to_meas(c[0], k)
        return (meas, m.info()[0][:k], int(m.ncells[0])) if return_info else meas
    meas = np.ascontiguousarray(np.stack((c["range"], c["doppler"], c["strength"]), axis=1))
    out = (m.counts, meas, np.ascontiguousarray(c["index"]))
    return out + (m.info(), m.ncells) if return_info else out


def _track_plots(xambg, frame_extent, ntracks, fw, gw, cfar, cfar_rank, thresh, connectivity, max_cells, capacity):
    """CFAR -> prc_plots -> prc_track_run on one stream; the maps themselves are the weights"""
    if cfar not in ("mean", "os"):
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")
    dev = _lib.is_device_tensor(xambg)
    if dev:
        import torch
        x = xambg.to(torch.complex64 if xambg.is_complex() else torch.float32).contiguous()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        shape, cplx = tuple(x.shape), x.is_complex()
    else:
        x = np.asarray(xambg)
        if x.ndim != 3:
            raise ValueError("track_maps takes (H, W, Nframes) frames")
        x = np.moveaxis(x, 2, 0)
        shape, cplx = x.shape, np.iscomplexobj(x)
    if len(shape) != 3:
        raise ValueError("track_maps takes a device stack [N, H, W]")
    nframes, H, W = (int(v) for v in shape)
    _plots_check_host(H, W, thresh, frame_extent, connectivity, 8, 4, max_cells, capacity, nframes)
    kw = dict(connectivity=connectivity, max_cells=max_cells, capacity=capacity)
    if dev:
        cf = _chain_cfar(x, fw, gw, cfar, cfar_rank, "plain")
        stream = _lib.torch_stream_ptr(x.device)
        alloc = lambda name, nb: _TorchBuf(nb, x.device)      # noqa: E731
        with torch.cuda.device(x.device):
            m = _Plots(cf.data_ptr(), x.data_ptr(), cplx, nframes, H, W, thresh, frame_extent, alloc, stream, **kw)
            rec = _plots_run_tracker(m, H, W, ntracks, frame_extent, alloc, stream)
    else:
        _lib.require_gpu()
        do, nframes, H, W, keep = _chain_cfar_staged(x, fw, gw, cfar, cfar_rank, "plain")
        alloc = lambda name, nb: _lib.DeviceBuffer(nb)        # noqa: E731
        m = _Plots(do.ptr, keep[0].ptr, cplx, nframes, H, W, thresh, frame_extent, alloc, None, **kw)
        rec = _plots_run_tracker(m, H, W, ntracks, frame_extent, alloc, None)
    return _records_to_history(rec, ntracks)


def _plots_run_tracker(m, H, W, ntracks, frame_extent, alloc, stream):
    if (m.ncells > m.max_cells).any():
        raise _lib.PrcoreError(_lib.PRC_EINVAL, "track_maps: a frame's detections exceeded plot_max_cells")
    plan = TrackPlan(H, W, ntracks, m.capacity, frame_extent)
    rec = alloc("records", 256 * max(m.nframes, 1) * ntracks)
    plan.run(m.counts_buf.ptr, m.cands_buf.ptr, m.nframes, rec.ptr, stream)
    out = rec.download(m.nframes * ntracks, _lib.TRACK_RECORD_DTYPE, stream=stream)
    plan.close()
    return out.reshape(m.nframes, ntracks)


# ---- track-before-detect (beyond the reference) ---------------------------------------------------
def tbd_row_shifts(H, W, frame_extent, frame_interval, wavelength):
    """Range columns an echo in Doppler row h advances per frame, int32 [H], for prc_tbd's ``row_shift``.  Bistatic Doppler
    is bistatic range rate, f = -(1/lambda) dR/dt, so on the axes of get_measurements / prc_plots (Doppler of row h:
    f_h = D - h 2D/(H-1) Hz, evaluated as (H-1-2h) D/(H-1) so that s[h] = -s[H-1-h] holds exactly; range of column w:
    R - w R/(W-1) km; [D, R] = frame_extent) s[h] = rint(lambda f_h dt (W-1) / (1000 R)) in float64, ``frame_interval`` dt in
    seconds, ``wavelength`` in metres.  Positive Doppler is closing: the range falls and w rises."""
    H, W = int(H), int(W)
    D, R = float(frame_extent[0]), float(frame_extent[1])
    dt, lam = float(frame_interval), float(wavelength)
    if H < 2 or W < 2:
        raise ValueError(f"H = {H}, W = {W}: the axes need at least two rows and two columns")
    if not (np.isfinite(D) and np.isfinite(R) and R != 0.0 and np.isfinite(dt) and np.isfinite(lam)):
        raise ValueError("frame_extent, frame_interval and wavelength must be finite, the range extent not zero")
    f = (H - 1 - 2 * np.arange(H, dtype=np.float64)) * D / (H - 1)
    s = np.rint(lam * f * dt * (W - 1) / (1000.0 * R))
    if np.abs(s).max() > 2**31 - 1:
        raise ValueError("a row shift does not fit int32")
    return s.astype(np.int32)


def _tbd_shifts_host(row_shifts, H):
    """int32 [H] on the host from whatever the caller passed (None stays None)"""
    if row_shifts is None:
        return None
    s = np.asarray(row_shifts.cpu() if hasattr(row_shifts, "cpu") else row_shifts)
    if s.shape != (H,) or s.dtype.kind not in "iu":
        raise ValueError(f"row_shifts must be {H} integers, one per Doppler row")
    if s.size and (s.min() < -2**31 or s.max() > 2**31 - 1):
        raise ValueError("a row shift does not fit int32")
    return np.ascontiguousarray(s, dtype=np.int32)


def _tbd_check_host(desc):
    """every argument check of prc_tbd, on the host (ValueError), before a device is touched"""
    check(lib().prc_tbd(C.byref(desc), None, None, None, 0, None, None, None))


def track_before_detect(stat, frame_extent=None, *, alpha=0.9, doppler_reach=1, range_reach=1, row_shifts=None, clip=None,
                        range_guard=8, doppler_guard=4, prev=None, return_back=True):
    """Track-before-detect (prc_tbd of include/prcore.h): the Viterbi integration of a stack of statistic frames.  Per cell
    and frame, score = z' + alpha max(score of the previous frame over the admissible predecessors): the cells within
    (``doppler_reach``, ``range_reach``) of the cell moved back by its row's entry of ``row_shifts`` (int32 [H], range columns
    per frame: tbd_row_shifts; None = no motion); z' is the statistic, 0 inside extract_plots' excluded zones
    (``range_guard``, ``doppler_guard``) and at most ``clip``.  ``back`` holds the chosen predecessor's code per cell (255: none):
    tbd_paths reads tracks back through it.  ``prev`` [H, W] is the score of the frame before the stack: passing a call's last
    score frame to the next call continues the stream exactly.  ``frame_extent`` is not needed (the shifts carry the geometry)
    and accepted only so that the call reads like extract_plots'.
    ``stat`` is a frame [H, W] or a stack [N, H, W] (H Doppler rows, W range columns), NumPy or a torch device tensor;
    returns ``(score, back)`` of stat's shape, float32 and uint8 (back None with ``return_back=False``): arrays for NumPy,
    tensors on the caller's device and torch's current stream for torch."""
    dev = _lib.is_device_tensor(stat)
    if dev:
        import torch
        t = stat.to(torch.float32).contiguous()
        shape = tuple(t.shape)
    else:
        t = np.ascontiguousarray(stat, dtype=np.float32)
        shape = t.shape
    if len(shape) not in (2, 3):
        raise ValueError("track_before_detect takes a frame [H, W] or a stack [nframes, H, W]")
    nframes, H, W = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    desc = engine.tbd_desc(H, W, alpha, doppler_reach, range_reach, clip, range_guard, doppler_guard)
    _tbd_check_host(desc)
    s = _tbd_shifts_host(row_shifts, H)
    if prev is not None and tuple(prev.shape) != (H, W):
        raise ValueError(f"prev has shape {tuple(prev.shape)}, a frame {(H, W)}")
    if dev:
        if prev is not None and not _lib.is_device_tensor(prev):
            raise ValueError("stat and prev are both NumPy arrays or both device tensors")
        ds = None if s is None else torch.from_numpy(s).to(t.device)
        dp = None if prev is None else prev.to(torch.float32).contiguous()
        score = torch.empty_like(t)
        back = torch.empty(shape, dtype=torch.uint8, device=t.device) if return_back else None
        if nframes:
            with torch.cuda.device(t.device):
                engine.tbd_execute(desc, t, ds, dp, nframes, score, back, _lib.torch_stream_ptr(t.device))
        return score, back
    _lib.require_gpu()
    n = nframes * H * W
    if n == 0:
        return np.zeros(shape, np.float32), (np.zeros(shape, np.uint8) if return_back else None)
    dx, dscore = _lib.DeviceBuffer(4 * n), _lib.DeviceBuffer(4 * n)
    dx.upload(t)
    dback = _lib.DeviceBuffer(n) if return_back else None
    ds = dp = None
    if s is not None:
        ds = _lib.DeviceBuffer(4 * H)
        ds.upload(s)
    if prev is not None:
        dp = _lib.DeviceBuffer(4 * H * W)
        dp.upload(np.ascontiguousarray(prev, dtype=np.float32))
    engine.tbd_execute(desc, dx, ds, dp, nframes, dscore, dback)
    return dscore.download(shape, np.float32), (dback.download(shape, np.uint8) if return_back else None)


def tbd_paths(back, ends, depth, row_shifts=None, *, doppler_reach=1, range_reach=1):
    """Read tracks back through track_before_detect's ``back`` [N, H, W] (prc_tbd_trace): ``ends`` [nends, 2] = (frame,
    storage cell h W + w); returns int32 [nends, depth]: column 0 the end's own cell, column j the cell in frame - j, -1 from
    where the path stops (no predecessor was chosen, the stack begins) and in the whole row of an end outside the stack.
    ``row_shifts`` and the reaches are those of the track_before_detect call.  NumPy in, NumPy out; torch device tensors in,
    a tensor on the same device and torch's current stream out."""
    dev = _lib.is_device_tensor(back)
    if len(back.shape) != 3:
        raise ValueError("back is a stack [nframes, H, W]")
    nframes, H, W = (int(v) for v in back.shape)
    depth = int(depth)
    if depth < 1:
        raise ValueError(f"depth = {depth}, not >= 1")
    desc = engine.tbd_desc(H, W, 1.0, doppler_reach, range_reach)
    _tbd_check_host(desc)
    s = _tbd_shifts_host(row_shifts, H)
    if dev:
        import torch
        b = back.to(torch.uint8).contiguous()
        e = torch.as_tensor(ends, device=b.device).to(torch.int32).contiguous()
        if e.dim() != 2 or e.shape[1] != 2:
            raise ValueError("ends is [nends, 2]: frame, cell")
        paths = torch.empty((e.shape[0], depth), dtype=torch.int32, device=b.device)
        ds = None if s is None else torch.from_numpy(s).to(b.device)
        if e.shape[0]:
            with torch.cuda.device(b.device):
                engine.tbd_trace(desc, b, ds, nframes, e, e.shape[0], depth, paths, _lib.torch_stream_ptr(b.device))
        return paths
    b = np.ascontiguousarray(back, dtype=np.uint8)
    e = np.ascontiguousarray(ends, dtype=np.int32)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError("ends is [nends, 2]: frame, cell")
    if e.shape[0] == 0:
        return np.zeros((0, depth), np.int32)
    _lib.require_gpu()
    db, de, dpaths = _lib.DeviceBuffer(b.nbytes), _lib.DeviceBuffer(e.nbytes), _lib.DeviceBuffer(4 * e.shape[0] * depth)
    db.upload(b)
    de.upload(e)
    ds = None
    if s is not None:
        ds = _lib.DeviceBuffer(4 * H)
        ds.upload(s)
    engine.tbd_trace(desc, db, ds, nframes, de, e.shape[0], depth, dpaths)
    return dpaths.download((e.shape[0], depth), np.int32)


def tbd_maps(xambg, frame_extent, frame_interval, wavelength, *, thresh, depth=16, fw=18, gw=4, cfar="os", cfar_rank=None,
             plot_connectivity=8, **tbd_kw):
    """CFAR -> track_before_detect -> extract_plots on the integrated score -> tbd_paths, stage after stage on the device:
    the multi-frame counterpart of ``track_maps(measure="plots")``'s first two stages.  ``xambg`` is a torch device tensor
    [N, H, W] or NumPy (H, W, Nframes) as track_maps takes it.  The CFAR is CFAR_2D_OS on the ``plain`` scale (``cfar="os"``)
    or CFAR_2D / CFAR_2D_abs (``"mean"``); the row shifts are tbd_row_shifts(H, W, frame_extent, frame_interval, wavelength)
    unless ``row_shifts`` is given; ``tbd_kw`` are track_before_detect's keywords.  The score stack is thresholded at
    ``thresh`` (calibrate it on noise: the integrated score has no closed-form threshold here) and clustered with the score
    as weight and the same guards; every plot's peak cell is the end of one path of ``depth`` cells.
    Returns ``(counts, meas, index, paths)``: the first three as extract_plots returns them for a stack, ``paths`` int32
    [N, capacity, depth] (tbd_paths' rows; -1 in the slots past counts[i])."""
    if cfar not in ("mean", "os"):
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")
    dev = _lib.is_device_tensor(xambg)
    if dev:
        import torch
        x = xambg if xambg.dim() == 3 else xambg.unsqueeze(0)
        x = x.to(torch.complex64 if x.is_complex() else torch.float32).contiguous()
    else:
        x = np.asarray(xambg)
        if x.ndim != 3:
            raise ValueError("tbd_maps takes (H, W, Nframes) frames")
        x = np.moveaxis(x, 2, 0)
    if len(x.shape) != 3:
        raise ValueError("tbd_maps takes a device stack [N, H, W]")
    N, H, W = (int(v) for v in x.shape)
    kw = dict(tbd_kw)
    bad = set(kw) - {"alpha", "doppler_reach", "range_reach", "row_shifts", "clip", "range_guard", "doppler_guard", "prev"}
    if bad:
        raise TypeError(f"tbd_maps: unexpected keyword(s) {sorted(bad)}")
    if kw.get("row_shifts") is None:
        kw["row_shifts"] = tbd_row_shifts(H, W, frame_extent, frame_interval, wavelength)
    guards = dict(range_guard=kw.get("range_guard", 8), doppler_guard=kw.get("doppler_guard", 4))
    _tbd_check_host(engine.tbd_desc(H, W, kw.get("alpha", 0.9), kw.get("doppler_reach", 1), kw.get("range_reach", 1),
                                    kw.get("clip"), **guards))
    _plots_check_host(H, W, float(thresh), frame_extent, plot_connectivity, guards["range_guard"], guards["doppler_guard"],
                      None, None, N)
    if cfar == "os":
        cf = CFAR_2D_OS(x, fw, gw, rank=cfar_rank, scale="plain")
    elif dev:
        cf = _chain_cfar(x, fw, gw, cfar, cfar_rank)
    else:
        cf = CFAR_2D_abs(x, fw, gw) if np.iscomplexobj(x) else CFAR_2D(x, fw, gw)
    score, back = track_before_detect(cf, frame_extent, **kw)
    counts, meas, index, info, _ = extract_plots(score, thresh, frame_extent, connectivity=plot_connectivity, return_info=True,
                                                 **guards)
    cap = int(index.shape[1])
    if dev:
        peak = info[:, :, 44:48].contiguous().view(torch.int32).view(N, cap)          # prc_plot_info.peak
        valid = torch.arange(cap, device=x.device)[None, :] < counts[:, None]
        frame = torch.arange(N, device=x.device, dtype=torch.int32)[:, None].expand(N, cap)
        ends = torch.stack((torch.where(valid, frame, -1), torch.where(valid, peak, -1)), dim=2).to(torch.int32)
    else:
        valid = np.arange(cap)[None, :] < counts[:, None]
        frame = np.broadcast_to(np.arange(N, dtype=np.int32)[:, None], (N, cap))
        ends = np.stack((np.where(valid, frame, -1), np.where(valid, info["peak"], -1)), axis=2).astype(np.int32)
    paths = tbd_paths(back, ends.reshape(N * cap, 2), depth, kw["row_shifts"], doppler_reach=kw.get("doppler_reach", 1),
                      range_reach=kw.get("range_reach", 1))
    return counts, meas, index, paths.reshape(N, cap, int(depth))


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
