"""Drop-ins for the reference's ``passiveRadar/target_detection.py``: ``CFAR_2D`` (:683-703), applied per frame to
``|xambg|`` by range_doppler_plot.py:56-57 (SURVEY 8f "next" #3), the multi-target Kalman tracker of
multitarget_kalman_tracker.py: ``get_measurements`` (:164-229) and ``multitarget_tracker`` (:455-537), plus
``track_maps``, that script's CFAR -> measure -> track chain (:44-63) in one device pass, and the single-target tracker
of simple_kalman_tracker.py: ``simple_target_tracker`` (:626-681), plus ``simple_track_maps``, its CFAR -> track
chain (:46-61).  Beyond the reference: ``CFAR_2D_OS``, the order-statistic CFAR on CFAR_2D's window (with
``cfar_training_cells`` and ``os_cfar_threshold``), which the chains take with ``cfar="os"``, ``refine_peaks``, and
``extract_plots``, the plot extractor between a CFAR map and the tracker (``track_maps(..., measure="plots")``), and
track-before-detect: ``track_before_detect`` (the Viterbi integration of a stack of CFAR maps along the paths the Doppler
rows allow, ``tbd_row_shifts``), ``tbd_paths`` and the chain ``tbd_maps``; and the fusion of several illuminators' maps on
a position-velocity grid: ``fuse_maps`` (with ``bistatic_axes`` and the forward model ``bistatic_cell``) and the chain
``locate_maps``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, engine, residence
from ._lib import check, lib

__all__ = ["CFAR_2D", "CFAR_2D_abs", "CFAR_2D_OS", "cfar_training_cells", "os_cfar_threshold", "get_measurements",
           "multitarget_tracker", "track_maps",
           "kalman_filter_dtype", "target_track_dtype", "simple_target_tracker", "simple_track_maps",
           "target_track_dtype_simple", "refine_peaks", "extract_plots", "tbd_row_shifts", "track_before_detect", "tbd_paths",
           "tbd_maps", "bistatic_axes", "bistatic_cell", "fuse_maps", "locate_maps"]


def _map_dtype(cplx):
    return np.complex64 if cplx else np.float32


def _cfar_mean(side, x, shape, cplx, fw, gw, thresh=None):
    """prc_cfar2d / prc_cfar2d_c64 of the resident frame or stack ``x``: the handle of the float32 map"""
    frames = 1 if len(shape) == 2 else shape[0]
    out = side.empty("cfar_o", shape, np.float32)
    fn = lib().prc_cfar2d_c64 if cplx else lib().prc_cfar2d
    with side.device():                            # launch on the data's device and, for torch, its current stream there
        check(fn(x.ptr, shape[-2], shape[-1], int(fw), int(gw), int(thresh is not None), float(thresh or 0.0), out.ptr, frames,
                 side.stream))
    return out


def _cfar_return(side, r, thresh):
    """CFAR_2D's return convention for the float32 map ``r``: float64 arrays / float32 tensors, boolean with a threshold"""
    if side.torch:
        return r.bool() if thresh is not None else r
    return r > 0.5 if thresh is not None else r.astype(np.float64)


def CFAR_2D(X, fw, gw, thresh=None):
    """Constant false alarm rate filter (same contract as target_detection.py:683-703): X is a 2-D
    (Doppler x range) magnitude map -- or a stack [nframes, H, W] / torch device tensor for batches;
    returns the CFAR ratio in float64 (boolean if ``thresh`` is given), like the reference."""
    side = residence.of(X)
    shape = residence.shape(X)
    out = _cfar_mean(side, side.put("cfar_x", X, np.float32), shape, False, fw, gw, thresh)
    return _cfar_return(side, side.result(out, shape, np.float32), thresh)


def CFAR_2D_abs(xambg, fw, gw, thresh=None):
    """``CFAR_2D(np.abs(xambg), fw, gw, thresh)`` -- the call of range_doppler_plot.py:56-57 -- in ONE kernel: the
    complex64 range-Doppler map (2-D, a stack [nframes, H, W], or torch device tensors of those shapes) goes in as it
    is and |X| is taken while the CFAR tiles are loaded, so the complex map is read once and no magnitude map is written.
    Same return convention as CFAR_2D."""
    side = residence.of(xambg)
    shape = residence.shape(xambg)
    if len(shape) not in (2, 3):
        raise ValueError("CFAR_2D_abs takes a 2-D map or a stack [nframes, H, W]")
    out = _cfar_mean(side, side.put("cfar_xc", xambg, np.complex64), shape, True, fw, gw, thresh)
    return _cfar_return(side, side.result(out, shape, np.float32), thresh)


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


def _cfar_os_plan(shape, cplx, fw, gw, thresh=None, rank=None, scale="reference"):
    """prc_cfar_os of a frame or a stack, as far as the host goes: (descriptor, frames, workspace bytes); every argument
    check (ValueError)"""
    frames = 1 if len(shape) == 2 else int(shape[0])
    desc = engine.cfar_os_desc(int(shape[-2]), int(shape[-1]), fw, gw, rank, scale, cplx, thresh)
    return desc, frames, engine.cfar_os_workspace_bytes(desc, max(frames, 1))


def _cfar_os(side, x, shape, plan, want_noise=False):
    """the resident ``x`` through prc_cfar_os as planned: the handles of the float32 map and of the noise map (or None)"""
    desc, frames, nws = plan
    out = side.empty("cfar_o", shape, np.float32)
    z = side.empty("cfar_z", shape, np.float32) if want_noise else None
    ws = side.scratch("cfar_ws", nws)
    with side.device():
        engine.cfar_os_execute(desc, x, out, z, frames, ws, side.stream)
    return out, z


def CFAR_2D_OS(X, fw, gw, thresh=None, *, rank=None, scale="reference", return_noise=False):
    """Order-statistic CFAR on CFAR_2D's window: the noise estimate z of a cell is the ``rank``-th smallest (1-based,
    default ceil(0.75 Nt)) of its Nt = cfar_training_cells(fw, gw) training cells, selected exactly, instead of their mean
    -- a few strong cells in the window (a second target, the clutter ridge, a sidelobe) leave it untouched.
    ``scale="reference"``: (X / mean|X|) / (z + 1e-10), CFAR_2D's own form, which the trackers and the render chain take
    unchanged; ``scale="plain"``: X / z, the ratio os_cfar_threshold's multiplier applies to.
    X is a 2-D map or a stack [nframes, H, W], NumPy or a torch device tensor, real or complex (|X| is taken on load, as
    CFAR_2D_abs does).  Returns as CFAR_2D: float64 from NumPy (bool with ``thresh``), float32 / bool tensors on the caller's
    device and stream for torch; with ``return_noise=True`` also the z map (float64 / float32)."""
    side = residence.of(X)
    shape = residence.shape(X)
    if len(shape) not in (2, 3):
        raise ValueError("CFAR_2D_OS takes a 2-D map or a stack [nframes, H, W]")
    cplx = residence.iscomplex(X)
    plan = _cfar_os_plan(shape, cplx, fw, gw, thresh, rank, scale)
    if plan[1] == 0:                               # no frames: nothing to launch, nothing to allocate
        out = z = side.nothing(shape, np.float32)
    else:
        out, z = _cfar_os(side, side.put("cfar_xc" if cplx else "cfar_x", X, _map_dtype(cplx)), shape, plan, return_noise)
        out, z = side.result(out, shape, np.float32), (side.result(z, shape, np.float32) if return_noise else None)
    out = _cfar_return(side, out, thresh)
    if not return_noise:
        return out
    return out, (z if side.torch else z.astype(np.float64))


def _check_cfar(cfar):
    if cfar not in ("mean", "os"):
        raise ValueError(f"cfar is 'mean' or 'os', not {cfar!r}")


def _chain_cfar(side, x, shape, cplx, fw, gw, cfar, cfar_rank, scale="reference"):
    """the CFAR stage of the chains on the resident stack ``x`` [nframes, H, W]: "mean" = CFAR_2D / CFAR_2D_abs, "os" =
    CFAR_2D_OS (``scale`` applies to it alone).  Returns the handle of the float32 maps."""
    _check_cfar(cfar)
    if cfar == "os":
        return _cfar_os(side, x, shape, _cfar_os_plan(shape, cplx, fw, gw, rank=cfar_rank, scale=scale))[0]
    return _cfar_mean(side, x, shape, cplx, fw, gw)


def _maps_stack(xambg, who, frame_ok=True):
    """what the chains take, as a stack [N, H, W] with its side and whether it is complex: a torch device tensor [N, H, W]
    (a frame [H, W] is a stack of one, where ``frame_ok``) or NumPy (H, W, Nframes) as the reference's scripts load it.  A chain holds its
    stages' buffers itself (not pooled): the front doors it calls use the pool."""
    side = residence.of(xambg, pooled=False)
    if side.torch:
        x = xambg.unsqueeze(0) if frame_ok and xambg.dim() == 2 else xambg
        if x.dim() != 3:
            raise ValueError(f"{who} takes a device stack [N, H, W]")
    else:
        x = np.asarray(xambg)
        if x.ndim != 3:
            raise ValueError(f"{who} takes (H, W, Nframes) frames")
        x = np.moveaxis(x, 2, 0)
    return side, x, residence.iscomplex(x)


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


def _frames_shape(shape):
    if len(shape) == 2:
        return 1, int(shape[0]), int(shape[1])
    if len(shape) == 3:
        return int(shape[0]), int(shape[1]), int(shape[2])
    raise ValueError("expected a frame [H, W] or a stack [nframes, H, W]")


class _Measured:
    """counts + candidate records of a resident stack of frames (``frames``: its handle, float32), measured with a plan whose
    capacity holds every frame's candidates: after one measure the counts are read, and if any exceeds the capacity the plan
    is rebuilt at the exact maximum and the stack measured again (a deterministic sizing step).  ``capacity`` pins the
    capacity (no rebuild: frames over it keep their first `capacity` candidates and the tracker flags them);
    ``start_capacity`` only replaces the first guess (default: expected_capacity)."""

    def __init__(self, side, frames, nframes, H, W, frame_extent, ntracks, percentile=TRACK_PERCENTILE, capacity=None,
                 start_capacity=None):
        self.side, self.frames, self.nframes = side, frames, nframes
        self.rebuilt = False
        cap = int(capacity or start_capacity or expected_capacity(H, W, percentile))
        with side.device():
            self.counts_buf = side.scratch("counts", 4 * max(nframes, 1))
            for attempt in range(2):
                self.plan = TrackPlan(H, W, ntracks, cap, frame_extent, percentile)
                self.cands_buf = side.scratch("cands", 32 * max(nframes, 1) * cap)
                self.plan.measure(frames.ptr, nframes, self.counts_buf.ptr, self.cands_buf.ptr, side.stream)
                self.counts = side.fetch(self.counts_buf, nframes, np.int32)
                need = int(self.counts.max()) if nframes else 0
                if need <= cap or capacity:
                    break
                cap = need
                self.rebuilt = True
        self.capacity = cap

    def candidates(self):
        return self.side.fetch(self.cands_buf, (self.nframes, self.capacity), _lib.TRACK_CAND_DTYPE)

    def run(self):
        side, ntracks = self.side, self.plan.ntracks
        with side.device():
            rec = side.scratch("records", 256 * max(self.nframes, 1) * ntracks)
            self.plan.run(self.counts_buf.ptr, self.cands_buf.ptr, self.nframes, rec.ptr, side.stream)
            return side.fetch(rec, (self.nframes, ntracks), _lib.TRACK_RECORD_DTYPE)


def _device_measure(x, frame_extent, ntracks=1, capacity=None, percentile=TRACK_PERCENTILE, start_capacity=None, side=None):
    """measure a 2-D frame or [nframes, H, W] stack: numpy (staged) or a torch device tensor (on its stream)"""
    side = side or residence.of(x, pooled=False)
    nframes, H, W = _frames_shape(residence.shape(x))
    return _Measured(side, side.put("frames", x, np.float32), nframes, H, W, frame_extent, ntracks, percentile, capacity,
                     start_capacity)


def _cands_to_meas(c, count):
    c = c[:count]
    return np.stack((c["range"], c["doppler"], c["strength"]))


def _cands_tensors(m):
    """(counts, meas, index) of a _Measured / _Plots on the torch side, as get_measurements documents them"""
    import torch
    N, cap = m.nframes, m.capacity
    raw = m.cands_buf.t[:32 * N * cap]
    meas = raw.view(torch.float64).view(N, cap, 4)[:, :, [1, 2, 0]].permute(0, 2, 1).contiguous()
    index = raw.view(torch.int64).view(N, cap, 4)[:, :, 3].contiguous()
    return m.counts_buf.t[:4 * N].view(torch.int32).clone(), meas, index


def get_measurements(dataFrame, p, frame_extent):
    """get_measurements (target_detection.py:164-229): candidate measurements of one range-Doppler frame (H Doppler rows
    x W range columns) as (3, M) float64 -- range, Doppler, strength, strongest first (ties: the later cell of the
    reference's fliplr(frame.T) order first).  ``p`` is ignored, as in the reference (always the 99.8th percentile).
    A torch device stack [N, H, W] returns ``(counts, meas, index)`` on the device instead: int32 [N], float64
    [N, 3, capacity] (range, Doppler, strength; entries past counts[i] unused) and int64 [N, capacity] flat indices."""
    side = residence.of(dataFrame, pooled=False)
    if not side.torch and np.ndim(dataFrame) != 2:
        raise ValueError("get_measurements takes one 2-D frame (a torch device stack for batches)")
    m = _device_measure(dataFrame, frame_extent, side=side)
    if side.torch:
        return _cands_tensors(m)
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
    side, x, _ = _maps_stack(data, "multitarget_tracker")
    m = _device_measure(x, frame_extent, int(N_TRACKS), side=side)
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
    if measure == "plots" and plot_thresh is None:
        raise ValueError("measure='plots' needs plot_thresh")
    _check_cfar(cfar)
    ntracks = int(N_TRACKS)
    side, x, cplx = _maps_stack(xambg, "track_maps")
    shape = nframes, H, W = tuple(int(v) for v in x.shape)
    plots = measure == "plots"
    if plots:
        _plots_check_host(H, W, float(plot_thresh), frame_extent, plot_connectivity, 8, 4, plot_max_cells, plot_capacity, nframes)
    xin = side.put("maps", x, _map_dtype(cplx))
    # with plots the order-statistic CFAR runs on the plain scale, and the maps themselves are the plots' weights
    cf = _chain_cfar(side, xin, shape, cplx, fw, gw, cfar, cfar_rank, "plain" if plots else "reference")
    if not plots:
        return _records_to_history(_Measured(side, cf, nframes, H, W, frame_extent, ntracks).run(), ntracks)
    m = _Plots(side, cf, xin, cplx, nframes, H, W, float(plot_thresh), frame_extent, connectivity=plot_connectivity,
               max_cells=plot_max_cells, capacity=plot_capacity)
    return _records_to_history(_plots_run_tracker(m, H, W, ntracks, frame_extent), ntracks)


# ---- plot extraction (beyond the reference) -------------------------------------------------------
PLOTS_DEFAULT_CAPACITY = 512


class _Plots:
    """counts + one prc_track_cand per plot of a resident stack of statistic frames (prc_plots; ``stat`` and ``weight`` are
    handles, weight may be None).  A bound left at
    None is sized from what the call reports, as _Measured sizes its capacity: after a run ncells / counts are read, and if
    a frame exceeded ``max_cells`` the stack is run again at the exact maximum (the workspace path if that is above
    PRC_PLOTS_LDS_CELLS); if then, or at first, a frame has more plots than ``capacity``, once more at that exact maximum
    (the plot count of a frame over max_cells is only known after the first re-run).  A pinned bound is never changed: the
    caller sees the overflow in ncells / counts.  ``start_max_cells`` / ``start_capacity`` only replace the first guesses."""

    def __init__(self, side, stat, weight, complex_weight, nframes, H, W, thresh, frame_extent, connectivity=8, range_guard=8,
                 doppler_guard=4, max_cells=None, capacity=None, want_info=False, start_max_cells=None, start_capacity=None):
        self.side, self.stat, self.weight, self.nframes = side, stat, weight, nframes
        mc = int(max_cells or start_max_cells or _lib.PLOTS_LDS_CELLS)
        cap = int(capacity or start_capacity or PLOTS_DEFAULT_CAPACITY)
        nf = max(nframes, 1)
        self.info_buf = None
        self.runs = 0
        with side.device():
            self.counts_buf = side.scratch("plot_counts", 4 * nf)
            self.ncells_buf = side.scratch("plot_ncells", 4 * nf)
            while True:
                desc = engine.plots_desc(H, W, thresh, frame_extent, connectivity, range_guard, doppler_guard, mc, cap,
                                         complex_weight)
                nws = engine.plots_workspace_bytes(desc, nframes)
                self.cands_buf = side.scratch("plot_cands", 32 * nf * cap)
                if want_info:
                    self.info_buf = side.scratch("plot_info", _lib.PLOT_INFO_DTYPE.itemsize * nf * cap)
                ws = side.scratch("plot_ws", nws)
                side.zero(self.cands_buf, 32 * nf * cap)                                     # slots past a count read as zeros
                if want_info:
                    side.zero(self.info_buf, _lib.PLOT_INFO_DTYPE.itemsize * nf * cap)
                engine.plots_execute(desc, stat, weight, nframes, self.counts_buf, self.ncells_buf, self.cands_buf, self.info_buf,
                                     ws, side.stream)
                self.runs += 1
                self.counts = side.fetch(self.counts_buf, nframes, np.int32)
                self.ncells = side.fetch(self.ncells_buf, nframes, np.int32)
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
        return self.side.fetch(self.cands_buf, (self.nframes, self.capacity), _lib.TRACK_CAND_DTYPE)

    def info(self):
        return self.side.fetch(self.info_buf, (self.nframes, self.capacity), _lib.PLOT_INFO_DTYPE)


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
    side = residence.of(stat, weight, pooled=False, mixed="stat and weight are both NumPy arrays or both device tensors")
    shape = residence.shape(stat)
    wshape = None if weight is None else residence.shape(weight)
    cplx = weight is not None and residence.iscomplex(weight)
    if len(shape) not in (2, 3):
        raise ValueError("extract_plots takes a frame [H, W] or a stack [nframes, H, W]")
    if wshape is not None and wshape != shape:
        raise ValueError(f"weight has shape {wshape}, stat {shape}")
    nframes, H, W = _frames_shape(shape)
    _plots_check_host(H, W, thresh, frame_extent, kw.get("connectivity", 8), kw.get("range_guard", 8),
                      kw.get("doppler_guard", 4), kw.get("max_cells"), kw.get("capacity"), nframes)
    t = side.put("stat", stat, np.float32)
    w = None if weight is None else side.put("weight", weight, _map_dtype(cplx))
    return _Plots(side, t, w, cplx, nframes, H, W, thresh, frame_extent, **kw)


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
    if m.side.torch:
        import torch
        out = _cands_tensors(m)
        if not return_info:
            return out
        nb = _lib.PLOT_INFO_DTYPE.itemsize
        return out + (m.info_buf.t[:nb * N * cap].view(N, cap, nb).clone(), m.ncells_buf.t[:4 * N].view(torch.int32).clone())
    c = m.candidates()
    if len(np.shape(stat)) == 2:
        k = int(m.stored()[0])
        meas = _cands_to_meas(c[0], k)
        return (meas, m.info()[0][:k], int(m.ncells[0])) if return_info else meas
    meas = np.ascontiguousarray(np.stack((c["range"], c["doppler"], c["strength"]), axis=1))
    out = (m.counts, meas, np.ascontiguousarray(c["index"]))
    return out + (m.info(), m.ncells) if return_info else out


def _plots_run_tracker(m, H, W, ntracks, frame_extent):
    """prc_track_run on the plots of ``m``, on its side"""
    if (m.ncells > m.max_cells).any():
        raise _lib.PrcoreError(_lib.PRC_EINVAL, "track_maps: a frame's detections exceeded plot_max_cells")
    side = m.side
    with side.device():
        plan = TrackPlan(H, W, ntracks, m.capacity, frame_extent)
        rec = side.scratch("records", 256 * max(m.nframes, 1) * ntracks)
        plan.run(m.counts_buf.ptr, m.cands_buf.ptr, m.nframes, rec.ptr, side.stream)
        out = side.fetch(rec, (m.nframes, ntracks), _lib.TRACK_RECORD_DTYPE)
    plan.close()
    return out


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
    shape = residence.shape(stat)
    if len(shape) not in (2, 3):
        raise ValueError("track_before_detect takes a frame [H, W] or a stack [nframes, H, W]")
    nframes, H, W = _frames_shape(shape)
    desc = engine.tbd_desc(H, W, alpha, doppler_reach, range_reach, clip, range_guard, doppler_guard)
    _tbd_check_host(desc)
    s = _tbd_shifts_host(row_shifts, H)
    if prev is not None and tuple(prev.shape) != (H, W):
        raise ValueError(f"prev has shape {tuple(prev.shape)}, a frame {(H, W)}")
    side = residence.of(stat, prev, pooled=False, mixed="stat and prev are both NumPy arrays or both device tensors")
    if nframes == 0:
        return side.nothing(shape, np.float32), (side.nothing(shape, np.uint8) if return_back else None)
    x = side.put("stat", stat, np.float32)
    ds = None if s is None else side.put("shifts", s, np.int32)
    dp = None if prev is None else side.put("prev", prev, np.float32)
    score = side.empty("score", shape, np.float32)
    back = side.empty("back", shape, np.uint8) if return_back else None
    with side.device():
        engine.tbd_execute(desc, x, ds, dp, nframes, score, back, side.stream)
    return side.result(score, shape, np.float32), (side.result(back, shape, np.uint8) if return_back else None)


def tbd_paths(back, ends, depth, row_shifts=None, *, doppler_reach=1, range_reach=1):
    """Read tracks back through track_before_detect's ``back`` [N, H, W] (prc_tbd_trace): ``ends`` [nends, 2] = (frame,
    storage cell h W + w); returns int32 [nends, depth]: column 0 the end's own cell, column j the cell in frame - j, -1 from
    where the path stops (no predecessor was chosen, the stack begins) and in the whole row of an end outside the stack.
    ``row_shifts`` and the reaches are those of the track_before_detect call.  NumPy in, NumPy out; torch device tensors in,
    a tensor on the same device and torch's current stream out."""
    if len(back.shape) != 3:
        raise ValueError("back is a stack [nframes, H, W]")
    nframes, H, W = (int(v) for v in back.shape)
    depth = int(depth)
    if depth < 1:
        raise ValueError(f"depth = {depth}, not >= 1")
    desc = engine.tbd_desc(H, W, 1.0, doppler_reach, range_reach)
    _tbd_check_host(desc)
    s = _tbd_shifts_host(row_shifts, H)
    eshape = residence.shape(ends)
    if len(eshape) != 2 or eshape[1] != 2:
        raise ValueError("ends is [nends, 2]: frame, cell")
    nends = int(eshape[0])
    side = residence.of(back, pooled=False)
    if nends == 0:
        return side.nothing((0, depth), np.int32)
    b = side.put("back", back, np.uint8)
    e = side.put("ends", ends if hasattr(ends, "shape") else np.asarray(ends), np.int32)
    ds = None if s is None else side.put("shifts", s, np.int32)
    paths = side.empty("paths", (nends, depth), np.int32)
    with side.device():
        engine.tbd_trace(desc, b, ds, nframes, e, nends, depth, paths, side.stream)
    return side.result(paths, (nends, depth), np.int32)


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
    _check_cfar(cfar)
    side, x, cplx = _maps_stack(xambg, "tbd_maps")
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
    # the stages are the front doors themselves: each returns what the next takes, on the side the maps came from
    if cfar == "os":
        cf = CFAR_2D_OS(x, fw, gw, rank=cfar_rank, scale="plain")
    else:
        cf = CFAR_2D_abs(x, fw, gw) if cplx else CFAR_2D(x, fw, gw)
    score, back = track_before_detect(cf, frame_extent, **kw)
    counts, meas, index, info, _ = extract_plots(score, thresh, frame_extent, connectivity=plot_connectivity, return_info=True,
                                                 **guards)
    cap = int(index.shape[1])
    if side.torch:
        import torch
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


# ---- fusion of several illuminators' maps on a position-velocity grid (beyond the reference) --------
SPEED_OF_LIGHT = 299792458.0


def bistatic_axes(rangeBins, freqBins, n, sampleRate):
    """``(col0, col_per_m, row0, row_per_hz)`` of a fast_xambg surface: an echo with ``r`` metres of excess bistatic range and
    ``f`` Hz of Doppler lands in column ``col0 + r col_per_m`` and row ``row0 + f row_per_hz``.  col = R - lag and
    row = F/2 - f CPI (the inverse of scene.expected_peak_cell): col0 = R, col_per_m = -fs/c, row0 = F/2, row_per_hz = -n/fs."""
    fs = float(sampleRate)
    return float(rangeBins), -fs / SPEED_OF_LIGHT, float(freqBins) / 2.0, -float(n) / fs


def _fuse_baseline(tx, rx):
    """|tx - rx| in float64, summed as prc_fuse sums a distance"""
    a = [np.float64(tx[i]) - np.float64(rx[i]) for i in range(3)]
    return float(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))


def bistatic_cell(position, velocity, tx, rx, wavelength, axes):
    """The forward model of prc_fuse in float64, operation for operation: the ``(row, col)`` (integers, not clipped to the
    map) in which an echo of a target at ``position`` (x, y, z) moving at ``velocity`` (vx, vy; no vertical component) lands
    on the surface of the illuminator at ``tx`` seen from ``rx``, ``axes`` = (col0, col_per_m, row0, row_per_hz)."""
    f8 = np.float64
    p, t, r = [f8(v) for v in position], [f8(v) for v in tx], [f8(v) for v in rx]
    vx, vy, lam = f8(velocity[0]), f8(velocity[1]), f8(wavelength)
    col0, col_per_m, row0, row_per_hz = (f8(v) for v in axes)
    at, ar = [p[i] - t[i] for i in range(3)], [p[i] - r[i] for i in range(3)]
    dt = np.sqrt((at[0] * at[0] + at[1] * at[1]) + at[2] * at[2])
    dr = np.sqrt((ar[0] * ar[0] + ar[1] * ar[1]) + ar[2] * ar[2])
    col = np.rint(col0 + ((dt + dr) - f8(_fuse_baseline(tx, rx))) * col_per_m)

    def quot(a, d):
        return f8(0.0) if d == 0.0 else a / d

    gx = (quot(at[0], dt) + quot(ar[0], dr)) / lam
    gy = (quot(at[1], dt) + quot(ar[1], dr)) / lam
    f = -(gx * vx + gy * vy)
    return int(np.rint(row0 + f * row_per_hz)), int(col)


def _fuse_illum(illuminators, rx):
    """the host array [K, 9] of prc_fuse from ``(tx, wavelength, axes)`` triples: the baseline is computed here"""
    rows = []
    for tx, wavelength, axes in illuminators:
        if len(tx) != 3 or len(axes) != 4:
            raise ValueError("an illuminator is (tx[3], wavelength, (col0, col_per_m, row0, row_per_hz))")
        rows.append([float(tx[0]), float(tx[1]), float(tx[2]), float(wavelength), _fuse_baseline(tx, rx)] + [float(v) for v in axes])
    return np.array(rows, dtype=np.float64).reshape(len(rows), _lib.FUSE_ILLUM_DOUBLES)


def _fuse_strides_ok(HW, K, s_illum, nframes, s_frame):
    """prc_fuse's condition on the two strides: no two of the K x nframes maps overlap"""
    if (K > 1 and s_illum < HW) or (nframes > 1 and s_frame < HW):
        return False
    if K == 1 or nframes == 1:
        return True
    return s_illum >= s_frame * (nframes - 1) + HW or s_frame >= s_illum * (K - 1) + HW


def fuse_maps(stat, illuminators, rx, grid, velocities, z=0.0, combine="sum", form=None, return_vel=True):
    """Non-coherent fusion of K illuminators' maps on a position-velocity grid (prc_fuse of include/prcore.h): per position
    cell (iy, ix) at (x0 + ix dx, y0 + iy dy, z) and velocity hypothesis j = jy nvx + jx at (vx0 + jx dvx, vy0 + jy dvy) the
    cell each illuminator's map would show that target in is read, the K samples are added (``combine="sum"``) or their
    minimum is taken (``"min"``), and per position cell the best score over the hypotheses and its j are kept.
    ``stat`` is [K, nframes, H, W] (or a list of K stacks [nframes, H, W]), float32 CFAR maps or any statistic, NumPy or a
    torch device tensor; ``illuminators`` a sequence of K ``(tx, wavelength, axes)`` with ``axes`` as bistatic_axes returns
    them; ``rx`` the receiver; ``grid`` = (x0, dx, nx, y0, dy, ny); ``velocities`` = (vx0, dvx, nvx, vy0, dvy, nvy).
    Returns ``(best, vel)``, float32 and int32 [nframes, ny, nx] (vel None with ``return_vel=False``): arrays for NumPy, tensors
    on the caller's device and torch's current stream for torch.  A device tensor whose maps are dense and do not overlap is
    read in place through its two leading strides, whatever they are; any other is copied first.  ``form``: None = the
    shipped kernel choice, 1 = gathers from global memory, 2 = gathers from LDS where a tile's columns fit."""
    if combine not in _lib.FUSE_COMBINES:
        raise ValueError(f"combine is 'sum' or 'min', not {combine!r}")
    if isinstance(stat, (list, tuple)):
        side = residence.of(stat[0], *stat[1:], pooled=False, mixed="the stacks are all NumPy arrays or all device tensors")
        if side.torch:
            import torch
            stat = torch.stack([s.to(torch.float32) for s in stat])
        else:
            stat = np.stack([np.asarray(s, dtype=np.float32) for s in stat])
    else:
        side = residence.of(stat, pooled=False)
    shape = residence.shape(stat)
    if len(shape) != 4:
        raise ValueError("fuse_maps takes [K, nframes, H, W] maps or a list of K stacks [nframes, H, W]")
    K, nframes, H, W = (int(v) for v in shape)
    if K != len(illuminators):
        raise ValueError(f"{K} stacks of maps, {len(illuminators)} illuminators")
    if len(rx) != 3 or len(grid) != 6 or len(velocities) != 6:
        raise ValueError("rx is (x, y, z), grid (x0, dx, nx, y0, dy, ny), velocities (vx0, dvx, nvx, vy0, dvy, nvy)")
    desc = engine.fuse_desc(K, H, W, grid, velocities, rx, z, _lib.FUSE_COMBINES[combine], form)
    illum = _fuse_illum(illuminators, rx)
    s_illum, s_frame = max(nframes, 1) * H * W, H * W
    if side.torch and residence.dtype_name(stat) == "float32" and stat.numel():
        st = stat.stride()
        if st[3] == 1 and st[2] == W and _fuse_strides_ok(H * W, K, st[0], nframes, st[1]):
            s_illum, s_frame = int(st[0]), int(st[1])
        else:
            stat = stat.contiguous()
    # every argument check of prc_fuse, on the host (ValueError), before a device is touched
    engine.fuse_execute(desc, illum, None, s_illum, s_frame, 0, None, None)
    oshape = (nframes, desc.ny, desc.nx)
    if nframes == 0:
        return side.nothing(oshape, np.float32), (side.nothing(oshape, np.int32) if return_vel else None)
    if side.torch and residence.dtype_name(stat) == "float32":
        x = residence._TorchBuf(stat)              # in place: the strides say where the maps are
    else:
        x = side.put("stat", stat, np.float32)
    best = side.empty("best", oshape, np.float32)
    vel = side.empty("vel", oshape, np.int32) if return_vel else None
    with side.device():
        engine.fuse_execute(desc, illum, x, s_illum, s_frame, nframes, best, vel, side.stream)
    return side.result(best, oshape, np.float32), (side.result(vel, oshape, np.int32) if return_vel else None)


def locate_maps(xambg_list, illuminators, rx, grid, velocities, z=0.0, *, thresh, npeaks, fw=18, gw=4, cfar="os", cfar_rank=None,
                combine="sum", form=None):
    """CFAR each illuminator's stack -> fuse_maps -> the ``npeaks`` strongest cells of ``best`` per frame above ``thresh``:
    where the targets of a multi-illuminator frame are and how they move.  ``xambg_list`` holds one stack per illuminator as
    the chains take them (a torch device tensor [N, H, W] or NumPy (H, W, Nframes), complex surfaces or magnitudes); the CFAR
    is CFAR_2D_OS on the ``plain`` scale (``cfar="os"``) or CFAR_2D / CFAR_2D_abs (``"mean"``); the other arguments are
    fuse_maps'.  Returns ``(position, velocity, score)``: float64 [N, npeaks, 2] (x, y), float64 [N, npeaks, 2] (vx, vy) and
    float32 [N, npeaks], strongest first; a slot whose cell is not above ``thresh`` (or that the grid has no cell for) holds
    NaN, NaN and -Inf.  Arrays for NumPy, tensors on the caller's device for torch (the peaks are picked by torch.topk there)."""
    _check_cfar(cfar)
    npeaks, thresh = int(npeaks), float(thresh)
    if npeaks < 1:
        raise ValueError(f"npeaks = {npeaks}, not >= 1")
    if len(xambg_list) != len(illuminators):
        raise ValueError(f"{len(xambg_list)} stacks of maps, {len(illuminators)} illuminators")
    maps = []
    for xambg in xambg_list:
        side, x, cplx = _maps_stack(xambg, "locate_maps")
        if cfar == "os":
            cf = CFAR_2D_OS(x, fw, gw, rank=cfar_rank, scale="plain")
        else:
            cf = CFAR_2D_abs(x, fw, gw) if cplx else CFAR_2D(x, fw, gw)
        maps.append(cf)
    best, vel = fuse_maps(maps, illuminators, rx, grid, velocities, z, combine, form)
    x0, dx, nx, y0, dy, ny = float(grid[0]), float(grid[1]), int(grid[2]), float(grid[3]), float(grid[4]), int(grid[5])
    vx0, dvx, nvx, vy0, dvy = float(velocities[0]), float(velocities[1]), int(velocities[2]), float(velocities[3]), float(velocities[4])
    N, k = int(best.shape[0]), min(npeaks, nx * ny)
    if side.torch:
        import torch
        score, cell = torch.topk(best.reshape(N, nx * ny), k, dim=1)
        j = torch.gather(vel.reshape(N, nx * ny), 1, cell).to(torch.int64)
        pad, stack, where, f8 = (lambda t, v: torch.nn.functional.pad(t, (0, npeaks - k), value=v)), torch.stack, torch.where, torch.float64
        cell, j, score = pad(cell, 0), pad(j, 0), pad(score, float("-inf"))
        iy, ix, jy, jx = cell // nx, cell % nx, j // nvx, j % nvx
        ok = score > thresh
        nan = torch.full_like(score, float("nan"), dtype=f8)
        ninf = torch.full_like(score, float("-inf"))
        ix, iy, jx, jy = ix.to(f8), iy.to(f8), jx.to(f8), jy.to(f8)
    else:
        flat = best.reshape(N, nx * ny)
        order = np.argsort(-np.where(np.isnan(flat), -np.inf, flat), axis=1, kind="stable")[:, :k]
        score = np.take_along_axis(flat, order, axis=1)
        j = np.take_along_axis(vel.reshape(N, nx * ny), order, axis=1).astype(np.int64)
        pad, stack, where, f8 = (lambda t, v: np.pad(t, ((0, 0), (0, npeaks - k)), constant_values=v)), np.stack, np.where, np.float64
        cell, j, score = pad(order, 0), pad(j, 0), pad(score, -np.inf)
        iy, ix, jy, jx = cell // nx, cell % nx, j // nvx, j % nvx
        ok = score > thresh
        nan = np.full(score.shape, np.nan)
        ninf = np.full(score.shape, -np.inf, dtype=np.float32)
    position = stack((where(ok, x0 + ix * dx, nan), where(ok, y0 + iy * dy, nan)), 2)
    velocity = stack((where(ok, vx0 + jx * dvx, nan), where(ok, vy0 + jy * dvy, nan)), 2)
    return position, velocity, where(ok, score, ninf)


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


def _strack_run(side, frames, nframes, H, W, dtype, range_extent, doppler_extent, state=None):
    """prc_strack_run on the resident frames [nframes][H][W] (``frames``: their handle; ``state``: a prc_strack_record to
    resume from); returns the history"""
    d = _strack_desc(H, W, dtype, range_extent, doppler_extent)
    nb = C.c_size_t(0)
    check(lib().prc_strack_workspace_bytes(C.byref(d), int(nframes), C.byref(nb)))
    with side.device():
        ws = side.scratch("strack_ws", nb.value)                               # no bytes only for no frames
        rec = side.scratch("strack_rec", _lib.STRACK_RECORD_DTYPE.itemsize * max(nframes, 1))
        st = None if state is None else side.put("strack_state", state.view(np.uint8), np.uint8)
        check(lib().prc_strack_run(C.byref(d), frames.ptr, int(nframes), engine._ptr(st), rec.ptr, engine._ptr(ws), side.stream))
        out = side.fetch(rec, nframes, _lib.STRACK_RECORD_DTYPE)
    return _strack_records_to_history(out, range_extent, doppler_extent)


def simple_target_tracker(data, rangeExtent, dopplerExtent, *, state=None):
    """simple_target_tracker (target_detection.py:626-681): ``data`` is numpy (H Doppler, W range, Nframes) as the
    reference takes it (float32 stays float32, anything else becomes float64), or a torch device tensor [N, H, W] of
    float32 / float64.  Returns the reference's (Nframes,) history of target_track_dtype_simple, computed as the
    reference does on the frames as float64 (a float64 frame may differ only where the reference's own division by the
    frame mean merges two values within about one ulp).  ``state=`` (the one extension) is a history row -- the last
    one of an earlier call -- to resume from; without it the track starts from the reference's initial state."""
    side, x, _ = _maps_stack(data, "simple_target_tracker", frame_ok=False)
    N, H, W = (int(v) for v in x.shape)
    f32 = residence.dtype_name(x) == "float32"
    state = None if state is None else _strack_state_record(state)
    frames = side.put("frames", x, np.float32 if f32 else np.float64)
    return _strack_run(side, frames, N, H, W, _lib.REAL_F32 if f32 else _lib.REAL_F64, rangeExtent, dopplerExtent, state)


def simple_track_maps(xambg, rangeExtent, dopplerExtent, fw=18, gw=4, cfar="mean", cfar_rank=None):
    """simple_kalman_tracker.py:46-61 as one device chain on the caller's stream: CFAR_2D(|xambg|, fw, gw) per frame
    (CFAR_2D_abs; CFAR_2D for a real magnitude stack) -> simple_target_tracker on the float32 CFAR maps.  ``xambg`` is
    a torch device tensor [N, H, W] or numpy (H, W, Nframes) as the script loads it.  ``cfar="os"`` puts CFAR_2D_OS
    (reference scale, rank ``cfar_rank``) in the cell average's place."""
    _check_cfar(cfar)
    side, x, cplx = _maps_stack(xambg, "simple_track_maps")
    shape = N, H, W = tuple(int(v) for v in x.shape)
    cf = _chain_cfar(side, side.put("maps", x, _map_dtype(cplx)), shape, cplx, fw, gw, cfar, cfar_rank)
    return _strack_run(side, cf, N, H, W, _lib.REAL_F32, rangeExtent, dopplerExtent)


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
    side = residence.of(X)
    nb = _lib.PATCH_PEAK_DTYPE.itemsize
    if npatches == 0:
        raw = side.nothing((0, nb), np.uint8)
    else:
        x = side.put("xp_out", X, np.complex64)
        d_rec = side.put("xp_rec", rec.view(np.uint8), np.uint8)
        peaks = side.empty("xp_peaks", (npatches, nb), np.uint8)
        with side.device():
            engine.xambg_patch_peaks(desc, d_rec, npatches, x, peaks, side.stream)
        raw = side.result(peaks, (npatches, nb), np.uint8)
    if not side.torch:
        return raw.view(_lib.PATCH_PEAK_DTYPE).reshape(npatches)
    import torch
    f64, f32, i32 = raw.view(torch.float64), raw.view(torch.float32), raw.view(torch.int32)
    return {"lag": f64[:, 0], "doppler": f64[:, 1], "amplitude": f32[:, 4], "d": i32[:, 5], "l": i32[:, 6],
            "flags": i32[:, 7]}
