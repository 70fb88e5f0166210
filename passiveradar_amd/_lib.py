"""ctypes binding of libprcore.so (include/prcore.h) -- the only way the package computes.

There is no CPU fallback: if the shared library is missing or no MI355X is visible the
functions raise.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C passiveradar_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRCORE_LIB", os.path.join(_HERE, "libprcore.so"))   # override: A/B kernel builds

PRC_OK, PRC_EINVAL, PRC_ESHAPE, PRC_EHIP, PRC_EROCFFT, PRC_EUNSUPPORTED = 0, -1, -2, -3, -4, -5
CAF_AUTO, CAF_DIRECT, CAF_FFT, CAF_FFT4096 = 0, 1, 2, 3
DOPPLER_AUTO, DOPPLER_ROCFFT, DOPPLER_COLUMN = 0, 1, 2
CAF_MULTI_AUTO, CAF_MULTI_TURNS, CAF_MULTI_SHARED, CAF_MULTI_PAIRS = 0, 1, 2, 3
CAF_MULTI_MODES = {"auto": CAF_MULTI_AUTO, "turns": CAF_MULTI_TURNS, "shared": CAF_MULTI_SHARED, "pairs": CAF_MULTI_PAIRS}
# prc_option
(OPT_CAF_MULTI_MODE, OPT_CAF_GROUP_MB, OPT_LS_TEAM_PIECES, OPT_LS_TEAM_ALIGN, OPT_NLMS_WAVES, OPT_LS_CACHE_LIMIT_MB,
 OPT_NLMS_WG_WAVES, OPT_CAF_XCD_CONTIG, OPT_CAF_PAIR_FRAMES, OPT_FE_METHOD,
 OPT_CFAR_METHOD, OPT_MARKERS, OPT_FE_BALANCE, OPT_CAF_TEAM8, OPT_FE_FOLD, OPT_TBD_FRAMES, OPT_TBD_ROWS,
 OPT_CHANNELIZE_FORM) = range(18)
CAF_MAX_REFS = 8
COMM_ID_BYTES = 128


class PrcoreError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libprcore error {code}: {msg}")
        self.code = code


DESC_MAGIC = 0x36435250      # PRC_DESC_MAGIC, "PRC6"


class _Desc(C.Structure):
    """Descriptor structs of include/prcore.h: the first field says how large the HOST's struct is (version 600), so the
    library never reads past it and takes fields the host does not know as 0."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))
        self.magic = DESC_MAGIC


class CafDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n", C.c_int64), ("range_bins", C.c_int32), ("freq_bins", C.c_int32),
                ("max_frames", C.c_int32), ("method", C.c_int32), ("doppler", C.c_int32),
                ("ntaps", C.c_int32), ("taps_host", C.POINTER(C.c_float)), ("multi", C.c_int32)]


class LsDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n", C.c_int64), ("filter_len", C.c_int32), ("peek", C.c_int32),
                ("circular", C.c_int32), ("max_blocks", C.c_int32), ("method", C.c_int32)]


class FrontendDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n_in", C.c_int64), ("raw_dtype", C.c_int32), ("up", C.c_int32), ("down", C.c_int32),
                ("ntaps", C.c_int32), ("n_pre_remove", C.c_int32), ("max_blocks", C.c_int32),
                ("taps_host", C.POINTER(C.c_float))]


class IirDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("q", C.c_int32), ("padlen", C.c_int32), ("settle", C.c_int32), ("nzeros", C.c_int32),
                ("npoles", C.c_int32), ("zeros_host", C.POINTER(C.c_double)),
                ("poles_host", C.POINTER(C.c_double)), ("gain", C.c_double)]


class TrackDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("H", C.c_int32), ("W", C.c_int32), ("ntracks", C.c_int32), ("capacity", C.c_int32),
                ("percentile", C.c_double), ("doppler_extent", C.c_double), ("range_extent", C.c_double)]


class TrackCand(C.Structure):
    _fields_ = [("strength", C.c_double), ("range", C.c_double), ("doppler", C.c_double), ("index", C.c_int64)]


class TrackRecord(C.Structure):
    _fields_ = [("status", C.c_int32), ("lifetime", C.c_int32), ("measurement", C.c_double * 2),
                ("estimate", C.c_double * 2), ("x", C.c_double * 4), ("P", C.c_double * 16), ("S", C.c_double * 4),
                ("history", C.c_uint8 * 20), ("overflow", C.c_int32)]


# NumPy views of prc_track_cand / prc_track_record (same layout as the ctypes mirrors)
TRACK_CAND_DTYPE = np.dtype([("strength", "<f8"), ("range", "<f8"), ("doppler", "<f8"), ("index", "<i8")])
TRACK_RECORD_DTYPE = np.dtype([("status", "<i4"), ("lifetime", "<i4"), ("measurement", "<f8", (2,)),
                               ("estimate", "<f8", (2,)), ("x", "<f8", (4,)), ("P", "<f8", (16,)), ("S", "<f8", (4,)),
                               ("history", "u1", (20,)), ("overflow", "<i4")])


class StrackDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("H", C.c_int32), ("W", C.c_int32), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("range_extent", C.c_double), ("doppler_extent", C.c_double)]


class StrackRecord(C.Structure):
    _fields_ = [("lock_mode", C.c_double * 4), ("measurement", C.c_double * 2), ("measurement_idx", C.c_int64 * 2),
                ("estimate", C.c_double * 2), ("x", C.c_double * 4), ("P", C.c_double * 16), ("S", C.c_double * 4)]


class WelchDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("nfft", C.c_int32), ("noverlap", C.c_int32), ("navg", C.c_int32), ("detrend", C.c_int32),
                ("in_dtype", C.c_int32), ("step", C.c_int32), ("scale", C.c_double)]


class FirdecDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("q", C.c_int32), ("ntaps", C.c_int32), ("raw_dtype", C.c_int32), ("mix", C.c_int32),
                ("fc", C.c_double), ("fs", C.c_double), ("phase_offset", C.c_double)]


class ChannelizeDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("nchan", C.c_int32), ("dec", C.c_int32), ("ntaps", C.c_int32), ("raw_dtype", C.c_int32),
                ("nsel", C.c_int32), ("reserved", C.c_int32), ("start", C.c_int64)]


class PatchDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n", C.c_int64), ("frame_stride", C.c_int64), ("nframes", C.c_int32), ("nlags", C.c_int32),
                ("ndoppler", C.c_int32), ("wrap", C.c_int32), ("sample_rate", C.c_double), ("doppler_step", C.c_double)]


class Patch(C.Structure):
    _fields_ = [("frame", C.c_int32), ("lag0", C.c_int32), ("doppler0", C.c_double)]


class PatchPeak(C.Structure):
    _fields_ = [("lag", C.c_double), ("doppler", C.c_double), ("amplitude", C.c_float), ("d", C.c_int32), ("l", C.c_int32),
                ("flags", C.c_uint32)]


# NumPy views of prc_patch / prc_patch_peak (same layout as the ctypes mirrors)
PATCH_DTYPE = np.dtype([("frame", "<i4"), ("lag0", "<i4"), ("doppler0", "<f8")])
PATCH_PEAK_DTYPE = np.dtype([("lag", "<f8"), ("doppler", "<f8"), ("amplitude", "<f4"), ("d", "<i4"), ("l", "<i4"),
                             ("flags", "<u4")])
PATCH_MAX_LAGS, PATCH_MAX_DOPPLER = 1024, 4096       # PRC_PATCH_MAX_LAGS, PRC_PATCH_MAX_DOPPLER
PATCH_EDGE_DOPPLER, PATCH_EDGE_LAG, PATCH_FLAT = 1, 2, 4   # prc_patch_peak.flags


class CfarOsDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("H", C.c_int32), ("W", C.c_int32), ("fw", C.c_int32), ("gw", C.c_int32), ("rank", C.c_int32),
                ("scale", C.c_int32), ("input", C.c_int32), ("use_thresh", C.c_int32), ("thresh", C.c_float)]


CFAR_SCALE_REFERENCE, CFAR_SCALE_PLAIN = 0, 1      # prc_cfar_scale
CFAR_SCALES = {"reference": CFAR_SCALE_REFERENCE, "plain": CFAR_SCALE_PLAIN}

class PlotsDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("H", C.c_int32), ("W", C.c_int32), ("connectivity", C.c_int32), ("range_guard", C.c_int32),
                ("doppler_guard", C.c_int32), ("max_cells", C.c_int32), ("capacity", C.c_int32), ("weight_input", C.c_int32),
                ("thresh", C.c_float), ("doppler_extent", C.c_double), ("range_extent", C.c_double)]


class PlotInfo(C.Structure):
    _fields_ = [("mass", C.c_double), ("hbar", C.c_double), ("wbar", C.c_double), ("ncells", C.c_int32), ("h0", C.c_int32),
                ("h1", C.c_int32), ("w0", C.c_int32), ("w1", C.c_int32), ("peak", C.c_int32)]


# NumPy view of prc_plot_info (same layout as the ctypes mirror)
PLOT_INFO_DTYPE = np.dtype([("mass", "<f8"), ("hbar", "<f8"), ("wbar", "<f8"), ("ncells", "<i4"), ("h0", "<i4"), ("h1", "<i4"),
                            ("w0", "<i4"), ("w1", "<i4"), ("peak", "<i4")])
PLOTS_LDS_CELLS = 4096       # PRC_PLOTS_LDS_CELLS: detections per frame prc_plots holds in LDS (above: the caller's workspace)


class TbdDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("H", C.c_int32), ("W", C.c_int32), ("doppler_reach", C.c_int32), ("range_reach", C.c_int32),
                ("range_guard", C.c_int32), ("doppler_guard", C.c_int32), ("alpha", C.c_float), ("clip", C.c_float)]


TBD_FRAMES, TBD_FRAMES_MAX = 8, 32      # PRC_TBD_FRAMES, PRC_TBD_FRAMES_MAX: frames per launch of prc_tbd's time-blocked form
TBD_LDS_BYTES = 159744                  # PRC_TBD_LDS_BYTES
TBD_NONE = 255                          # the back pointer of a cell without a predecessor


class FuseDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("nillum", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32),
                ("nvx", C.c_int32), ("nvy", C.c_int32), ("combine", C.c_int32), ("form", C.c_int32), ("reserved", C.c_int32),
                ("x0", C.c_double), ("dx", C.c_double), ("y0", C.c_double), ("dy", C.c_double), ("z", C.c_double),
                ("vx0", C.c_double), ("dvx", C.c_double), ("vy0", C.c_double), ("dvy", C.c_double), ("rx", C.c_double * 3)]


FUSE_MAX_ILLUM, FUSE_ILLUM_DOUBLES = 8, 9      # PRC_FUSE_MAX_ILLUM, PRC_FUSE_ILLUM_DOUBLES
FUSE_LDS_BYTES = 159744                        # PRC_FUSE_LDS_BYTES
FUSE_SUM, FUSE_MIN = 0, 1                      # prc_fuse_combine
FUSE_COMBINES = {"sum": FUSE_SUM, "min": FUSE_MIN}
FUSE_FORM_AUTO, FUSE_FORM_GLOBAL, FUSE_FORM_LDS = 0, 1, 2      # prc_fuse_form


class BatchXambgDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n", C.c_int64), ("start", C.c_int64), ("hop", C.c_int64), ("batch_len", C.c_int32), ("range_bins", C.c_int32),
                ("freq_bins", C.c_int32), ("filter", C.c_int32), ("floor", C.c_float), ("reserved", C.c_int32)]


BATCH_MATCHED, BATCH_RECIPROCAL = 0, 1                     # prc_batch_filter
BATCH_FILTERS = {"matched": BATCH_MATCHED, "reciprocal": BATCH_RECIPROCAL}
BATCH_LENGTHS = (1024, 4096)                               # batch_len prc_batch_xambg transforms
BATCH_FREQ_BINS = (256, 512, 1024, 2048, 4096)             # freq_bins the column Doppler kernel takes
BATCH_XAMBG_MAX_BATCHES = 2 ** 31 - 1                      # PRC_BATCH_XAMBG_MAX_BATCHES


class EchoDesc(_Desc):
    _fields_ = [("struct_size", C.c_uint32), ("magic", C.c_uint32),
                ("n", C.c_int64), ("frame_stride", C.c_int64), ("out_stride", C.c_int64), ("nframes", C.c_int32),
                ("max_atoms", C.c_int32), ("wrap", C.c_int32), ("ramp", C.c_int32), ("refine", C.c_int32), ("reserved", C.c_int32),
                ("sample_rate", C.c_double), ("reg", C.c_double)]


class EchoAtom(C.Structure):
    _fields_ = [("lag", C.c_int32), ("reserved", C.c_int32), ("doppler", C.c_double)]


class EchoFit(C.Structure):
    _fields_ = [("doppler", C.c_double), ("amp", C.c_double * 2), ("slope", C.c_double * 2), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


# NumPy views of prc_echo_atom / prc_echo_fit (same layout as the ctypes mirrors)
ECHO_ATOM_DTYPE = np.dtype([("lag", "<i4"), ("reserved", "<i4"), ("doppler", "<f8")])
ECHO_FIT_DTYPE = np.dtype([("doppler", "<f8"), ("amp", "<c16"), ("slope", "<c16"), ("flags", "<u4"), ("reserved", "<u4")])
ECHO_MAX_ATOMS, ECHO_MAX_REFINE = 32, 8                    # PRC_ECHO_MAX_ATOMS, PRC_ECHO_MAX_REFINE
ECHO_SKIPPED, ECHO_CLAMPED, ECHO_BROKE_DOWN = 1, 2, 4      # prc_echo_fit.flags

FIRDEC_TILE_MAX_Q = 59       # PRC_FIRDEC_TILE_MAX_Q: the last q of decimate's filter that runs the LDS-tile form
CHANNELIZE_MAX_CHAN, CHANNELIZE_MAX_SEL = 256, 64       # PRC_CHANNELIZE_MAX_CHAN, PRC_CHANNELIZE_MAX_SEL
CHANNELIZE_TILE_MAX_BYTES = 163840                      # PRC_CHANNELIZE_TILE_MAX_BYTES

# NumPy view of prc_strack_record (same layout as the ctypes mirror)
STRACK_RECORD_DTYPE = np.dtype([("lock_mode", "<f8", (4,)), ("measurement", "<f8", (2,)),
                                ("measurement_idx", "<i8", (2,)), ("estimate", "<f8", (2,)), ("x", "<f8", (4,)),
                                ("P", "<f8", (16,)), ("S", "<f8", (4,))])
REAL_F32, REAL_F64 = 0, 1          # prc_real_dtype
PERSISTENCE_TERMS_PER_LAUNCH = 256
DISPLAY_PLOT, DISPLAY_STORED = 0, 1   # prc_display_orient


MIN_LIB_VERSION = 680      # PRC_VERSION of include/prcore.h these ctypes declarations mirror

RAW_DTYPES = {"int8": 0, "uint8": 1, "int16": 2, "float32": 3, "complex64": 4}

_lib = None
_lib_lock = threading.Lock()

_SIGNATURES = {
    "prc_version": (C.c_int, []),
    "prc_last_error": (C.c_char_p, []),
    "prc_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "prc_set_device": (C.c_int, [C.c_int]),
    "prc_get_device": (C.c_int, [C.POINTER(C.c_int)]),
    "prc_mem_info": (C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "prc_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "prc_free": (C.c_int, [C.c_void_p]),
    "prc_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "prc_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "prc_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "prc_stream_sync": (C.c_int, [C.c_void_p]),
    "prc_set_option": (C.c_int, [C.c_int32, C.c_int64]),
    "prc_get_option": (C.c_int, [C.c_int32, C.POINTER(C.c_int64)]),
    "prc_caf_plan_multi_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "prc_caf_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CafDesc)]),
    "prc_caf_plan_destroy": (C.c_int, [C.c_void_p]),
    "prc_caf_plan_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int64)]),
    "prc_caf_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_caf_execute_multi": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64,
                                        C.c_int64, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p]),
    "prc_caf_execute_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_caf_execute_doppler": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_batch_xambg_workspace_bytes": (C.c_int, [C.POINTER(BatchXambgDesc), C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_batch_xambg": (C.c_int, [C.POINTER(BatchXambgDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p]),
    "prc_ofdm_timing": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_ls_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(LsDesc)]),
    "prc_ls_plan_destroy": (C.c_int, [C.c_void_p]),
    "prc_ls_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                 C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_int32, C.c_double,
                                 C.c_void_p, C.c_void_p]),
    "prc_ls_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "prc_ls_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "prc_nlms_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                   C.c_void_p]),
    "prc_gal_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_gal_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_float, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p]),
    "prc_ls_svd_workspace_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_ls_svd_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                     C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "prc_ls_svd_set_profiling": (C.c_int, [C.c_int32]),
    "prc_ls_svd_get_profile": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "prc_eca_workspace_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_eca_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double,
                                  C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_eca_set_profiling": (C.c_int, [C.c_int32]),
    "prc_eca_get_profile": (C.c_int, [C.POINTER(C.c_double)]),
    "prc_frontend_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(FrontendDesc)]),
    "prc_frontend_plan_destroy": (C.c_int, [C.c_void_p]),
    "prc_frontend_out_len": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "prc_frontend_execute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                       C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "prc_frontend_execute2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double,
                                        C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "prc_deinterleave": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "prc_frequency_shift_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                            C.c_double, C.c_void_p]),
    "prc_frequency_shift_phases": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                             C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_cfar2d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                             C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_cfar2d_c64": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                 C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_cfar_training_cells": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "prc_cfar_os_workspace_bytes": (C.c_int, [C.POINTER(CfarOsDesc), C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_cfar_os": (C.c_int, [C.POINTER(CfarOsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "prc_decimate_iir": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(IirDesc), C.c_void_p, C.c_void_p]),
    "prc_channel_offset": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(IirDesc), C.c_int64,
                                     C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
    "prc_xcorr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                            C.c_void_p]),
    "prc_frequency_shift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                      C.c_double, C.c_void_p]),
    "prc_track_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(TrackDesc)]),
    "prc_track_plan_destroy": (C.c_int, [C.c_void_p]),
    "prc_track_measure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_track_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "prc_plots_workspace_bytes": (C.c_int, [C.POINTER(PlotsDesc), C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_plots": (C.c_int, [C.POINTER(PlotsDesc), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p]),
    "prc_tbd": (C.c_int, [C.POINTER(TbdDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_tbd_trace": (C.c_int, [C.POINTER(TbdDesc), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                C.c_void_p]),
    "prc_fuse": (C.c_int, [C.POINTER(FuseDesc), C.POINTER(C.c_double), C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                           C.c_void_p, C.c_void_p]),
    "prc_strack_workspace_bytes": (C.c_int, [C.POINTER(StrackDesc), C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_strack_run": (C.c_int, [C.POINTER(StrackDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "prc_persistence": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_double, C.c_void_p, C.c_int32, C.c_void_p]),
    "prc_display_limits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p]),
    "prc_display_rgba": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p, C.c_void_p]),
    "prc_welch_rows": (C.c_int, [C.POINTER(WelchDesc), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "prc_welch_workspace_bytes": (C.c_int, [C.POINTER(WelchDesc), C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_welch": (C.c_int, [C.POINTER(WelchDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_fir_decimate": (C.c_int, [C.POINTER(FirdecDesc), C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                   C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "prc_shift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "prc_normalize_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "prc_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "prc_channelize": (C.c_int, [C.POINTER(ChannelizeDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_int64, C.c_void_p]),
    "prc_xambg_patch_workspace_bytes": (C.c_int, [C.POINTER(PatchDesc), C.c_int32, C.POINTER(C.c_size_t)]),
    "prc_xambg_patch": (C.c_int, [C.POINTER(PatchDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "prc_xambg_patch_peaks": (C.c_int, [C.POINTER(PatchDesc), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_echo_cancel_workspace_bytes": (C.c_int, [C.POINTER(EchoDesc), C.POINTER(C.c_size_t)]),
    "prc_echo_cancel": (C.c_int, [C.POINTER(EchoDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "prc_comm_unique_id": (C.c_int, [C.c_void_p]),
    "prc_comm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_int32]),
    "prc_comm_destroy": (C.c_int, [C.c_void_p]),
    "prc_comm_rccl_version": (C.c_int, [C.POINTER(C.c_int32)]),
    "prc_comm_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "prc_comm_loopback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "prc_gather_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.c_void_p,
                                    C.c_int32, C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 under
    torch/lib (same SONAMEs as /opt/rocm's).  Whichever copy is loaded first serves every later user of that
    SONAME: if libprcore pulled in /opt/rocm's first, a later ``import torch`` would run on a runtime it was not
    built with and report "No HIP GPUs are available".  So when torch is installed its copy is loaded first (without
    importing torch) -- the configuration every GPU test runs in.  Found by the fuzz run with two caller threads: one thread
    loading this library while another is half way through `import torch` used to take the "torch is already there" shortcut."""
    import importlib.util
    import sys
    # (no shortcut for "torch is in sys.modules": another thread may be in the middle of `import torch` -- the module is
    # registered before its libraries are loaded -- and loading an already loaded library again is a no-op)
    try:
        mod = sys.modules.get("torch")
        spec = getattr(mod, "__spec__", None) if mod is not None else importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load libprcore.so once; raise (never fall back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} is not built: run `make -C passiveradar_amd/csrc` (hipcc, gfx950). "
                    "passiveradar_amd has no CPU fallback.")
            _share_hip_runtime_with_torch()
            handle = C.CDLL(LIB_PATH)
            # a stale build next to newer Python would fail below with an AttributeError on the first missing symbol, or --
            # worse -- read descriptors of another layout: say what to do instead
            handle.prc_version.restype = C.c_int
            built = handle.prc_version()
            if built < MIN_LIB_VERSION:
                raise ImportError(f"{LIB_PATH} was built from prcore.h version {built}, this package needs >= "
                                  f"{MIN_LIB_VERSION} (descriptor layout with struct_size): rebuild it with "
                                  f"`make -C passiveradar_amd/csrc`")
            for name, (res, args) in _SIGNATURES.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError:
                    # entry points added without a layout change keep PRC_VERSION (prc_cfar_os): the symbol is the check
                    raise ImportError(f"{LIB_PATH} (prcore.h version {built}) has no {name}: it was built from an older "
                                      f"source tree; rebuild it with `make -C passiveradar_amd/csrc`") from None
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def check(rc):
    """Map a prc_status to the reference's error convention (PRC_ESHAPE -> ValueError)."""
    if rc == PRC_OK:
        return
    msg = lib().prc_last_error().decode("utf-8", "replace")
    if rc == PRC_ESHAPE:
        raise ValueError(msg)
    if rc == PRC_EINVAL:
        raise ValueError(msg)
    if rc == PRC_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise PrcoreError(rc, msg)


def device_count():
    n = C.c_int(0)
    rc = lib().prc_device_count(C.byref(n))
    return n.value if rc == PRC_OK else 0


def current_device():
    """the calling thread's current HIP device index (-1 without a GPU)"""
    d = C.c_int(-1)
    return d.value if lib().prc_get_device(C.byref(d)) == PRC_OK else -1


def set_option(option, value):
    """prc_set_option: process-wide tuning option (the library reads no environment variables); plans copy the options
    that concern them when they are created.  Returns the previous value."""
    old = get_option(option)
    check(lib().prc_set_option(int(option), int(value)))
    return old


def get_option(option):
    v = C.c_int64(0)
    check(lib().prc_get_option(int(option), C.byref(v)))
    return int(v.value)


def mem_info():
    """(free, total) bytes of the current device's memory (hipMemGetInfo)"""
    f, t = C.c_size_t(0), C.c_size_t(0)
    check(lib().prc_mem_info(C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def rccl_version():
    """ncclGetVersion of the RCCL bound by the gather (None when RCCL cannot be loaded)"""
    v = C.c_int32(0)
    return int(v.value) if lib().prc_comm_rccl_version(C.byref(v)) == PRC_OK else None


_gpu_seen = False


def require_gpu():
    """raise unless a ROCm device is visible (asked of the runtime until one was seen: it does not go away again)"""
    global _gpu_seen
    if not _gpu_seen:
        if device_count() < 1:
            raise PrcoreError(PRC_EHIP, "no ROCm device visible: " +
                              lib().prc_last_error().decode("utf-8", "replace"))
        _gpu_seen = True


class DeviceBuffer:
    """A hipMalloc'ed region owned by Python (library-side allocator, no torch needed)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().prc_malloc(C.byref(p), max(self.nbytes, 8)))
        self.ptr = p.value

    def upload(self, arr, offset_bytes=0, stream=None):
        arr = np.ascontiguousarray(arr)
        assert offset_bytes + arr.nbytes <= self.nbytes
        check(lib().prc_memcpy_h2d(self.ptr + offset_bytes, arr.ctypes.data, arr.nbytes, stream))
        check(lib().prc_stream_sync(stream))   # arr may be a temporary

    def zero(self, offset_bytes=0, nbytes=None, stream=None):
        nbytes = self.nbytes - offset_bytes if nbytes is None else nbytes
        check(lib().prc_memset(self.ptr + offset_bytes, 0, nbytes, stream))

    def download(self, shape, dtype, offset_bytes=0, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        check(lib().prc_memcpy_d2h(out.ctypes.data, self.ptr + offset_bytes, out.nbytes, stream))
        check(lib().prc_stream_sync(stream))
        return out

    def free(self):
        if getattr(self, "ptr", None):
            lib().prc_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def is_device_tensor(x):
    """torch CUDA/HIP tensor (zero-copy path) vs host array (staged through DeviceBuffer)."""
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def torch_stream_ptr(device=None):
    """hipStream_t of torch's current stream on ``device`` (default: the current device)"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
