/*
 * prcore.h -- C ABI of libprcore.so, the MI355X (gfx950) range-Doppler core.
 *
 * The reference (Max-Manning/passiveRadar) is pure Python and has no FFI layer; its
 * boundary for this path is the Python function level.  Each entry
 * point below replaces one reference function (or the SciPy/NumPy sequence inside it) and
 * is what a reference-side ctypes stub binds (INTEGRATION.md shows the stubs).  Citations
 * are file:line in the reference checkout.
 *
 * Conventions
 *   - extern "C", plain ints / pointers / POD structs; no C++ types, no exceptions cross.
 *   - complex64 samples are interleaved float pairs (re, im): `const void*` to 8-byte items.
 *   - all data pointers are DEVICE pointers unless the name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Work is enqueued
 *     asynchronously; nothing synchronises unless stated.
 *   - caller owns inputs and outputs; the library owns plans and their workspaces.
 *   - HOST arrays (names ending in `_host`) are read before the call returns and never afterwards: temporaries are fine.
 *   - every function returns PRC_OK (0) or a negative prc_status; prc_last_error() gives a
 *     thread-local message.  The Python layer maps PRC_ESHAPE to ValueError to keep the
 *     reference's error convention (range_doppler_processing.py:46-49, clutter_removal.py:28-29).
 *   - a plan may be used by one thread at a time (internally serialised by a mutex);
 *     different plans may be used concurrently from different threads (dask-style callers).
 *   - descriptors: every descriptor struct starts with `uint32_t struct_size`, which the host sets to sizeof(the
 *     struct) of the header IT was compiled against (ctypes: ctypes.sizeof), and `uint32_t magic` = PRC_DESC_MAGIC
 *     (PRC_DESC_INIT(d) zeroes a descriptor and sets both).  Descriptors only ever grow at the end.  The library reads
 *     min(struct_size, its own sizeof) bytes and takes fields the host did not know as 0 (= AUTO / default).  A wrong
 *     magic (a host built against a pre-600 header has the first field of the old layout there), a struct_size below
 *     the version-600 layout or not a multiple of 4 is PRC_EINVAL with a message naming the sizes -- a host built
 *     against another layout can never make the library read past its struct.
 *   - memory: an entry point reads block / frame / stream b of an input only inside [b*stride, b*stride + extent) elements
 *     -- and a CAF frame only below n_valid -- and writes only inside the documented extents of its outputs: what lies
 *     before the first block, between two blocks or after the last one is neither used in a result nor changed.  Data
 *     pointers need only the alignment of their element type (complex64: 8 bytes, int8 raw: any address).  No result
 *     depends on what a plan, a caller's workspace or the library's scratch was used for before
 *     (tests/test_gpu_bounds.py holds every single-rank device entry point to this; tests/test_gpu_display.py the
 *     two display entry points, tests/test_gpu_psd.py prc_welch, tests/test_gpu_preproc.py prc_fir_decimate, prc_shift and
 *     prc_normalize, tests/test_gpu_patch_bounds.py prc_xambg_patch and prc_xambg_patch_peaks,
 *     tests/test_gpu_cfar_os_bounds.py prc_cfar_os, tests/test_gpu_plots_bounds.py prc_plots, tests/test_gpu_tbd_bounds.py prc_tbd and
 *     prc_tbd_trace, tests/test_gpu_echo_bounds.py prc_echo_cancel, tests/test_gpu_channelize_bounds.py prc_channelize,
 *     tests/test_gpu_map_fuse_bounds.py prc_fuse, tests/test_gpu_recip_xambg_bounds.py prc_batch_xambg and prc_ofdm_timing;
 *     tests/test_gpu_far_blocks.py holds the strided entry points to it with the blocks more than 4 GiB apart and the dense
 *     stacks with their last frame beyond 2^32 bytes, tests/test_gpu_long_streams.py the whole-recording entry points on
 *     streams past 2^31 samples and 2^32 bytes).  Every length, stride and step declared int64_t either works at any such
 *     distance or is refused before any launch with a status and a message naming the size; each entry point's comment says
 *     which, tests/test_limits_host.py holds every limit, DESIGN.md section 26 has the audit.
 */
#ifndef PRCORE_H
#define PRCORE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRC_DESC_MAGIC 0x36435250u     /* "PRC6" */
/* zero a descriptor and fill in its header; then set the fields */
#define PRC_DESC_INIT(d) do { memset(&(d), 0, sizeof(d)); (d).struct_size = (uint32_t)sizeof(d); (d).magic = PRC_DESC_MAGIC; } while (0)

#define PRC_VERSION 680   /* 680, ninth edition (additions only, the number stays as for the editions below): prc_batch_xambg_desc,
                             prc_batch_xambg_workspace_bytes, prc_batch_xambg, prc_ofdm_timing (reciprocal-filter range-Doppler maps for OFDM
                             illuminators by the batches algorithm, and the symbol timing that aligns the batches);
                             680, eighth edition (additions only, the number stays as for the editions below): prc_fuse_desc, prc_fuse
                             (non-coherent fusion of several illuminators' maps on a position-velocity grid, on device);
                             680, seventh edition (additions only, the number stays as for the editions below): prc_channelize_desc, prc_channelize,
                             PRC_OPT_CHANNELIZE_FORM (uniform polyphase filter bank: K of M channels out of one pass over the raw samples);
                             680, sixth edition (additions only, the number stays as for the editions below): prc_echo_desc, prc_echo_atom, prc_echo_fit,
                             prc_echo_cancel_workspace_bytes, prc_echo_cancel (joint least-squares removal of strong echoes at any lag and Doppler);
                             680, fifth edition (additions only, the number stays as for the editions below): prc_tbd_desc, prc_tbd, prc_tbd_trace,
                             PRC_OPT_TBD_FRAMES, PRC_OPT_TBD_ROWS (track-before-detect: Viterbi integration of a stack of CFAR maps, on device);
                             680, fourth edition (additions only, the number stays as for the editions below): prc_plots_desc, prc_plot_info,
                             prc_plots_workspace_bytes, prc_plots (plot extraction: CFAR detections clustered into plots, on device);
                             680, third edition (additions only, no layout of 680 changed, so the number stays: a host checks for the new
                             entry points by symbol): prc_eca_workspace_bytes, prc_eca_execute, prc_eca_set_profiling, prc_eca_get_profile
                             (ECA_Filter, the joint multi-Doppler least-squares canceller, on device);
                             680, second edition (the same way): prc_cfar_os_desc, prc_cfar_training_cells, prc_cfar_os_workspace_bytes, prc_cfar_os
                             (order-statistic CFAR on CFAR_2D's window, on device);
                             680: prc_patch_desc, prc_patch, prc_patch_peak, prc_xambg_patch_workspace_bytes, prc_xambg_patch, prc_xambg_patch_peaks
                             (exact, un-decimated cross-ambiguity patches and sub-cell peak refinement on device);
                             670: prc_ls_svd_workspace_bytes, prc_ls_svd_execute, prc_ls_svd_set_profiling, prc_ls_svd_get_profile (LS_Filter_SVD
                             on device);
                             660: prc_firdec_desc, prc_fir_decimate, prc_shift, prc_normalize_workspace_bytes, prc_normalize (the rest of
                             signal_utils.py on device: decimate, channel_preprocessing, shift, offset_compensation, normalize);
                             650: prc_welch_desc, prc_welch_rows, prc_welch_workspace_bytes, prc_welch (Welch spectra on device: the psd, csd and
                             specgram of signal_preview.py);
                             640: prc_display_limits, prc_display_rgba (the render loop's percentile limits and colour map on device);
                             630: prc_strack_desc, prc_strack_record, prc_strack_workspace_bytes, prc_strack_run
                             (simple_target_tracker on device), prc_persistence (plotting_tools.persistence on device);
                             620: prc_gal_execute, prc_gal_workspace_bytes (GAL_JPE on device);
                             610: prc_track_desc, prc_track_record, prc_track_plan_create / _destroy, prc_track_measure, prc_track_run
                             (get_measurements and multitarget_tracker on device);
                             600: every descriptor (prc_caf_desc, prc_ls_desc, prc_frontend_desc, prc_iir_desc) starts with `struct_size`,
                             `magic` (layout break: rebuild hosts; from here on descriptors only grow at the end and an older host keeps
                             working); PRC_OPT_CAF_TEAM8; host arrays passed to an entry point are read before it returns;
                             500: prc_frequency_shift_phases, prc_frontend_execute2, prc_cfar2d_c64, prc_mem_info, PRC_OPT_MARKERS; 401: prc_comm_loopback, PRC_OPT_FE_METHOD, PRC_OPT_CFAR_METHOD; 400: prc_caf_desc.multi, prc_set_option / prc_get_option (no environment variables are read),
                             prc_comm_count; 310: prc_ls_desc.method = 4, NLMS up to 8192 taps */

typedef enum prc_status {
    PRC_OK = 0,
    PRC_EINVAL = -1,       /* bad argument (null pointer, non-positive size, ...)           */
    PRC_ESHAPE = -2,       /* length mismatch -> ValueError on the Python side             */
    PRC_EHIP = -3,         /* a HIP runtime call failed (no GPU, OOM, launch failure)      */
    PRC_EROCFFT = -4,      /* a rocFFT call failed                                          */
    PRC_EUNSUPPORTED = -5  /* valid request outside what this build implements              */
} prc_status;

/* ---- library / device ------------------------------------------------------------- */
int prc_version(void);
const char* prc_last_error(void);
int prc_device_count(int* count);
int prc_set_device(int device);
int prc_get_device(int* device);       /* the calling thread's current HIP device */
/* Device-memory helpers for hosts that do not bring their own allocator (the NumPy-facing
 * drop-in functions use these; torch-based callers pass tensor.data_ptr() instead). */
int prc_mem_info(size_t* free_bytes, size_t* total_bytes);   /* hipMemGetInfo of the current device */
int prc_malloc(void** dptr, size_t bytes);
int prc_free(void* dptr);
int prc_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int prc_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int prc_memset(void* dptr, int value, size_t bytes, void* stream);
int prc_stream_sync(void* stream);

/* Tuning options.  The library reads NO environment variables: kernel-selection knobs are fields of the plan
 * descriptors (method, doppler, multi) or these process-wide options, which a plan copies ONCE, at creation (a later
 * prc_set_option never changes an existing plan); prc_nlms_execute, which has no plan, reads PRC_OPT_NLMS_WAVES per call. */
typedef enum prc_option {
    PRC_OPT_CAF_MULTI_MODE = 0,   /* what prc_caf_desc.multi = PRC_CAF_MULTI_AUTO resolves to; default AUTO = the library's
                                     measured choice                                                                      */
    PRC_OPT_CAF_GROUP_MB = 1,     /* > 0: surfaces per segment/Doppler round of prc_caf_execute sized to this many MiB of
                                     slow-time buffer; default 0 = the whole batch in one round                           */
    PRC_OPT_LS_TEAM_PIECES = 2,   /* pieces per team of the 4096-point LS chain (default 32)                              */
    PRC_OPT_LS_TEAM_ALIGN = 3,    /* 1 (default): pieces of the 4096-point LS chain start on 128-byte lines; 0: E = T - 1  */
    PRC_OPT_NLMS_WAVES = 4,       /* 0 (default): wavefronts per NLMS stream from the tap count; 2 / 4: split a stream
                                     that would fit one wavefront over 2 / 4 (latency experiments)                        */
    PRC_OPT_LS_CACHE_LIMIT_MB = 5,/* > 0: an LS plan does not allocate a spectrum cache larger than this many MiB and runs
                                     the recomputing / per-bin kernels instead; default 0 = no limit                      */
    PRC_OPT_NLMS_WG_WAVES = 6,    /* 0 (default): NLMS wavefronts (= independent streams) per workgroup / CU from the stream count
                                     and the measured step times; 4 / 8 / 12 / 16: forced (16 = four per SIMD exists for the
                                     config-3 filter length only; A/B runs)                                                */
    PRC_OPT_CAF_XCD_CONTIG = 7,   /* workgroup order of the 4096-point segment kernel, read per launch (A/B runs): 0 (default) =
                                     segments go round the XCDs in launch order, 1 = every XCD takes a contiguous run of them
                                     (measured slower on MI355X)                                                            */
    PRC_OPT_CAF_PAIR_FRAMES = 8,  /* 4096-point segment kernel, frames overlapping by half, read per launch (A/B runs): 1 (default) =
                                     the two frames that cover the same samples run in consecutive slots of one XCD (config 5: -2 %
                                     at one channel, -3 % at four), 0 = frame after frame                                   */
    PRC_OPT_FE_METHOD = 9,        /* front-end kernel, read per launch: 0 (default) = the group form (`up` outputs per thread, taps
                                     through the scalar unit) where it applies (up <= 16, window within LDS), else one output per
                                     thread; 1 = one output per thread; 2 = the group form or PRC_EUNSUPPORTED                */
    PRC_OPT_CFAR_METHOD = 10,     /* prc_cfar2d, read per call: 0 (default) = separable sums (rows, then columns) where the tile fits
                                     LDS, 1 = every tap of the box per output                                               */
    PRC_OPT_MARKERS = 11,         /* 1: every prc_*_execute (and the other device entry points) opens a roctx range named after
                                     itself -- rocprofv3 --marker-trace shows the library's calls around its kernels.  The roctx
                                     library (librocprofiler-sdk-roctx.so.1, else libroctx64.so.4) is bound at run time, the first
                                     time the option is set; PRC_EUNSUPPORTED if neither loads.  Default 0: nothing is loaded    */
    PRC_OPT_FE_BALANCE = 12,      /* front-end plans, read at creation: 0 (default) = the group kernel's wavefronts take equal runs of
                                     tap rows at full width; N > 0 = runs of about equal cost (2 w + N per two rows), each run
                                     multiplying only the w output columns its rows reach (37 % fewer multiply-adds at 13:119;
                                     measured no faster at any N, 7 % slower at N = 8: A/B runs)                             */
    PRC_OPT_CAF_TEAM8 = 13,       /* 4096-point CAF segment kernel, read per launch: 0 = teams of four wavefronts, 16 points per
                                     thread (three wavefronts per SIMD); 1 = teams of EIGHT wavefronts, 8 points per thread (six per
                                     SIMD, a third LDS exchange per transform); default: the measured choice  */
    PRC_OPT_FE_FOLD = 14,         /* front-end group kernel, read per launch: 1 (default) = FOLDED tap rows where they apply (odd decimation:
                                     rows rho and rho + M of the banded tap table never meet the same output, so they share one row of
                                     full width: 184 rows instead of 294 at 13:119, no multiply-adds on zero taps); 0 = the unfolded rows  */
    PRC_OPT_TBD_FRAMES = 15,      /* prc_tbd, read per call: frames one launch advances.  0 (default) = the shipped choice (PRC_TBD_FRAMES
                                     in the time-blocked form where a frame is narrow enough for it, see prc_tbd); 1 = one frame per
                                     launch; 2 .. PRC_TBD_FRAMES_MAX = the time-blocked form with that many frames (fewer, down to 2,
                                     where LDS does not hold them; one frame per launch where it holds none).  Same bytes out at every value */
    PRC_OPT_TBD_ROWS = 16,        /* prc_tbd, read per call: rows of the band a workgroup of the time-blocked form owns.  0 (default) =
                                     from the shape (see prc_tbd); 1 .. 4096 = forced (lowered to what LDS holds).  Same bytes out       */
    PRC_OPT_CHANNELIZE_FORM = 17, /* prc_channelize, read per call: 0 (default) = the LDS-tile form where the tile fits
                                     PRC_CHANNELIZE_TILE_MAX_BYTES, the direct form elsewhere; 1 = the direct form always (tests) */
    PRC_OPT_COUNT_ = 18
} prc_option;
int prc_set_option(int32_t option, int64_t value);     /* PRC_EINVAL for an unknown option or a value out of range */
int prc_get_option(int32_t option, int64_t* value);

/* ---- cross-ambiguity surface: fast_xambg (range_doppler_processing.py:12-90) -------- */
typedef enum prc_caf_method {
    PRC_CAF_AUTO = 0,
    PRC_CAF_DIRECT = 1,    /* time-domain lagged products in LDS tiles (any decimation FIR) */
    PRC_CAF_FFT = 2,       /* per-segment FFT correlation held in LDS/registers (boxcar FIR):
                              1024-point transforms, one wavefront per segment                 */
    PRC_CAF_FFT4096 = 3    /* the same with 4096-point transforms by a team of four wavefronts:
                              what AUTO takes for wide range spans (1025 lags and more)       */
} prc_caf_method;

typedef enum prc_doppler_method {
    PRC_DOPPLER_AUTO = 0,   /* COLUMN when freq_bins is 256, 512, 1024, 2048 or 4096, else ROCFFT           */
    PRC_DOPPLER_ROCFFT = 1, /* transpose + batched 1-D rocFFT over the slow-time axis (any freq_bins) +
                               one fftshift/transpose kernel (:89)                           */
    PRC_DOPPLER_COLUMN = 2  /* one column-FFT kernel over the row-major slow-time buffer, fftshift folded
                               into the store: the surface is read once and written once    */
} prc_doppler_method;

/* How prc_caf_execute_multi runs several reference channels against one surveillance channel */
typedef enum prc_caf_multi_mode {
    PRC_CAF_MULTI_AUTO = 0,   /* the library's choice (PRC_OPT_CAF_MULTI_MODE overrides what AUTO means)               */
    PRC_CAF_MULTI_TURNS = 1,  /* one single-reference pass per illuminator (any method)                                */
    PRC_CAF_MULTI_SHARED = 2, /* 4096-point method: the surveillance pieces of a segment are transformed once for ALL
                                 illuminators (two wavefronts per SIMD)                                                */
    PRC_CAF_MULTI_PAIRS = 3   /* 4096-point method: once per PAIR of illuminators (three wavefronts per SIMD)           */
} prc_caf_multi_mode;

typedef struct prc_caf_desc {
    uint32_t struct_size;  /* sizeof(prc_caf_desc) as the host compiled it (see Conventions)   */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                 */
    int64_t n;             /* samples per CPI after zero padding = inputLen (:52-55)         */
    int32_t range_bins;    /* rangeBins; the surface has range_bins+1 columns (:64)          */
    int32_t freq_bins;     /* freqBins; decimation q = (int)(n / freq_bins) (:61)            */
    int32_t max_frames;    /* workspace is sized for this many frames per execute           */
    int32_t method;        /* prc_caf_method                                                 */
    int32_t doppler;       /* prc_doppler_method                                             */
    int32_t ntaps;         /* 0: boxcar ones(q+1) (shortFilt=True, :72); else length of taps */
    const float* taps_host;/* HOST pointer, copied at plan creation (shortFilt=False, :76)   */
    int32_t multi;         /* prc_caf_multi_mode of prc_caf_execute_multi (0 = AUTO)         */
} prc_caf_desc;
#define PRC_CAF_DESC_SIZE_600 56u      /* sizeof(prc_caf_desc) at PRC_VERSION 600: the smallest struct_size accepted */

typedef struct prc_caf_plan prc_caf_plan;

/* Limits: the segment kernels address a frame with 32-bit byte offsets, so a frame and one transform of slack must lie below
 * 4 GiB: n <= PRC_CAF_MAX_N, else PRC_ESHAPE (the message names n and the limit), checked before anything is allocated.
 * frame_stride is a 64-bit element count with no such limit: frames may lie any distance apart.  The direct and the
 * 1024-point method, and any method with the rocFFT Doppler path, put the frames of a call into a grid dimension:
 * max_frames <= PRC_MAX_BATCH there, else PRC_ESHAPE (the 4096-point method with the column Doppler kernel takes any count).
 * The limit on n holds for every method: the direct kernels index with 64 bits, but have never been run or measured
 * beyond it, and 2^16 samples of slack (sixteen 4096-point pieces) keep every prefetch of a piece past the end in range. */
#define PRC_MAX_BATCH 65535                  /* blocks / frames / channels one launch takes as a grid dimension */
#define PRC_CAF_MAX_N ((int64_t)536805376)   /* 2^29 - 2^16 complex64 samples per CPI */
int prc_caf_plan_create(prc_caf_plan** plan, const prc_caf_desc* desc);
int prc_caf_plan_destroy(prc_caf_plan* plan);
/* Which kernels the plan resolved AUTO to (prc_caf_method / prc_doppler_method values). */
int prc_caf_plan_info(const prc_caf_plan* plan, int32_t* method, int32_t* doppler,
                      int64_t* workspace_bytes);
/* The prc_caf_multi_mode the plan resolved AUTO to (TURNS / SHARED / PAIRS). */
int prc_caf_plan_multi_mode(const prc_caf_plan* plan, int32_t* multi);

/* out[f][k] for each frame: complex64 [nframes][freq_bins][range_bins+1], C order; frame b
 * reads ref/srv at element offset b*frame_stride (frame_stride = n for dense batches, = n/2
 * for the 50 %-overlapped frames of main.py:178-194).  Samples with index >= n_valid inside
 * a frame are taken as zero (the zero-pad branch :52-55); pass n_valid = n otherwise.
 * window: float32[n] device pointer or NULL (:83-84).  Column k <-> delay range_bins-k,
 * rows fftshift-ed, circular wrap of srv within the frame (:82) -- exactly as the reference. */
int prc_caf_execute(prc_caf_plan* plan, const void* ref, const void* srv, int64_t frame_stride,
                    int64_t n_valid, const float* window, void* out, int32_t nframes,
                    void* stream);
/* fast_xambg for nref (<= 8) reference channels against ONE surveillance channel in one call -- a multi-illuminator
 * frame (range_doppler_processing.py:12-90 once per pair; :81-86 is the per-pair unit): outs_host[i] receives what
 * prc_caf_execute(plan, refs_host[i], srv, ...) would write.  refs_host / outs_host are HOST arrays of nref DEVICE
 * pointers.  nframes * nref surfaces must fit the plan's max_frames.  prc_caf_desc.multi selects how (prc_caf_multi_mode):
 * the illuminators take turns through the single-reference kernels, or -- 4096-point method, segments of at most two
 * pieces (wide range spans: BASELINE configs 3 and 5) -- the surveillance pieces of a segment are transformed once for all
 * illuminators or once per pair (same results to the order of two sums).  A mode the plan's shape does not support falls
 * back to TURNS. */
int prc_caf_execute_multi(prc_caf_plan* plan, const void* const* refs_host, int32_t nref, const void* srv,
                          int64_t frame_stride, int64_t n_valid, const float* window, void* const* outs_host,
                          int32_t nframes, void* stream);
/* Stages timed separately by bench.py (same arguments; `segment` writes the plan's internal
 * slow-time buffer, `doppler` turns it into out). */
int prc_caf_execute_segments(prc_caf_plan* plan, const void* ref, const void* srv,
                             int64_t frame_stride, int64_t n_valid, const float* window,
                             int32_t nframes, void* stream);
int prc_caf_execute_doppler(prc_caf_plan* plan, void* out, int32_t nframes, void* stream);

/* cross-ambiguity surface, batches algorithm with a matched or a RECIPROCAL filter, for OFDM illuminators.
 * Beyond the reference: on a QAM-OFDM illuminator (DVB-T/T2, DAB, LTE, 5G) the matched filter of fast_xambg lifts the whole
 * surface by about 1 / sqrt(B T) of every strong echo's peak; dividing each batch of the surveillance channel by the reference
 * batch's spectrum instead of multiplying by its conjugate turns every echo into a clean impulse per batch, so no data-dependent
 * pedestal is left.  tests/batch_xambg_oracle.py is this definition in float64.
 * Per frame: ref, srv complex64 [n]; batch j = 0 .. freq_bins - 1 is the batch_len samples from start + j hop of both channels
 *   (start >= 0, hop >= 1, start + (freq_bins - 1) hop + batch_len <= n: no wrap, no zero padding; hop < batch_len overlaps).
 * Per batch: Rj = DFT(r_j), Sj = DFT(s_j), unnormalised, L = batch_len points; P_j = sum_t |r_j[t]|^2;
 *   G_j(f) = 1 (PRC_BATCH_MATCHED) or 1 / max(|Rj(f)|^2, floor^2 P_j) (PRC_BATCH_RECIPROCAL; 0 where that maximum is 0: a silent
 *   reference batch contributes nothing.  The clamp is continuous: no threshold at which two roundings could disagree);
 *   c_j(d) = (1 / L) sum_f G_j(f) Rj(f) conj(Sj(f)) e^{-2 pi i f d / L}, d = 0 .. range_bins < L: circular within the batch, in
 *   fast_xambg's conjugation convention.
 * Surface: y[j][k] = window[j] c_j(range_bins - k) (window: DEVICE float32 [freq_bins] or NULL = ones);
 *   out = fftshift over rows of DFT over j of y: complex64 [nframes][freq_bins][range_bins + 1], C order -- fast_xambg's layout:
 *   column k is delay range_bins - k, rows mirrored and fftshift-ed, a CPI of freq_bins hop samples.
 * With the reciprocal filter and batches aligned to the useful parts of the symbols (start = symbol start + cp, hop = nfft + cp,
 * batch_len = nfft) an echo a ref(t - d), d <= cp, peaks at a freq_bins (occupied carriers / batch_len).  On constant-modulus
 * carriers (QPSK) the two filters coincide up to scale; with batches that are not aligned the reciprocal filter gains nothing.
 * Kernels: batch_len 1024 = one wavefront per batch, 4096 = a team of four wavefronts per batch: both channels of a batch are
 *   loaded once, two forward transforms, the pointwise step in the transforms' permuted frequency layout, ONE inverse transform,
 *   lags 0 .. range_bins stored into `workspace` in the tile-major layout of the column Doppler kernel, which then runs.  Other
 *   batch_len, and freq_bins outside 256, 512, 1024, 2048, 4096: PRC_EUNSUPPORTED.
 * workspace: DEVICE, prc_batch_xambg_workspace_bytes bytes, the caller's; its contents before the call do not matter.
 * The call does not allocate (the small per-device twiddle tables are made the first time a shape needs them), free, copy or
 * synchronise, uses no atomics and can be captured on one stream.  Element alignment suffices.  Frame b reads ref and srv only
 * inside [b frame_stride + start, b frame_stride + start + (freq_bins - 1) hop + batch_len); frame_stride is a 64-bit element
 * count without a limit.
 * PRC_EINVAL: a bad descriptor header, an unknown filter, a floor that is negative or not finite (reciprocal filter), nframes < 0,
 * a null or misaligned pointer.  PRC_ESHAPE (the message names the value and the limit; checked before anything runs):
 * start < 0; hop < 1; range_bins outside 0 .. batch_len - 1; n outside 1 .. PRC_CAF_MAX_N; a last batch that ends beyond n;
 * nframes freq_bins > PRC_BATCH_XAMBG_MAX_BATCHES.  nframes == 0 is a no-op. */
typedef enum prc_batch_filter { PRC_BATCH_MATCHED = 0, PRC_BATCH_RECIPROCAL = 1 } prc_batch_filter;
/* (struct tag first, typedef after: tests/test_abi.py lists by name the ctypes mirror of every `typedef struct {` with int64_t
 * fields; tests/test_batch_xambg_host.py holds this one's three to c_int64, and every offset to the layout below) */
struct prc_batch_xambg_desc {
    uint32_t struct_size;  /* sizeof(prc_batch_xambg_desc) as the host compiled it (see Conventions)           */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                                   */
    int64_t n;             /* samples per frame                                                                */
    int64_t start;         /* first sample of batch 0                                                          */
    int64_t hop;           /* samples between batch starts                                                     */
    int32_t batch_len;     /* L: 1024 or 4096                                                                  */
    int32_t range_bins;    /* the surface has range_bins + 1 columns                                           */
    int32_t freq_bins;     /* batches = Doppler rows: 256, 512, 1024, 2048 or 4096                             */
    int32_t filter;        /* prc_batch_filter                                                                 */
    float floor;           /* reciprocal filter: |Rj(f)|^2 is held above floor^2 P_j (0.1 is a good start)     */
    int32_t reserved;      /* 0                                                                                */
};
typedef struct prc_batch_xambg_desc prc_batch_xambg_desc;
#define PRC_BATCH_XAMBG_DESC_SIZE_MIN 56u
#define PRC_BATCH_XAMBG_MAX_BATCHES ((int64_t)2147483647)   /* nframes * freq_bins of one call */
int prc_batch_xambg_workspace_bytes(const prc_batch_xambg_desc* desc, int32_t nframes, size_t* bytes);
int prc_batch_xambg(const prc_batch_xambg_desc* desc, const void* ref, const void* srv, int64_t frame_stride, const float* window,
                    void* out, int32_t nframes, void* workspace, void* stream);
/* OFDM symbol timing from the cyclic prefix: for o = 0 .. nfft + cp - 1
 *   metric[o] = | sum_{s < nsym} sum_{t < cp} ref[o + s (nfft + cp) + t] conj(ref[o + s (nfft + cp) + t + nfft]) |,
 * the products of the float32 samples summed in float64 (every product is exact there, so the result does not depend on the order
 * of the sums beyond the last bits); *start_out = the lowest o of the largest metric.  The batches of prc_batch_xambg are aligned
 * with start = *start_out + cp, hop = nfft + cp, batch_len = nfft.  metric_out: DEVICE float64 [nfft + cp]; start_out: DEVICE int32.
 * Any nfft >= 2, 1 <= cp < nfft, nsym >= 1 (else PRC_EINVAL); (nsym + 1) (nfft + cp) + nfft <= n and nfft + cp <= 2^31 - 1, else
 * PRC_ESHAPE (the message names the sizes).  Two launches on `stream`, no allocation, no atomics; capturable. */
int prc_ofdm_timing(const void* ref, int64_t n, int32_t nfft, int32_t cp, int32_t nsym, double* metric_out, int32_t* start_out,
                    void* stream);

/* ---- block least-squares clutter cancellers (clutter_removal.py) ------------------- */
typedef struct prc_ls_desc {
    uint32_t struct_size;  /* sizeof(prc_ls_desc) as the host compiled it (see Conventions)     */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                 */
    int64_t n;             /* samples per block (chunk)                                     */
    int32_t filter_len;    /* filterLen                                                     */
    int32_t peek;          /* non-causal taps (default 10 in the reference)                 */
    int32_t circular;      /* 0: LS_Filter_Toeplitz semantics (:109-160: circular peek shift,
                              linear correlations, linear FIR); 1: LS_Filter semantics (:6-56:
                              circular data matrix => circular correlations and FIR)        */
    int32_t max_blocks;    /* workspace is sized for this many independent blocks           */
    int32_t method;        /* 0 auto (= 3 when it fits; = 4 from 120 taps on blocks of >= 65536 samples), 1 time-domain kernels, 2 FFT kernels that
                              recompute the reference spectra per Doppler bin, 3 FFT kernels with
                              the reference spectra cached in HBM between Doppler bins, 4 the chain
                              of method 3 on 4096-point transforms where it applies (linear form,
                              <= 769 taps, n >= 8192: fewer cache bytes per sample; else as 3).  The FFT
                              kernels take up to 769 taps on 1024-point transforms (one wavefront
                              each) and up to 3073 taps on 4096-point transforms (four wavefronts).
                              Any filter_len + peek < n runs (the reference, clutter_removal.py:109-160,
                              accepts any length): above 3073 taps correlations and FIR run on the time-domain
                              kernels (the FIR in tap tiles beyond ~9000 taps); the Levinson recursion keeps
                              its three complex128 T-vectors in LDS up to 3413 taps, the autocorrelation in a
                              global workspace up to 5120, all three there beyond (seconds at 10^4 taps)       */
} prc_ls_desc;
#define PRC_LS_DESC_SIZE_600 40u

typedef struct prc_ls_plan prc_ls_plan;

/* Limits: the FFT kernels address a block with 32-bit byte offsets, so a block and one transform of slack must lie below
 * 4 GiB: n <= PRC_LS_MAX_N, else PRC_ESHAPE; the blocks of a call are one grid dimension: max_blocks <= PRC_MAX_BATCH, else
 * PRC_ESHAPE (each message names the value and the limit); both are checked before anything is allocated.  stride and
 * out_stride of prc_ls_execute are 64-bit element counts with no such limit: blocks may lie any distance apart.  The limit
 * on n holds for every method, the time-domain kernels (method 1, or more taps than the FFT kernels carry) included: they
 * index with 64 bits but have never been run or measured beyond it, and a plan is then not a different object per method. */
#define PRC_LS_MAX_N ((int64_t)536805376)    /* 2^29 - 2^16 complex64 samples per block */
int prc_ls_plan_create(prc_ls_plan** plan, const prc_ls_desc* desc);
int prc_ls_plan_destroy(prc_ls_plan* plan);

/* LS_Filter_Multiple (:162-187) on nblocks independent blocks: for each Doppler bin in
 * order, cancel the (frequency-shifted, float32 phase -- signal_utils.py:24-27) reference from
 * the previous bin's output.  nbins = 1, bins = {0} is LS_Filter_Toeplitz; with
 * desc.circular = 1 and reg it is LS_Filter.  block b reads ref/srv at b*stride elements and
 * writes complex64 out at b*out_stride.  taps_out: optional complex128 [nblocks][T] (device)
 * taps of the LAST bin (return_filter=True), T = filter_len + peek.
 * doppler_bins_host: HOST array of nbins doubles (Hz). reg is added to the Gram diagonal. */
int prc_ls_execute(prc_ls_plan* plan, const void* ref, const void* srv, int64_t stride,
                   void* out, int64_t out_stride, int32_t nblocks, double sample_rate,
                   const double* doppler_bins_host, int32_t nbins, double reg,
                   void* taps_out, void* stream);

/* Per-kernel timing for bench.py's roofline: when enabled, HIP events are recorded on the
 * caller's stream around every kernel of the next prc_ls_execute.  prc_ls_get_profile waits
 * for them and returns ms[0..2] = correlation / Levinson / FIR kernel time of that execute
 * (summed over its Doppler bins) and the number of launches of each kind. */
int prc_ls_set_profiling(prc_ls_plan* plan, int32_t enable);
int prc_ls_get_profile(prc_ls_plan* plan, double* ms, int32_t* launches_per_kind);

/* ---- NLMS_filter (clutter_removal.py:189-249) ---------------------------------------- */
/* Any filter_len + peek < n runs (the reference, clutter_removal.py:189-249, takes any length): a stream's taps live in
 * registers, 32 per lane -- one wavefront up to 2048 taps, a workgroup of two up to 4096, of four up to 8192; beyond that a
 * plain kernel (one workgroup per stream, taps in a global workspace allocated for the call: microseconds per step, and
 * the call synchronises `stream`).
 * nstreams independent sample-recursive filters, one wavefront (or one such workgroup) each.  taps_in: optional
 * complex64 [nstreams][T] initial taps (initialTaps), NULL = zeros.  taps_out: optional
 * complex64 [nstreams][T].  out: complex64, zero outside [filter_len, n-peek). */
int prc_nlms_execute(const void* ref, const void* srv, int64_t n, int64_t stride,
                     int32_t filter_len, int32_t peek, float mu, const void* taps_in,
                     void* out, int64_t out_stride, void* taps_out, int32_t nstreams,
                     void* stream);

/* ---- LS_Filter_SVD (clutter_removal.py:58-107) ------------------------------------------ */
/* nblocks independent truncated-SVD block least-squares cancellers on the circulant data matrix A[:, k] = roll(ref, k - peek),
 * T = filter_len + peek columns: h = V S^+ U^H srv, out = srv - A h (complex64).  Computed from the Gram matrix A^H A (the
 * Hermitian Toeplitz matrix of the circular autocorrelation, accumulated in float64) by one-sided Jacobi in float64; no
 * N x T matrix is formed.  Block b reads ref and srv at b*stride and writes out at b*out_stride.
 * Cut rule: a singular value is dropped when sigma < max(1e-10, rcond * sigma_max).  rcond < 0 selects the default
 * 4 sqrt(T) 2^-26 (lambda below 16 T 2^-52 lambda_max: what a Gram matrix accumulated in float64 cannot tell from its own
 * rounding); rcond = 0 is the reference's absolute rule alone; rcond must be below 1.
 * taps_out: optional complex128 [nblocks][T]; sv_out: optional double [nblocks][T], the singular values of A in descending
 * order; info_out: optional int32 [nblocks][3] = directions kept, Jacobi sweeps run (the last one without a rotation
 * included), 1 if the block converged within the cap of 30 sweeps, else 0 (its results are then those of the last sweep).
 * out = (srv - A hi) - A lo with h = hi + lo, hi the float32-representable part of h: the circular FIR kernel of
 * prc_ls_execute, which carries float32 taps, twice.
 * workspace: prc_ls_svd_workspace_bytes(n, filter_len, peek, nblocks) bytes of device memory, 16-byte aligned, owned by the
 * caller and not shared by calls in flight; nothing in it needs initialising (about 32 T^2 + 8 n bytes per block plus the
 * correlation partials).
 * The call does not allocate device memory.  It DOES synchronise: the host reads the rotation counters back once per sweep
 * (stream synchronisation) and stops at the first sweep without rotations, so the call cannot be captured into a graph; it
 * returns with the sweeps complete and the last kernels (taps, FIR) enqueued on `stream`.  Results are bit-identical from
 * run to run and do not depend on which other blocks share the call.
 * Limits: 1 <= T < n, T <= 4096, stride and out_stride >= n.  Anything else, a null ref / srv / out / workspace or a
 * misaligned workspace: PRC_EINVAL.  PRC_ESHAPE: n >= 2^31 or nblocks > PRC_MAX_BATCH (the message names the value and the
 * limit; prc_ls_svd_workspace_bytes refuses the same).  stride and out_stride have no upper limit. */
int prc_ls_svd_workspace_bytes(int64_t n, int32_t filter_len, int32_t peek, int32_t nblocks, size_t* bytes);
int prc_ls_svd_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t filter_len, int32_t peek,
                       double rcond /* < 0: the default above */, int32_t nblocks, void* out, int64_t out_stride,
                       void* taps_out /* c128 [nblocks][T] or NULL */, double* sv_out /* [nblocks][T] or NULL */,
                       int32_t* info_out /* [nblocks][3]: kept, sweeps, converged; or NULL */,
                       void* workspace, void* stream);
/* Stage timing for tools/ls_svd_bench.py, process-wide: while enabled, every prc_ls_svd_execute records events around its
 * stages and waits for its last kernel; get_profile returns the last call's milliseconds for correlate (float64
 * correlations and their reduction), jacobi (Gram set-up, the sweeps and their counter read-backs), taps (eigenvalues, cut,
 * taps) and apply (the FIR), and the number of sweeps launched. */
int prc_ls_svd_set_profiling(int32_t enable);
int prc_ls_svd_get_profile(double* ms /* [4] */, int32_t* sweeps);

/* ---- ECA_Filter: joint multi-Doppler least squares (extensive cancellation algorithm) ---- */
/* nblocks independent cancellers that solve for the taps of ALL nbins Doppler bins at once, where prc_ls_execute with the same
 * bins solves one bin after another on the previous bin's output.  T = filter_len + peek taps per bin.  Regressors
 * r_a = roll(ref ramp_a, -peek), ramp_a the float32-phase ramp of prc_frequency_shift at doppler_bins_host[a] (Hz) and
 * sample_rate, r_a = roll(ref, -peek) for a bin of 0.  In LS_Filter_Toeplitz's convention (linear lags, zero outside [0, n)):
 *     R_k[a][c] = sum_m r_c[m] conj(r_a[m-k]),  y_k[a] = sum_m srv[m] conj(r_a[m-k]),  sum_j R_{i-j} x_j = y_i  (R_-k = R_k^H),
 * `reg` >= 0 added to the diagonal of R_0, and out = srv - sum_a (r_a * w_a)[0:n] with w_a[j] = x_j[a], a linear FIR with zero
 * history (complex64).  With nbins = 1 this is prc_ls_execute with that one bin (non-circular).  Products and sums are float64
 * in a fixed order (no floating-point atomics), the solve is a block Levinson recursion in float64, the FIR keeps its taps in
 * float64.  Block b reads ref and srv at b*stride and writes out at b*out_stride.
 * taps_out: optional complex128 [nblocks][nbins][T]; info_out: optional int32 [nblocks], 0, or 1 for a block whose recursion
 * broke down: a pivot of a prediction-error block not above 2^-40 of R_0's diagonal, or anything non-finite.  Such a block
 * gets zero taps and out = srv bit for bit; nothing non-finite is stored.  Duplicate bins and an all-zero reference, both
 * with reg = 0, are the cases that reach this; bins closer than 1 / (n / sample_rate) make G ill-conditioned and are what
 * `reg` is for.
 * workspace: prc_eca_workspace_bytes(...) bytes of device memory, 16-byte aligned, owned by the caller and not shared by calls
 * in flight; nothing in it needs initialising (per block about 80 nbins^2 T bytes plus the correlation partials, at most
 * 64 x 16 nbins (nbins + 1) T bytes).
 * The call neither allocates nor synchronises, has a fixed number of launches and reads nothing back: it can be captured
 * into a graph.  Results are bit-identical from run to run and do not depend on which other blocks share the call.
 * Limits: 1 <= T < n, 1 <= nbins <= 8, nbins * T <= 4096, stride and out_stride >= n.  Anything else, a null ref / srv / out /
 * doppler_bins_host / workspace, a misaligned workspace, a negative or non-finite reg or a zero sample_rate: PRC_EINVAL.
 * PRC_ESHAPE: n >= 2^31 or nblocks > PRC_MAX_BATCH (the message names the value and the limit; prc_eca_workspace_bytes refuses
 * the same).  stride and out_stride have no upper limit. */
int prc_eca_workspace_bytes(int64_t n, int32_t filter_len, int32_t peek, int32_t nbins, int32_t nblocks, size_t* bytes);
int prc_eca_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t filter_len, int32_t peek,
                    double sample_rate, const double* doppler_bins_host, int32_t nbins, double reg, int32_t nblocks,
                    void* out, int64_t out_stride, void* taps_out /* c128 [nblocks][nbins][T] or NULL */,
                    int32_t* info_out /* [nblocks] or NULL */, void* workspace, void* stream);
/* Stage timing for tools/eca_bench.py, process-wide: while enabled, every prc_eca_execute records events around its stages and
 * waits for its last kernel; get_profile returns the last call's milliseconds for correlate (float64 correlations and their
 * reduction), solve (block Levinson) and apply (the FIR of every bin). */
int prc_eca_set_profiling(int32_t enable);
int prc_eca_get_profile(double* ms /* [3] */);

/* ---- GAL_JPE (clutter_removal.py:251-365) --------------------------------------------- */
/* nstreams independent gradient-adaptive-lattice joint-process estimators: lattice_len reflection coefficients k, then a
 * transversal NLMS stage of delay_len taps h over the lattice's backward errors (1 <= lattice_len <= delay_len).  Per
 * sample n < n - peek - 1 the input is ref[n + peek] and the output out[n] = srv[n] - h^H b; every element of out in
 * [0, n) is written (zero from n - peek - 1 on).  mu1 / mu2 are the lattice / transversal step sizes (mu1 evolves as the
 * reference's complex mu1 = min(0.999 mu1 + 1e-8 e^2, 5e-3)).  Everything is complex64 (float2) on the device.
 * k_out, h_out: optional complex64 [nstreams][delay_len], the final k (k[0] = 0) and h.
 * delay_len <= 2048: one wavefront per stream, state in registers, no workspace.  Above: one workgroup per stream, state in
 * `workspace`, prc_gal_workspace_bytes(delay_len, nstreams) bytes of device memory owned by the caller (NULL when that
 * count is 0; it must not be shared by calls in flight).  Neither allocates nor synchronises.
 * PRC_EINVAL: null pointers, non-positive sizes, negative peek, a missing workspace; PRC_ESHAPE: lattice_len > delay_len
 * or a stride shorter than n. */
int prc_gal_workspace_bytes(int32_t delay_len, int32_t nstreams, size_t* bytes);
int prc_gal_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t lattice_len,
                    int32_t delay_len, int32_t peek, float mu1, float mu2, void* out, int64_t out_stride,
                    void* k_out, void* h_out, int32_t nstreams, void* workspace, void* stream);

/* ---- helpers that sit on the path (signal_utils.py) ---------------------------------- */
/* xcorr (:29-32): z[i] = sum_n s1[n] conj(s2[n-(i-nlead)]), i = 0..nlag+nlead; complex64 out.  n is a 64-bit count: whole
 * recordings run (blocks of 4096 samples are one grid dimension: PRC_ESHAPE for n > 4096 (2^31 - 1), with n in the message). */
int prc_xcorr(const void* s1, const void* s2, int64_t n, int32_t nlead, int32_t nlag,
              void* out, void* stream);
/* frequency_shift (:24-27): y[n] = x[n] exp(j(fl32 phase ramp + phase_offset)). */
int prc_frequency_shift(const void* x, void* y, int64_t n, double fc, double fs,
                        double phase_offset, void* stream);

/* ---- front end (SURVEY 8f "next" #1): main.py:105-166 per block ------------------------------ */
typedef enum prc_raw_dtype {
    PRC_RAW_I8 = 0, PRC_RAW_U8 = 1, PRC_RAW_I16 = 2, PRC_RAW_F32 = 3, /* interleaved I,Q scalars */
    PRC_RAW_C64 = 4                                                   /* already complex64        */
} prc_raw_dtype;

typedef struct prc_frontend_desc {
    uint32_t struct_size;  /* sizeof(prc_frontend_desc) as the host compiled it (see Conventions)      */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                     */
    int64_t n_in;          /* complex samples per block (= raw scalars / 2)                     */
    int32_t raw_dtype;     /* prc_raw_dtype of the input                                         */
    int32_t up, down;      /* rational resampling factor, already reduced by their gcd           */
    int32_t ntaps;         /* length of taps_host                                                */
    int32_t n_pre_remove;  /* resample_poly's output alignment: (half_len + n_pre_pad) / down    */
    int32_t max_blocks;
    const float* taps_host;/* HOST: firwin(20 max+1, 1/max, ('kaiser',5.0)) * up with n_pre_pad
                              leading zeros (scipy.signal.resample_poly's h), copied at creation  */
} prc_frontend_desc;
#define PRC_FRONTEND_DESC_SIZE_600 48u

typedef struct prc_frontend_plan prc_frontend_plan;
/* Limits, checked before anything is allocated: n_in < 2^30 (PRC_EINVAL); the blocks of a call are one grid dimension:
 * max_blocks <= PRC_MAX_BATCH, else PRC_ESHAPE (the message names max_blocks and the limit).  raw_stride and out_stride are
 * 64-bit element counts with no upper limit. */
int prc_frontend_plan_create(prc_frontend_plan** plan, const prc_frontend_desc* desc);
int prc_frontend_plan_destroy(prc_frontend_plan* plan);
int prc_frontend_out_len(const prc_frontend_plan* plan, int64_t* n_out);   /* ceil(n_in*up/down) */
/* deinterleave_IQ (signal_utils.py:19-22) -> frequency_shift(fc, fs, block phase) (:24-27 with the
 * array phase of main.py:125-149; mix = 0 skips it) -> resample(up, down) (:15-17, padtype 'line'),
 * fused; block b reads raw at b*raw_stride (elements of the raw type) and writes complex64 at
 * b*out_stride.  phases_host: HOST array of nblocks block phase offsets (radians) or NULL; read while the call is being
 * made (the values travel in the kernel arguments), it may be freed or reused as soon as the call returns. */
int prc_frontend_execute(prc_frontend_plan* plan, const void* raw, int64_t raw_stride, int32_t mix,
                         double fc, double fs, const double* phases_host, void* out, int64_t out_stride,
                         int32_t nblocks, void* stream);
/* The same for BOTH channels of every block in one launch (main.py:133-149 tunes the reference and the surveillance
 * recording with the same frequency and the same block phases): raw_a / raw_b and out_a / out_b share the strides and
 * the phases; one rotation factor per input sample serves the two channels.  Results are bit-identical to two
 * prc_frontend_execute calls.  Ratios the group kernel does not carry run the channels one after the other. */
int prc_frontend_execute2(prc_frontend_plan* plan, const void* raw_a, const void* raw_b, int64_t raw_stride,
                          int32_t mix, double fc, double fs, const double* phases_host, void* out_a, void* out_b,
                          int64_t out_stride, int32_t nblocks, void* stream);
/* deinterleave_IQ alone: n_complex pairs of raw scalars -> complex64 */
int prc_deinterleave(const void* raw, int32_t raw_dtype, int64_t n_complex, void* out, void* stream);
/* frequency_shift with an array (per-block) phase offset: complex64 in, complex128 out, float32 ramp
 * + double block phase, as NumPy promotes it (signal_utils.py:24-27, main.py:133-149) */
int prc_frequency_shift_block(const void* x, void* y, int64_t n, double fc, double fs,
                              double block_phase, void* stream);
/* frequency_shift with one phase PER SAMPLE (signal_utils.py:24-27 broadcasts any array): phases = DEVICE double[n]
 * (phases_f32 = 0: float32 ramp + double phase, complex128 out, NumPy's promotion for float64 / integer arrays) or
 * DEVICE float[n] (phases_f32 = 1: everything in float32, complex64 out, its promotion for float32 arrays) */
int prc_frequency_shift_phases(const void* x, void* y, int64_t n, double fc, double fs,
                               const void* phases, int32_t phases_f32, void* stream);

/* ---- CFAR_2D (SURVEY 8f "next" #3): target_detection.py:683-703 ------------------------------ */
/* X: float32 [nframes][H][W] (|xambg|, H = Doppler rows, W = range columns); out float32 same shape:
 * the CFAR ratio, or 0/1 where ratio > thresh when use_thresh != 0.  Wrap-around box filter of width fw
 * with the (gw+1)^2 guard hole and the 1/(fw^2-gw^2) gain of the reference, normalised by mean|X|.  The frames are a grid
 * dimension: nframes > PRC_MAX_BATCH is PRC_ESHAPE (prc_cfar2d_c64 too), checked before anything is allocated; frame f
 * is read and written at the 64-bit offset f H W, so a stack may be longer than 2^32 bytes. */
int prc_cfar2d(const float* X, int32_t H, int32_t W, int32_t fw, int32_t gw, int32_t use_thresh,
               float thresh, float* out, int32_t nframes, void* stream);
/* CFAR_2D(np.abs(X), fw, gw[, thresh]) as range_doppler_plot.py:56-57 calls it: X = the complex64 range-Doppler maps
 * [nframes][H][W] themselves, |X| (hypotf, as np.abs) taken while the tiles are loaded -- one read of the complex map */
int prc_cfar2d_c64(const void* X, int32_t H, int32_t W, int32_t fw, int32_t gw, int32_t use_thresh,
                   float thresh, float* out, int32_t nframes, void* stream);

/* ---- order-statistic CFAR (OS-CFAR, Rohling) on CFAR_2D's window: DESIGN.md section 18 -------- */
/* The training set of cell (i, j) is X[(i + c - a) mod H, (j + c - b) mod W] for (a, b) in [0, fw)^2 outside the guard block
 * [e1, e2)^2, c = (fw-1)/2, e1 = max((fw-gw)/2, 0), e2 = min(fw-e1+1, fw): the taps of prc_cfar2d, even-fw asymmetry and
 * wrap-around (more than once when fw > H or fw > W; cells then repeat) included.  Nt = fw^2 - (e2-e1)^2 training cells
 * (prc_cfar_training_cells: 299 at (18, 4)).  The noise estimate z(i, j) is the rank-th smallest (1-based) of the Nt values,
 * selected exactly by value over all finite float32 inputs (negative ones included, -0 == +0), stored as z + 0.0f (never -0).
 * A NaN in X leaves the cells whose window holds it unspecified; nothing hangs and nothing is written elsewhere.
 *   scale PRC_CFAR_SCALE_REFERENCE: out = (X / mean|X|) / (z + 1e-10f) -- prc_cfar2d's form with z for the box mean, mean|X|
 *     from the same partial sums (an all-zero frame gives NaN, as there);
 *   scale PRC_CFAR_SCALE_PLAIN: out = X / z, IEEE float32, no epsilon, no mean pass (0/0 = NaN, x/0 = inf).
 * use_thresh != 0: out = 1.0f where the ratio > thresh, else 0.0f (NaN gives 0).  noise (or NULL): the z map.
 * X: DEVICE float32 (input = 0) or complex64 (input = 1: |X| = hypotf on the tile load, as prc_cfar2d_c64) [nframes][H][W];
 * out, noise: DEVICE float32 [nframes][H][W].  workspace: DEVICE, prc_cfar_os_workspace_bytes bytes (the mean partials of
 * the reference scale, 4-byte aligned, not shared by calls in flight; 0 bytes for the plain scale, workspace may then be NULL).
 * One kernel (plain) or two (reference) on `stream`; the call allocates, frees, copies and synchronises nothing (it can be
 * captured).  Memory: frame f of X is read only inside [f H W, (f+1) H W); only out, noise and the workspace are written;
 * element alignment suffices; a frame's result does not depend on its position in the stack or on the other frames.
 * PRC_EINVAL: a bad descriptor header, null X / out, a null workspace with the reference scale, sizes that are not positive,
 * gw < 0, Nt == 0, rank outside 0 .. Nt, a scale or input that is not listed.  PRC_EUNSUPPORTED: the 16 x 64 tile with its
 * halo does not fit 64 KiB of LDS, 4 (fw + 15) ((fw + 69) & ~3) bytes: fw <= 90 works (the same kind of limit as
 * prc_cfar2d's).  prc_cfar_training_cells and prc_cfar_os_workspace_bytes are host arithmetic and need no device. */
enum prc_cfar_scale { PRC_CFAR_SCALE_REFERENCE = 0, PRC_CFAR_SCALE_PLAIN = 1 };
typedef struct prc_cfar_os_desc {
    uint32_t struct_size;  /* sizeof(prc_cfar_os_desc) as the host compiled it (see Conventions)     */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int32_t H, W;          /* Doppler rows, range columns of a frame                                  */
    int32_t fw, gw;        /* window and guard widths, as CFAR_2D takes them                          */
    int32_t rank;          /* 1 .. Nt; 0 = ceil(0.75 Nt)                                              */
    int32_t scale;         /* prc_cfar_scale                                                          */
    int32_t input;         /* 0 = float32 magnitudes, 1 = complex64 maps                              */
    int32_t use_thresh;    /* != 0: out is 1.0f / 0.0f for ratio > thresh                             */
    float thresh;
} prc_cfar_os_desc;
#define PRC_CFAR_OS_DESC_SIZE_MIN 44u
int prc_cfar_training_cells(int32_t fw, int32_t gw, int32_t* ncells);
int prc_cfar_os_workspace_bytes(const prc_cfar_os_desc* desc, int32_t nframes, size_t* bytes);
int prc_cfar_os(const prc_cfar_os_desc* desc, const void* X, float* out, float* noise /* or NULL */, int32_t nframes,
                void* workspace, void* stream);

/* ---- channel offset estimation (SURVEY 8f "next" #2): signal_utils.py:73-78 ------------------- */
/* The zero-phase IIR decimator of scipy.signal.decimate(x, q) (ftype 'iir', zero_phase=True:
 * sosfiltfilt of a Chebyshev-I low-pass, odd extension of `padlen` samples each side, steady-state
 * initial conditions) as two spectral passes H then conj(H) on device.  The host designs the filter
 * (zeros/poles/gain of the digital low-pass) and says how many samples its impulse response needs to
 * settle (`settle`, >= log(1e-9)/log(max|pole|)). */
typedef struct prc_iir_desc {
    uint32_t struct_size;  /* sizeof(prc_iir_desc) as the host compiled it (see Conventions)           */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                      */
    int32_t q;             /* keep every q-th filtered sample                                    */
    int32_t padlen;        /* sosfiltfilt's odd-extension length, 3*(2*nsections+1 - ...) = 27    */
    int32_t settle;        /* constant-extension length standing in for the steady-state zi      */
    int32_t nzeros, npoles;/* <= 16 each                                                          */
    const double* zeros_host;  /* HOST (re, im) pairs                                             */
    const double* poles_host;  /* HOST (re, im) pairs                                             */
    double gain;
} prc_iir_desc;
#define PRC_IIR_DESC_SIZE_600 56u
/* y[j] = filtfilt(x)[j*q], j < ceil(n/q); x, y complex64 DEVICE.  PRC_ESHAPE if n <= padlen. */
int prc_decimate_iir(const void* x, int64_t n, const prc_iir_desc* iir, void* y, void* stream);
/* find_channel_offset(s1, s2, nd, nl), signal_utils.py:73-78: B1 = decimate(s1, nd), B2 = decimate(s2, nd)
 * zero-padded by nl each side, xc = |correlate(B1, B2, 'valid')| (m2 + 2 nl - m1 + 1 values,
 * xc[i] = |sum_l B1[l] conj(B2[l + m2 - m1 + nl - i])|), via rocFFT.  xc_out: DEVICE float32[n_xc] or
 * NULL; *argmax_out (HOST) = first index of the maximum, so the reference's return value is
 * (*argmax_out - nl) * nd.  Synchronises `stream` before returning. */
int prc_channel_offset(const void* s1, int64_t n1, const void* s2, int64_t n2, const prc_iir_desc* iir,
                       int64_t nl, float* xc_out, int64_t* n_xc, int64_t* argmax_out, void* stream);

/* ---- frame gather over xGMI: main.py:213-224 (da.store / to_zarr) for sharded frames ---- */
/* CPI frames shard contiguously over the GPUs of a node (one process per GPU); the only exchange of
 * the path is the gather of every rank's [frames][freq_bins][range_bins+1] complex64 block to one
 * root, as a group of RCCL point-to-point transfers (ncclSend on the peers, one ncclRecv per peer on
 * the root), each on its own xGMI link.  RCCL is bound at run time (dlopen librccl.so.1); without it
 * these entry points return PRC_EUNSUPPORTED and everything else still works.
 *   rank 0:      prc_comm_unique_id(id)  -> ship the 128 bytes to every rank (any side channel)
 *   every rank:  prc_set_device(local_gpu); prc_comm_create(&comm, id, rank, world)   (collective)
 *   every pass:  prc_gather_frames(comm, my_frames, frames_per_rank, F*(R+1), all_frames, 0, stream) */
#define PRC_COMM_ID_BYTES 128
typedef struct prc_comm prc_comm;
int prc_comm_unique_id(void* id_host);                       /* HOST buffer of PRC_COMM_ID_BYTES      */
int prc_comm_create(prc_comm** comm, const void* id_host, int32_t rank, int32_t world);
int prc_comm_rccl_version(int32_t* version);                  /* ncclGetVersion of the RCCL that was bound      */
/* what RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank): the number of ranks it connected and
 * this process's rank among them -- a bench line can show that N ranks really met */
int prc_comm_count(const prc_comm* comm, int32_t* nranks, int32_t* rank);
/* Link check of the point-to-point path on THIS rank alone: nfloats float32 from `send` to `recv` (both DEVICE, not
 * overlapping) as one grouped ncclSend + ncclRecv with this rank as its own peer -- the same RCCL calls, datatype and
 * stream discipline as prc_gather_frames, runnable on a communicator of any size including one (a one-GPU box), so a host
 * can check the RCCL binding before the first gather.  Enqueued on `stream`; not a collective. */
int prc_comm_loopback(prc_comm* comm, const void* send, void* recv, int64_t nfloats, void* stream);
int prc_comm_destroy(prc_comm* comm);
/* send: this rank's frames_per_rank_host[rank] frames of frame_elems complex64 (DEVICE).  recv (root
 * only, DEVICE): sum(frames_per_rank_host) frames, rank r's block at frame offset sum_{q<r}.  Blocks may
 * be ragged or empty.  Enqueued on `stream`; nothing synchronises.  The root's own block is a device
 * copy (skipped when send already points at its slot in recv). */
int prc_gather_frames(prc_comm* comm, const void* send, const int64_t* frames_per_rank_host,
                      int64_t frame_elems, void* recv, int32_t root, void* stream);

/* ---- target tracking: target_detection.py:164-537 (get_measurements, multitarget_tracker) ---------------------- */
/* Frames are float32 [nframes][H][W] (H = Doppler rows, W = range columns), the layout prc_cfar2d / prc_cfar2d_c64
 * write.  prc_track_measure reproduces get_measurements (:190-227) per frame: mean |v| over the whole frame (fp64), the
 * reference's fliplr(frame.T) orientation with range rows [:8] and [-8:] and Doppler columns [H/2-4, H/2+4) zeroed,
 * numpy's linear percentile from the exact order statistics x(k), x(k+1) (radix select), and every cell with
 * v/mean >= threshold, sorted by descending strength, ties by descending flat index (r*H + c in fliplr(T) row-major
 * order: np.flip(np.argsort(s, kind="stable"))).  A frame holding a NaN or Inf, or of mean 0, has no candidates.
 * prc_track_run is multitarget_tracker (:455-537) on those lists: one wavefront walks all frames in order, the track
 * state stays on the device, everything in fp64. */
typedef struct prc_track_desc {
    uint32_t struct_size;  /* sizeof(prc_track_desc) as the host compiled it (see Conventions)          */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                       */
    int32_t H, W;          /* frame shape: Doppler rows (>= 8), range columns (>= 17)              */
    int32_t ntracks;       /* 1 .. 64                                                              */
    int32_t capacity;      /* candidates stored per frame (>= 1)                                   */
    double percentile;     /* in [0, 100]; the tracker's own call uses 99.8                        */
    double doppler_extent; /* frame_extent[0] (Hz): Doppler coordinates np.linspace(-D, D, H)       */
    double range_extent;   /* frame_extent[1] (km): range coordinates np.linspace(R, 0, W)          */
} prc_track_desc;
#define PRC_TRACK_DESC_SIZE_610 48u

/* one candidate: strength v/mean, its coordinates (numpy 2.x linspace bitwise), flat index r*H + c of fliplr(T) */
typedef struct prc_track_cand {
    double strength, range, doppler;
    int64_t index;
} prc_track_cand;
#define PRC_TRACK_CAND_SIZE 32u

/* the state of one track after one frame (target_track_dtype + kalman_filter_dtype; F1, F2, Q, H, R are constants) */
typedef struct prc_track_record {
    int32_t status;          /* 0 free, 1 preliminary, 2 confirmed                                     */
    int32_t lifetime;
    double measurement[2];   /* range (km), Doppler (Hz)                                               */
    double estimate[2];
    double x[4];
    double P[16];            /* row-major 4 x 4                                                        */
    double S[4];             /* row-major 2 x 2                                                        */
    uint8_t history[20];     /* measurement_history: 1 where a measurement was assigned, newest first  */
    int32_t overflow;        /* 1: this frame had more candidates than the plan's capacity; the first
                                `capacity` (in strength order) were used                               */
} prc_track_record;
#define PRC_TRACK_RECORD_SIZE 256u

typedef struct prc_track_plan prc_track_plan;
/* PRC_EINVAL for H < 8 or W < 17 (the reference's mask slices go negative or overlap), ntracks outside 1..64, a
 * percentile outside [0, 100] or capacity < 1.  Any capacity works: above 2^19 the plan allocates a device workspace of
 * capacity / 8 bytes for prc_track_run's per-candidate bits (below, they sit in LDS). */
int prc_track_plan_create(prc_track_plan** plan, const prc_track_desc* desc);
int prc_track_plan_destroy(prc_track_plan* plan);
/* frames: DEVICE float32 [nframes][H][W]; counts: DEVICE int32 [nframes] = the TRUE candidate count of each frame (may
 * exceed capacity); cands: DEVICE prc_track_cand [nframes][capacity], the first min(count, capacity) written.  Neither
 * allocates nor synchronises. */
int prc_track_measure(prc_track_plan* plan, const float* frames, int32_t nframes, int32_t* counts,
                      prc_track_cand* cands, void* stream);
/* counts / cands as prc_track_measure wrote them; records: DEVICE prc_track_record [nframes][ntracks].  The tracks
 * start free (initialize_track(None)) at every call. */
int prc_track_run(prc_track_plan* plan, const int32_t* counts, const prc_track_cand* cands, int32_t nframes,
                  prc_track_record* records, void* stream);

/* ---- plot extraction: connected clusters of CFAR detections, one measurement per cluster: DESIGN.md section 20 ------ */
/* Beyond the reference (which has no plot extractor): the stage between a CFAR statistic and prc_track_run.
 * stat: DEVICE float32 [nframes][H][W] (H Doppler rows, W range columns: what prc_cfar2d / prc_cfar_os write).  weight: NULL
 * (the weights are stat itself) or DEVICE [nframes][H][W], float32 (weight_input = 0) or complex64 (1: |.| = hypotf on load,
 * evaluated through float64 -- exact squares, a rounded sum, a rounded root -- and rounded to float32).
 * Detection: storage cell i = h W + w detects iff stat[i] > thresh (float32 compare: NaN never detects, +Inf does) and it lies
 *   outside the excluded zones, get_measurements' masks with their widths as parameters: w < range_guard or
 *   w >= W - range_guard; Doppler column c = H-1-h inside [H/2 - doppler_guard, H/2 + doppler_guard).  The reference's widths
 *   are 8 and 4; 0 switches a zone off.
 * Plot: a connected component of detecting cells under `connectivity` 4 or 8 in (h, w); neither axis wraps.
 * Per plot, g = the weight of a cell as float64, members taken in ascending storage index: ncells; the inclusive box h0, h1,
 *   w0, w1; mass M = sum g, hbar = (sum g h) / M, wbar = (sum g w) / M, every add and divide rounded on its own (g h is exact);
 *   if M is not finite or not > 0, hbar, wbar are the peak cell's h, w.  Peak: the member with the largest stat, ties to the
 *   smallest storage index; strength = that stat as float64, peak = its storage index, index = w_p H + (H-1-h_p) (the flat
 *   index of prc_track_cand).  Coordinates, get_measurements' axes evaluated at the centroid (an integer centroid gives
 *   numpy's arange * step + start): range = wbar ((0 - R) / (W-1)) + R, doppler = ((H-1) - hbar) (2 D / (H-1)) + (-D),
 *   R = range_extent, D = doppler_extent.
 * Order of a frame's plots: descending strength, ties by descending index (prc_track_measure's key).
 * Capacities: ncells_out[f] is always the frame's true detection count.  A frame with more than max_cells detections gets
 *   counts[f] = 0 and nothing else written; the other frames of the call are unaffected.  Otherwise counts[f] = the true
 *   number of plots (it may exceed capacity) and the first min(counts[f], capacity) plots in the order above are written to
 *   cands[f][.] (and info[f][.]); slots beyond that are not touched.  cands is what prc_track_run takes from a track plan of
 *   the same capacity.
 * Storage: one 1024-thread workgroup per frame keeps three lists of C = 2^ceil(log2 min(max_cells, H W)) entries, 20 C bytes
 *   (two of 8-byte keys, one of 4-byte positions).  Up to PRC_PLOTS_LDS_CELLS = 4096 cells they sit in LDS: 20 * 4096 = 80 KiB
 *   of the 160 KiB a CDNA4 workgroup can address (8192 cells would need all 160 KiB and leave nothing for the counters).
 *   Above, the same code runs on frame f's slice [20 C f, 20 C (f+1)) of `workspace` (prc_plots_workspace_bytes bytes, 8-byte
 *   aligned, not shared by calls in flight; 0 bytes and NULL allowed on the LDS path): slower, same bytes out.
 * Results are a pure function of the inputs (integer atomics only, no float atomics): the same bytes on every call and on
 * both storage paths.  One kernel on `stream`; the call allocates, frees, copies and synchronises nothing (it can be
 * captured).  Memory: frame f of stat / weight is read only inside its H W elements; element alignment suffices.
 * PRC_ESHAPE: H or W < 2, H W > 2^31 - 1.  PRC_EINVAL: a bad descriptor header, connectivity not 4 or 8, a negative guard,
 * max_cells or capacity < 1, a NaN thresh, an extent that is not finite, weight_input not 0 or 1 with a weight, nframes < 0,
 * a null stat / counts / ncells_out / cands, a missing or misaligned workspace where one is needed.  Every check is host
 * arithmetic and needs no device; nframes == 0 is a no-op. */
#define PRC_PLOTS_LDS_CELLS 4096
typedef struct prc_plots_desc {
    uint32_t struct_size;  /* sizeof(prc_plots_desc) as the host compiled it (see Conventions)       */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int32_t H, W;          /* Doppler rows, range columns of a frame (>= 2 each)                      */
    int32_t connectivity;  /* 4 or 8                                                                  */
    int32_t range_guard, doppler_guard;   /* >= 0; the reference's masks are 8 and 4                  */
    int32_t max_cells;     /* detections held per frame (>= 1)                                        */
    int32_t capacity;      /* plots stored per frame (>= 1)                                           */
    int32_t weight_input;  /* 0 = float32, 1 = complex64; ignored when weight == NULL                 */
    float thresh;          /* NaN: PRC_EINVAL                                                         */
    double doppler_extent; /* frame_extent[0] (Hz)                                                    */
    double range_extent;   /* frame_extent[1] (km)                                                    */
} prc_plots_desc;
#define PRC_PLOTS_DESC_SIZE_MIN 64u
typedef struct prc_plot_info {
    double mass, hbar, wbar;
    int32_t ncells, h0, h1, w0, w1, peak;
} prc_plot_info;
#define PRC_PLOT_INFO_SIZE 48u
int prc_plots_workspace_bytes(const prc_plots_desc* desc, int32_t nframes, size_t* bytes);
int prc_plots(const prc_plots_desc* desc, const float* stat, const void* weight /* or NULL */, int32_t nframes,
              int32_t* counts, int32_t* ncells_out, prc_track_cand* cands /* [nframes][capacity] */,
              prc_plot_info* info /* or NULL, [nframes][capacity] */, void* workspace, void* stream);

/* ---- track-before-detect: Viterbi (dynamic-programming) integration of a stack of statistic frames: DESIGN.md section 21 ---- */
/* Beyond the reference (which decides every detection in one frame): a per-cell statistic is integrated along every admissible
 * path through the frame stack; per cell and frame the best accumulated score and a back pointer are kept (Barniv 1985;
 * Tonissen & Evans 1996).  tests/tbd_oracle.py is this definition in NumPy; the device result equals it bit for bit (the
 * sign and payload of a NaN excepted, which IEEE 754 leaves open).
 * Layout: stat, score: DEVICE float32 [nframes][H][W] (h = Doppler row, w = range column, as prc_cfar2d / prc_cfar_os / prc_plots);
 *   back: DEVICE uint8 [nframes][H][W] or NULL; row_shift: DEVICE int32 [H] or NULL (= all zero), any values; prev: DEVICE
 *   float32 [H][W] or NULL, the score of the frame before the call.
 * Input cell z'_k[h, w]: 0.0f inside an excluded zone (prc_plots' two masks with prc_plots' meaning of range_guard and
 *   doppler_guard: w < range_guard or w >= W - range_guard; Doppler column c = H-1-h inside [H/2 - doppler_guard,
 *   H/2 + doppler_guard)); otherwise z if not (z > clip), else clip (a NaN stays a NaN; clip = +Inf switches clipping off).
 * Predecessors of (h, w): for dh in [-qd, qd] (outer loop), dw in [-qr, qr] (inner loop), qd = doppler_reach, qr = range_reach,
 *   code = (dh + qd)(2 qr + 1) + (dw + qr): the cell h' = h + dh, w' = w - row_shift[h'] + dw (the shift of the PREDECESSOR's
 *   row: a row's shift is the number of range columns an echo at that row's Doppler advances per frame), evaluated without
 *   overflow for any int32 shift; it counts only if 0 <= h' < H and 0 <= w' < W.
 * Choice: best = -Inf, none chosen; over ascending codes an in-bounds predecessor with v = I_{k-1}[h', w'] is chosen iff
 *   v > best (float32 compare): a NaN or -Inf is never chosen, ties go to the smallest code.  back_k[h, w] = the chosen code,
 *   255 if none; m = the chosen v, 0.0f if none.
 * Recursion: I_k = z'_k + alpha m, the product and the sum each rounded to float32 on its own (no fused multiply-add).  Frame 0
 *   takes `prev` as I_{-1} when it is given; without it I_0 = z'_0 and back_0 = 255.  score[k] = I_k.  To continue a stream, pass
 *   the last score frame of one call as `prev` of the next: the result is that of one call over both stacks.
 * prc_tbd_trace: for end e = (frame f, storage cell c = h W + w) of ends [nends][2], paths[e][0] = c; for j >= 1 the code is
 *   back[f-j+1][paths[e][j-1]]: on 255, on a code >= ncodes, when f - j < 0 or when the predecessor formula leaves the frame (a
 *   `back` array that prc_tbd did not write), this entry and all later ones are -1; otherwise paths[e][j] = the predecessor cell
 *   (it lies in frame f - j).  An end whose frame is outside [0, nframes) or whose cell is outside [0, H W) gives a row of -1.
 *   Nothing outside back [nframes][H][W], row_shift [H], ends and paths [nends][depth] is touched.
 * Kernels.  The recursion is sequential in k and parallel in the cells.  Time-blocked form: a workgroup owns a band of B rows
 *   at full width, keeps two score buffers of B + 2 K qd rows of W + 2 qr floats in LDS (every row staged with its shift applied
 *   and -Inf where no predecessor exists) and advances K frames per launch, recomputing a halo of K qd rows on either side:
 *   ceil(nframes / K) launches.  It runs where 2 frames fit: 8 (W + 2 qr)(1 + 4 qd) <= PRC_TBD_LDS_BYTES, i.e. W <= 3991 at reach
 *   (1, 1); K = PRC_TBD_FRAMES (PRC_OPT_TBD_FRAMES overrides), lowered while B >= 1 does not fit; B = ceil(H / 256), one
 *   workgroup per compute unit (PRC_OPT_TBD_ROWS overrides), lowered to what LDS holds.  Wider frames run one frame per
 *   launch from global memory (the same device code for z', the choice and the sum).  Both forms, every K and every B write the
 *   same bytes.  Frames are ordered by launches on `stream` alone: no workgroup waits for another.
 * Neither call allocates, frees, copies or synchronises; both can be captured.  No atomics: the bytes out are a pure function
 * of the arguments.  Element alignment suffices.  score must not overlap stat or prev.
 * PRC_ESHAPE: H or W < 1, H W > 2^31 - 1.  PRC_EINVAL: a bad descriptor header, a negative reach or guard, more than 255 codes,
 * alpha not in (0, 1], a NaN clip, depth < 1, nframes or nends < 0, a null stat / score (prc_tbd, nframes > 0) or back / ends /
 * paths (prc_tbd_trace, nends > 0).  Every check is host arithmetic and needs no device; nframes == 0 and nends == 0 are no-ops. */
#define PRC_TBD_FRAMES 8            /* K of the shipped time-blocked form (DESIGN.md section 21 has the measurements) */
#define PRC_TBD_FRAMES_MAX 32
#define PRC_TBD_LDS_BYTES 159744    /* 156 KiB of the 160 KiB a CDNA4 workgroup can address */
typedef struct prc_tbd_desc {
    uint32_t struct_size;  /* sizeof(prc_tbd_desc) as the host compiled it (see Conventions)                   */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                                    */
    int32_t H, W;          /* Doppler rows, range columns of a frame (>= 1 each)                                */
    int32_t doppler_reach, range_reach;   /* qd, qr >= 0, (2 qd + 1)(2 qr + 1) <= 255                           */
    int32_t range_guard, doppler_guard;   /* >= 0, as prc_plots_desc                                            */
    float alpha;           /* forgetting factor in (0, 1]                                                       */
    float clip;            /* largest z' (+Inf: off; NaN: PRC_EINVAL)                                           */
} prc_tbd_desc;
#define PRC_TBD_DESC_SIZE_MIN 40u
int prc_tbd(const prc_tbd_desc* desc, const float* stat, const int32_t* row_shift /* or NULL */, const float* prev /* or NULL */,
            int32_t nframes, float* score /* [nframes][H][W] */, uint8_t* back /* or NULL */, void* stream);
int prc_tbd_trace(const prc_tbd_desc* desc, const uint8_t* back, const int32_t* row_shift /* or NULL */, int32_t nframes,
                  const int32_t* ends /* [nends][2]: frame, cell */, int32_t nends, int32_t depth, int32_t* paths /* [nends][depth] */,
                  void* stream);

/* Fusion of several illuminators' maps on a position-velocity grid: the third consumer of a stack of
 * CFAR maps beside prc_plots and prc_tbd, and the first of the K stacks of prc_caf_execute_multi together.
 * Beyond the reference (which has one illuminator): each illuminator puts a target on an ellipsoid (excess bistatic range) and
 * on a plane in velocity space (bistatic Doppler); only the true position and velocity lie on all of them.  Every
 * (x, y, vx, vy) hypothesis is scored by reading the cell each illuminator's map would show it in, the scores are combined
 * without phase, and per position cell the best velocity is kept.  tests/fuse_oracle.py is this definition in NumPy; the device
 * result equals it bit for bit.
 * Layout: stat: DEVICE float32, the map [H][W] (h = Doppler row, w = range column, as prc_cfar2d / prc_cfar_os / prc_tbd) of
 *   illuminator k, frame f at stat + k illum_stride + f frame_stride (elements); best: DEVICE float32 [nframes][ny][nx]; vel:
 *   DEVICE int32 [nframes][ny][nx] or NULL; illum_host: HOST double [nillum][PRC_FUSE_ILLUM_DOUBLES], per illuminator
 *   {tx[3], wavelength, baseline, col0, col_per_m, row0, row_per_hz} -- nine values (baseline = |tx - rx| as the caller
 *   computed it); it is read before the call returns and travels in the kernel arguments: nothing is queued from caller memory.
 * Arithmetic: all geometry is float64, every operation rounded on its own (no fused multiply-add), in the order written.
 * Position: cell (iy, ix) is p = (x0 + ix dx, y0 + iy dy, z).
 * Per cell and illuminator: d_t = sqrt(((px - tx_x)^2 + (py - tx_y)^2) + (pz - tx_z)^2), d_r the same against rx;
 *   col = rint(col0 + ((d_t + d_r) - baseline) col_per_m);  g_x = ((px - tx_x) / d_t + (px - rx_x) / d_r) / wavelength, g_y the
 *   same in y; a quotient whose distance is 0 is 0.  rint rounds halves to even.
 * Velocity: hypothesis j = jy nvx + jx has v = (vx0 + jx dvx, vy0 + jy dvy), no vertical component;
 *   f = -(g_x vx + g_y vy) (positive Doppler: the bistatic range is closing, as in prc_tbd's row shifts);
 *   row = rint(row0 + f row_per_hz).
 * Sample: s_k = stat_k[row][col] if 0 <= row <= H - 1 and 0 <= col <= W - 1, compared in float64 before any conversion (a NaN
 *   or a huge value misses); otherwise s_k = 0.0f.
 * Combine: PRC_FUSE_SUM: S = ((s_0 + s_1) + s_2) ... in float32, each sum rounded; PRC_FUSE_MIN: m = s_0, then
 *   m = s_k < m ? s_k : m (a NaN s_k, k >= 1, is passed over; a NaN s_0 stays).
 * Reduce: best = -Inf, vel = -1; over ascending j, hypothesis j is chosen iff S > best (float32 compare): ties go to the lowest
 *   j, a NaN (or -Inf) is never chosen.  best[f][iy][ix] = the chosen S, vel[f][iy][ix] = the chosen j.  Nothing depends on
 *   the frame except the samples.
 * Kernels (form): PRC_FUSE_FORM_GLOBAL gathers the samples from global memory.  PRC_FUSE_FORM_LDS: a workgroup owns a tile of
 *   8 x 8 (above four illuminators: 4 x 4) neighbouring position cells and a run of frames, computes the geometry once, and -- neighbouring cells see
 *   neighbouring columns -- stages per frame and illuminator only the band of columns its cells read, [H][cmax_k - cmin_k + 1],
 *   in LDS and gathers from there, where the K bands fit PRC_FUSE_LDS_BYTES less 2 KiB; a tile whose bands do not fit gathers
 *   from global memory.  PRC_FUSE_FORM_AUTO (0) = the shipped choice.  Every form writes the same bytes.  In both several lanes
 *   split a cell's hypotheses and merge their partial results under the rule above (larger S, at equal S the lower j).
 * The call does not allocate, free, copy or synchronise and can be captured.  No atomics: the bytes out are a pure function of
 * the arguments.  Element alignment suffices; every index into stat is formed in 64 bits, so the maps may lie anywhere.
 * PRC_EINVAL (host arithmetic, no device needed): a bad descriptor header; nillum outside 1 .. PRC_FUSE_MAX_ILLUM; H, W, nx, ny,
 * nvx or nvy < 1; H W, nx ny or nvx nvy > 2^31 - 1; more than 2^22 tiles of 4 x 4 cells; an unknown combine or form; a
 * non-finite grid, velocity, receiver or illuminator parameter; a wavelength <= 0; nframes < 0; strides that let two maps
 * overlap (a stride counts only where there is a second illuminator / frame; negative strides are refused); a null
 * illum_host; a null stat or best with nframes > 0.  nframes == 0 is a no-op. */
#define PRC_FUSE_MAX_ILLUM 8        /* the reference channels prc_caf_execute_multi takes in one call */
#define PRC_FUSE_ILLUM_DOUBLES 9
#define PRC_FUSE_LDS_BYTES 159744   /* 156 KiB of the 160 KiB a CDNA4 workgroup can address */
typedef enum prc_fuse_combine { PRC_FUSE_SUM = 0, PRC_FUSE_MIN = 1 } prc_fuse_combine;
typedef enum prc_fuse_form { PRC_FUSE_FORM_AUTO = 0, PRC_FUSE_FORM_GLOBAL = 1, PRC_FUSE_FORM_LDS = 2 } prc_fuse_form;
typedef struct prc_fuse_desc {
    uint32_t struct_size;  /* sizeof(prc_fuse_desc) as the host compiled it (see Conventions)                   */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                                    */
    int32_t nillum;        /* K illuminators, 1 .. PRC_FUSE_MAX_ILLUM                                           */
    int32_t H, W;          /* Doppler rows, range columns of a map (>= 1 each)                                  */
    int32_t nx, ny;        /* position cells                                                                    */
    int32_t nvx, nvy;      /* velocity hypotheses                                                               */
    int32_t combine;       /* prc_fuse_combine                                                                  */
    int32_t form;          /* prc_fuse_form                                                                     */
    int32_t reserved;      /* 0                                                                                 */
    double x0, dx, y0, dy, z;          /* position of cell (iy, ix): (x0 + ix dx, y0 + iy dy, z), metres        */
    double vx0, dvx, vy0, dvy;         /* velocity of hypothesis (jy, jx): (vx0 + jx dvx, vy0 + jy dvy), m/s    */
    double rx[3];                      /* the receiver, metres                                                  */
} prc_fuse_desc;
#define PRC_FUSE_DESC_SIZE_MIN 144u
int prc_fuse(const prc_fuse_desc* desc, const double* illum_host, const float* stat, int64_t illum_stride, int64_t frame_stride,
             int32_t nframes, float* best /* [nframes][ny][nx] */, int32_t* vel /* or NULL */, void* stream);

/* ---- single-target tracker: target_detection.py:530-681 (simple_target_tracker) ------------------------------------ */
/* Frames are [nframes][H][W] (H Doppler rows, W range columns), float32 (the CFAR output) or float64.  The result is the
 * reference's on the frames as float64: per frame, v / mean|v| (whole frame), s = fliplr(frame.T), the masks s[:8, :],
 * s[-8:, :], s[:, 250:260] (Python slice rules), the lock state's gate around the previous measurement_idx (slice
 * normalisation, so a gate may wrap to empty), np.argmax(s * gate) with its NaN rule, then lock state and the adaptive
 * Kalman update in fp64.  A float64 frame may differ only where the reference's own division merges two values within
 * about one ulp (the kernels compare raw values).
 * prc_strack_run enqueues two kernels on `stream`: a scan of every frame (several workgroups per frame, each frame read
 * once) into `workspace`, then ONE workgroup that walks the frames in order, keeps the state on the device and reads only
 * the gate window of a gated frame.  Neither allocates nor synchronises. */
typedef enum prc_real_dtype { PRC_REAL_F32 = 0, PRC_REAL_F64 = 1 } prc_real_dtype;

typedef struct prc_strack_desc {
    uint32_t struct_size;  /* sizeof(prc_strack_desc) as the host compiled it (see Conventions)          */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                         */
    int32_t H, W;          /* frame shape: Doppler rows, range columns (>= 1 each, H * W < 2^31)       */
    int32_t dtype;         /* prc_real_dtype of the frames                                           */
    int32_t reserved;      /* 0                                                                      */
    double range_extent;   /* rangeExtent (km):   range   = range_extent * (1 - i0 / W)               */
    double doppler_extent; /* dopplerExtent (Hz): doppler = doppler_extent * (2 * i1 / H - 1)         */
} prc_strack_desc;
#define PRC_STRACK_DESC_SIZE_630 40u

/* the tracker's state after one frame (target_track_dtype_simple; range/doppler extents and F1, F2, Q, H, R are
 * constants and not stored) */
typedef struct prc_strack_record {
    double lock_mode[4];        /* one-hot: 0 unlocked, 1 locking on, 2 locked, 3 losing lock             */
    double measurement[2];      /* range (km), Doppler (Hz)                                               */
    int64_t measurement_idx[2]; /* (range row, Doppler column) of s = fliplr(frame.T)                     */
    double estimate[2];
    double x[4];
    double P[16];               /* row-major 4 x 4                                                        */
    double S[4];                /* row-major 2 x 2                                                        */
} prc_strack_record;
#define PRC_STRACK_RECORD_SIZE 272u

/* device bytes prc_strack_run needs in `workspace` for nframes frames of desc's shape */
int prc_strack_workspace_bytes(const prc_strack_desc* desc, int32_t nframes, size_t* bytes);
/* frames: DEVICE [nframes][H][W] of desc->dtype; state_in: DEVICE record to resume from (the last record of an earlier
 * call), or NULL for the reference's initial state -- kept with its field-order quirk: measurement [30, -20],
 * measurement_idx [35, -30], estimate [50, 50], lock_mode unlocked; records: DEVICE prc_strack_record [nframes];
 * workspace: DEVICE, prc_strack_workspace_bytes bytes, not shared by calls in flight.  PRC_EINVAL for a bad descriptor,
 * dtype or shape, nframes < 0 or a null pointer. */
int prc_strack_run(const prc_strack_desc* desc, const void* frames, int32_t nframes, const prc_strack_record* state_in,
                   prc_strack_record* records, void* workspace, void* stream);

/* ---- persistence: plotting_tools.py persistence(X, k, hold, decay) ------------------------------------------------- */
/* out[j] = sum_{i < n} frames[k - i] * decay**i for k = k_first + j, j < k_count, n = min(k + 1, hold), bitwise as the
 * reference: the sum starts at +0.0 and adds the terms in order i = 0, 1, ..., each product and sum rounded on its own (no
 * FMA); decay**i is the host libm pow(decay, i); a float32 frame gives the float32 product fl32(x * fl32(decay**i))
 * (NumPy >= 2), widened and added in float64.  k < 0 or hold <= 0 give zeros.  frames: DEVICE [nframes][frame_elems] of
 * in_dtype; out: DEVICE [k_count][frame_elems] of out_dtype (float32: the float64 sum rounded once).  The powers travel in
 * the kernel arguments, 256 per launch; with more terms the launches chain through a float64 `out`, so a float32 out
 * takes at most 256 terms.  Neither allocates nor synchronises.  PRC_EINVAL for bad dtypes, negative sizes, a null
 * pointer, a frame k >= nframes that would be read, more than 256 terms with a float32 out, frame_elems above
 * 256 (2^31 - 1) or k_count above 8 PRC_MAX_BATCH (the message names the value and the limit).  frame_elems and every
 * element index k * frame_elems + e are 64-bit: a stack may be longer than 2^32 bytes. */
#define PRC_PERSISTENCE_TERMS_PER_LAUNCH 256
int prc_persistence(const void* frames, int32_t in_dtype, int64_t frame_elems, int32_t nframes, int32_t k_first,
                    int32_t k_count, int32_t hold, double decay, void* out, int32_t out_dtype, void* stream);

/* ---- display frames: range_doppler_plot.py:72-92 (np.percentile limits, imshow's Normalize + colour map) ------------- */
/* Frames are [nframes][H][W] (H Doppler rows, W range columns) of `dtype` (prc_real_dtype); a float32 frame is taken as
 * its values widened to float64 (not NumPy's float32 percentile arithmetic).  All arithmetic is float64, every operation
 * rounded on its own, so limits and pixels are those of NumPy / matplotlib bit for bit.
 * prc_display_limits: limits[f] = {percentile(frame f, p_lo), hi_scale * percentile(frame f, p_hi)}, NumPy's default
 * (linear) percentile from the exact order statistics x(k), x(k+1) (radix select, one workgroup per frame) and NumPy's
 * _lerp.  A frame holding a NaN has both limits NaN; as in NumPy, so has one whose interpolation meets Inf - Inf or
 * Inf * 0 (a frame holding Inf).  -0.0 and +0.0 are one value and the sign of a zero limit is unspecified.
 * prc_display_rgba: per cell v, xa = ((v - vmin) / (vmax - vmin)) * 256 with {vmin, vmax} = limits[f] read on the device
 * (the two calls chain on a stream with no host round trip); the pixel is (0,0,0,0) for a NaN xa (matplotlib's "bad"
 * colour), lut[0] for xa < 0, lut[255] for xa >= 256, else lut[trunc(xa)]; vmin == vmax gives lut[0] everywhere.
 * Deviation: for vmin > vmax matplotlib raises; here the whole frame is (0,0,0,0) and the limits show why (a batched
 * device call does not synchronise to raise).  lut_host: HOST 256 x RGBA8, or NULL for gnuplot2 (closed form at
 * linspace(0, 1, 256), clipped, * 255 truncated, alpha 255); it travels in the kernel arguments.
 * out: PRC_DISPLAY_PLOT writes s = fliplr(frame.T), out[f][r][c] = colour(frame[f][H-1-c][r]), shape [nframes][W][H][4];
 * PRC_DISPLAY_STORED writes [nframes][H][W][4].
 * Memory: reads only inside the nframes * frame_elems frame elements and the 2 * nframes limits, writes only the
 * 2 * nframes limits / the 4 * nframes * H * W bytes of out; pointers need the alignment of their element (out: of one
 * pixel, 4 bytes).  Neither allocates, copies nor synchronises.  PRC_EINVAL for a bad dtype or orient, a percentile
 * outside [0, 100] or NaN, frame_elems < 1 or >= 2^31, H or W < 1 or H * W >= 2^31, nframes < 0 or a null pointer
 * (lut_host excepted); nothing is written then.  nframes == 0 is a no-op. */
typedef enum prc_display_orient { PRC_DISPLAY_PLOT = 0, PRC_DISPLAY_STORED = 1 } prc_display_orient;
int prc_display_limits(const void* frames, int32_t dtype, int64_t frame_elems, int32_t nframes, double p_lo, double p_hi,
                       double hi_scale, double* limits, void* stream);
int prc_display_rgba(const void* frames, int32_t dtype, int32_t H, int32_t W, int32_t nframes, const double* limits,
                     const uint8_t* lut_host, int32_t orient, uint8_t* out, void* stream);

/* ---- Welch spectra: signal_preview.py:51-54, 68-71 (plt.psd = matplotlib.mlab.psd), mlab.csd, mlab.specgram ------------ */
/* mlab._spectral_helper for complex input (sides='twosided', pad_to == NFFT): segment s of a channel is its samples
 * [s * (nfft - noverlap), + nfft); per segment the mean is subtracted (detrend = 1), THEN the window applied, then the
 * nfft-point DFT X_s taken.  With y == NULL out is float64 [nch][rows][nfft] of mean_s |X_s[k]|^2 * scale; with y given
 * (same n, stride, step and in_dtype as x) it is complex128 [nch][rows][nfft] of mean_s conj(X_s[k]) Y_s[k] * scale.  The
 * frequency axis is stored centred as mlab returns it (np.roll(., -nfft/2)): bin k sits at index (k + nfft/2) mod nfft.
 * n < nfft is one segment, zero from n on (mlab pads it; the zeros take part in the mean); otherwise
 * nseg = (n - nfft) / (nfft - noverlap) + 1 and the samples after the last whole segment are never read.
 * Memory: channel c is read at element c * stride + i * step for i < n and nowhere else, an ELEMENT being one complex
 * sample (one I,Q pair of the raw types: x + c * stride elements is 2 * c * stride scalars on); every element of out is
 * written.  x, y need the alignment of their scalar type (int8: any address), out and workspace 8 bytes.
 * Arithmetic: the samples are converted while they are loaded, the transform is float32 inside LDS with twiddles from
 * float64 sincospi rounded once, |X|^2 or conj(X) Y is formed in float64 and summed in float64 in a fixed order (no
 * atomics): two calls give the same bits, and prc_welch(x, x) has the auto spectrum as its real part, bit for bit, and a
 * zero imaginary part.  Three kernels on `stream`; neither allocates nor synchronises.  `workspace`: DEVICE,
 * prc_welch_workspace_bytes bytes, not shared by calls in flight (it holds the twiddles and the per-workgroup sums).
 * PRC_EINVAL: nfft not a power of two in 64 .. 8192, noverlap outside [0, nfft), navg < 0, a detrend other than 0 / 1, a
 * bad in_dtype, step < 1, n < 1, nch < 1, null pointers (y excepted), a bad descriptor header; PRC_ESHAPE: navg > nseg;
 * PRC_EUNSUPPORTED: nch * rows * (workgroups per row, at most 64) above 2^31 - 1.  n, stride and every sample index are 64-bit.
 * prc_welch_rows and prc_welch_workspace_bytes are host arithmetic and need no device. */
typedef struct prc_welch_desc {
    uint32_t struct_size;  /* sizeof(prc_welch_desc) as the host compiled it (see Conventions)             */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int32_t nfft;          /* power of two, 64 .. 8192                                                */
    int32_t noverlap;      /* 0 .. nfft-1; segment s starts at sample s*(nfft-noverlap)               */
    int32_t navg;          /* 0: one output row = the mean of all segments; k > 0: row r = the mean of
                              segments [r*k, (r+1)*k), rows = nseg / k (segments left over are dropped) */
    int32_t detrend;       /* 0 none, 1 subtract the segment's mean before the window                 */
    int32_t in_dtype;      /* prc_raw_dtype: I8/U8/I16/F32 interleaved I,Q scalars, or C64            */
    int32_t step;          /* >= 1: sample i of a channel is element i*step (complex elements);
                              2 = two channels interleaved sample by sample, signal_preview.py:33-34  */
    double scale;          /* every output value is multiplied by this once, in float64               */
} prc_welch_desc;
#define PRC_WELCH_DESC_SIZE_650 40u
int prc_welch_rows(const prc_welch_desc* desc, int64_t n, int64_t* nseg, int64_t* rows);
int prc_welch_workspace_bytes(const prc_welch_desc* desc, int64_t n, int32_t nch, size_t* bytes);
int prc_welch(const prc_welch_desc* desc, const void* x, const void* y /* NULL: auto spectrum */, int64_t n, int64_t stride,
              int32_t nch, const float* window /* DEVICE float32[nfft] */, void* out, void* workspace, void* stream);

/* ---- FIR decimator and the rest of signal_utils.py: decimate (:11-13), channel_preprocessing (:80-85), shift (:34-47),
 *      normalize (:7-9) ------------------------------------------------------------------------------------------------- */
/* prc_fir_decimate: y[j] = sum_{k < ntaps} taps[k] * xt[j*q + (ntaps-1)/2 - k], j < ceil(n / q), xt zero outside [0, n):
 * scipy.signal.decimate(x, q, ntaps - 1, ftype='fir') -- zero phase, zero padding -- with the caller's taps.  xt[i] is
 * sample i of the channel converted to complex64 (raw_dtype: interleaved I,Q scalars of deinterleave_IQ, or complex64) and,
 * with mix != 0, multiplied by exp(j ph), ph = fl32(fl32(fl32(2 pi fc) fl32(i)) fl32(1 / fl32(fs))) + fl32(phase_offset):
 * the float32 ramp of frequency_shift (:24-27), bit for bit what prc_frequency_shift computes.  deinterleave -> tune ->
 * decimate is then ONE launch (channel_preprocessing) and the tuned samples never reach memory.
 * Memory: channel c is read at element c*stride + i*step for i < n and nowhere else, an ELEMENT being one complex sample
 * (one I,Q pair of the raw types); output j of channel c is written at complex64 element c*out_stride + j*out_step and
 * nothing else is.  An (n, k) C-order array is step = k, stride = 1, nch = k (and out_step = k, out_stride = 1 for the
 * (ceil(n/q), k) result); two channels interleaved sample by sample are step = 2, stride = 1.  x needs the alignment of its
 * scalar type, out 8 bytes.  taps: DEVICE float32[ntaps].
 * Two forms, chosen from q and ntaps alone: ntaps == 20 q + 1 and 2 <= q <= PRC_FIRDEC_TILE_MAX_Q stages a tile of tuned
 * samples in LDS, phase-major, and every lane slides a register window along q short filters (taps wave-uniform); anything
 * else runs one wavefront per output, lanes striding over the taps.  Sums are float32 in a fixed order, no atomics: two calls
 * give the same bits.  One kernel on `stream`; neither allocates nor synchronises (it can be captured).  n == 0 is a no-op.
 * PRC_EINVAL: a bad descriptor header, q < 1, ntaps < 1 or even, a bad raw_dtype, fs == 0 with mix, step < 1, n < 0,
 * nch < 1 or > 65535, out_step < 1, null pointers; PRC_ESHAPE: ntaps >= 2^24. */
typedef struct prc_firdec_desc {
    uint32_t struct_size;  /* sizeof(prc_firdec_desc) as the host compiled it (see Conventions)            */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int32_t q;             /* keep every q-th filtered sample                                         */
    int32_t ntaps;         /* odd; decimate's own filter is 20 q + 1 taps                             */
    int32_t raw_dtype;     /* prc_raw_dtype of the input                                              */
    int32_t mix;           /* 0: no rotation; 1: rotate sample i by the float32 ramp of fc, fs        */
    double fc, fs;         /* frequency_shift(x, fc, fs, phase_offset)                                 */
    double phase_offset;   /* scalar phase (radians), rounded to float32 as NumPy does                 */
} prc_firdec_desc;
#define PRC_FIRDEC_DESC_SIZE_660 48u
#define PRC_FIRDEC_TILE_MAX_Q 59       /* the phase-major LDS tile is 2760 q bytes: 59 is the last q within 160 KiB */
int prc_fir_decimate(const prc_firdec_desc* desc, const float* taps, const void* x, int64_t n, int64_t step, int64_t stride,
                     int32_t nch, void* out, int64_t out_step, int64_t out_stride, void* stream);
/* shift: y = x delayed by `shift` rows (shift < 0: advanced), zeros where nothing arrives; x, y: [rows][row_bytes] bytes,
 * not overlapping.  Every byte of y is written, nothing else; x is read only where it is used.  Any alignment.
 * PRC_EINVAL: null pointers, rows < 0, row_bytes < 1.  rows == 0 is a no-op. */
int prc_shift(const void* x, void* y, int64_t rows, int64_t row_bytes, int64_t shift, void* stream);
/* normalize: y = x / mean|x| over all n elements; is_complex = 0: float32, 1: complex64 (|x| = hypotf).  |x| is summed
 * in float64, per workgroup into `workspace` (prc_normalize_workspace_bytes bytes, DEVICE, 8-byte aligned, not shared by
 * calls in flight), the partial sums are added in workgroup order, the mean is rounded to float32 once and every element is
 * divided by it in float32.  Two kernels on `stream`, no atomics, two calls give the same bits; neither allocates nor
 * synchronises.  y may be x.  PRC_EINVAL: null pointers, n < 1, is_complex not 0 / 1. */
int prc_normalize_workspace_bytes(int64_t n, size_t* bytes);
int prc_normalize(const void* x, void* y, int64_t n, int32_t is_complex, void* workspace, void* stream);

/* channelize (signal_utils.channelize, beside channel_preprocessing in this section): a uniform polyphase filter bank, K of M
 * channels out of one pass over the raw samples.  Channel k of nchan = M is centred at k fs / M.  With real taps h of odd length L = ntaps, c = (L - 1) / 2, x zero outside
 * [0, n) and `start` the stream index of x[0], row i of the result is channel k_i = channels[i]:
 *   y[i][j] = sum_{t < L} h[t] x[j dec + c - t] w^((k_i (start + j dec + c - t)) mod M),  w = exp(-2 pi i / M),  j < ceil(n / dec)
 * -- what prc_fir_decimate with mix gives for fc = -k_i fs / M if its phase ramp were exact.  dec need not equal, divide or
 * be divided by M.  The exponent is an integer reduced modulo M (start is an int64: 2^40 is as accurate as 0), the rotation
 * is read from `twiddles`, DEVICE float2[M] = (cos, sin)(2 pi r / M) evaluated in float64 and rounded to float32.  The FIR is
 * computed once per output time and shared by the channels: grouped by tap phase p = t mod M it leaves M partial sums u_p,
 * and channel k is w^(k (start + j dec + c)) sum_p w^(-k p) u_p -- an M-point DFT at the output rate.
 * taps: DEVICE float32[ntaps]; channels: DEVICE int32[nsel], each in [-M/2, M) (k and k - M are the same channel; any other
 * value is folded modulo M), duplicates allowed; x: DEVICE raw_dtype (interleaved I,Q scalars of deinterleave_IQ, or
 * complex64); out: DEVICE complex64, row i at element i * out_stride.
 * Memory: x is read only inside [0, n) samples, taps inside [0, ntaps), twiddles inside [0, M), channels inside [0, nsel);
 * exactly the nsel * ceil(n / dec) promised elements of out are written and nothing else is.  x needs the alignment of its
 * scalar type, out and twiddles 8 bytes, taps and channels 4.
 * Two forms, chosen from dec and ntaps alone: where the (256 + ceil(c / dec) + floor(c / dec) + 1 | 1) * dec * 8 bytes of a
 * tile are at most PRC_CHANNELIZE_TILE_MAX_BYTES (dec <= 73 with decimate's 20 dec + 1 taps) a wavefront stages the raw
 * samples of 256 output times in LDS, sample-phase-major modulo dec, and runs the sums above with wave-uniform taps and
 * twiddles, eight channels at a time over the same staged tile; anything else runs one wavefront per output time and
 * channel, lanes striding over the taps (PRC_OPT_CHANNELIZE_FORM = 1 forces this form).  Sums are float32 fused
 * multiply-adds in a fixed order, no atomics: two calls give the same bits, and the bits of a channel do not depend on which
 * other channels were asked for or in what order.  One kernel on `stream`; neither allocates nor synchronises (it can be
 * captured).  n == 0 is a no-op.
 * PRC_EINVAL: a bad descriptor header, nchan outside 2 .. PRC_CHANNELIZE_MAX_CHAN, dec < 1, ntaps < 1 or even, a bad
 * raw_dtype, nsel outside 1 .. PRC_CHANNELIZE_MAX_SEL, n < 0, out_stride < ceil(n / dec) with nsel > 1, null or misaligned
 * pointers; PRC_ESHAPE: ntaps >= 2^24. */
typedef struct prc_channelize_desc {
    uint32_t struct_size;  /* sizeof(prc_channelize_desc) as the host compiled it (see Conventions)       */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int32_t nchan;         /* M: channels of the bank, centred at k fs / M; 2 .. PRC_CHANNELIZE_MAX_CHAN */
    int32_t dec;           /* D >= 1: keep every D-th output time                                     */
    int32_t ntaps;         /* odd; decimate's own filter is 20 D + 1 taps                             */
    int32_t raw_dtype;     /* prc_raw_dtype of the input                                              */
    int32_t nsel;          /* K: channels this call computes, 1 .. PRC_CHANNELIZE_MAX_SEL             */
    int32_t reserved;      /* 0                                                                       */
    int64_t start;         /* stream index of x[0]: a later block of a stream continues the phase     */
} prc_channelize_desc;
#define PRC_CHANNELIZE_DESC_SIZE_680 40u
#define PRC_CHANNELIZE_MAX_CHAN 256
#define PRC_CHANNELIZE_MAX_SEL 64
#define PRC_CHANNELIZE_TILE_MAX_BYTES 163840   /* the LDS of a CU: a larger tile runs the direct form */
int prc_channelize(const prc_channelize_desc* desc, const float* taps, const void* twiddles, const int32_t* channels, const void* x,
                   int64_t n, void* out, int64_t out_stride, void* stream);

/* ---- exact cross-ambiguity patches ("zoom") and sub-cell peak refinement ------------------------------------------------ */
/* The un-decimated cross-ambiguity function on small lag x Doppler patches placed anywhere, at any Doppler spacing.  For a
 * frame of n samples and a patch (frame, lag0, doppler0):
 *   X[d][l] = sum_{i < n} w[i] ref[i] conj(srv[idx(i + lag0 + l)]) exp(+j 2 pi (doppler0 + d doppler_step) i / sample_rate),
 *   d < ndoppler, l < nlags;  wrap = 1: idx(m) = m mod n (true modulus, negative lags allowed: the np.roll convention of
 *   fast_xambg);  wrap = 0: terms with m outside [0, n) are dropped (the convention of prc_xcorr / direct_xambg).
 * An echo srv[i] = ref[i - D] exp(+j 2 pi f i / Fs) peaks at lag D, Doppler +f (direct_xambg's row sense, the mirror of
 * fast_xambg's rows); cell (row, col) of a fast_xambg surface is lag R - col, Doppler (F/2 - row) / CPI.
 * ref, srv: DEVICE complex64, frame b at element b * frame_stride; window: DEVICE float32[n] shared by the frames, or NULL;
 * patches: DEVICE prc_patch[npatches] (a detector can write it on the device; nothing returns to the host);
 * out: DEVICE complex64 [npatches][ndoppler][nlags].
 * Arithmetic: the phase is exact -- no float32 ramp over i.  A workgroup takes 1024-sample tiles of one (patch, 64 lags --
 * 16 when nlags <= 32 --, 16 Dopplers); inside a tile every 16 samples are one float32 Horner run acc = acc conj(z) + p over the lag product p, and
 * each run is rotated by a phasor whose argument frac(f i / Fs) was reduced in float64; runs add in float32 inside a tile,
 * tiles in float64; the per-workgroup sums go to `workspace` and a second kernel adds them in float64 in a fixed order and
 * rounds to complex64 once.  No atomics: two calls give the same bits, whatever the workspace held.  Error <= 1e-6 of
 * ||w ref||_2 ||srv||_2 (DESIGN.md section 17 has the measured figures).
 * A patch whose frame is outside [0, nframes), whose |lag0| >= n or whose doppler0 is not finite is skipped on the device:
 * its cells are written as zeros and nothing is read for it.
 * Memory: frame b of ref / srv is read only inside [b * frame_stride, b * frame_stride + n), the window inside [0, n), the
 * npatches records of the list; every cell of out is written and nothing else is, but the workspace
 * (prc_xambg_patch_workspace_bytes bytes, DEVICE, 16-byte aligned, not shared by calls in flight).
 * prc_xambg_patch_peaks, one wavefront per patch: the argmax of |X|^2 (float64 from the stored complex64 cells; the first
 * cell in [d][l] order wins ties), then along each axis a 3-point parabola on |X|: off = (y- - y+) / (2 (y- - 2 y0 + y+)),
 * clamped to +-1/2, 0 when the denominator is 0; lag = lag0 + l + off_l, doppler = doppler0 + (d + off_d) doppler_step.
 * flags: bit 0 = the argmax is on a Doppler edge of the patch (d = 0 or ndoppler - 1): no Doppler interpolation; bit 1 = the
 * same for the lag axis; bit 2 = a flat patch (all |X|^2 equal, dead air included): cell (0, 0), offsets 0, never a NaN.
 * Two kernels (patch) / one kernel (peaks) on `stream`; neither allocates, copies nor synchronises (both can be captured).
 * PRC_EINVAL: a bad descriptor header, null pointers (window excepted), n < 1, nframes < 1, frame_stride < n with more than
 * one frame, nlags outside 1 .. 1024, ndoppler outside 1 .. 4096, wrap not 0 / 1, a sample_rate or doppler_step that is not
 * finite, sample_rate == 0, npatches < 0.  npatches == 0 is a no-op.  (prc_xambg_patch_peaks reads only nlags, ndoppler and
 * doppler_step of the descriptor.)  prc_xambg_patch_workspace_bytes is host arithmetic and needs no device. */
typedef struct prc_patch_desc {
    uint32_t struct_size;  /* sizeof(prc_patch_desc) as the host compiled it (see Conventions)             */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int64_t n;             /* samples per frame                                                       */
    int64_t frame_stride;  /* elements between frames of ref / srv (>= n when nframes > 1)            */
    int32_t nframes;       /* frames in the stack                                                     */
    int32_t nlags;         /* 1 .. 1024 lags per patch                                                */
    int32_t ndoppler;      /* 1 .. 4096 Doppler rows per patch                                        */
    int32_t wrap;          /* 1: circular lags (fast_xambg), 0: terms outside the frame dropped       */
    double sample_rate;    /* Hz                                                                      */
    double doppler_step;   /* Hz between Doppler rows of a patch                                      */
} prc_patch_desc;
#define PRC_PATCH_DESC_SIZE_680 56u
#define PRC_PATCH_MAX_LAGS 1024
#define PRC_PATCH_MAX_DOPPLER 4096
typedef struct prc_patch {       /* 16 bytes */
    int32_t frame;         /* index into the stack                                                    */
    int32_t lag0;          /* lag of column 0, samples, |lag0| < n                                    */
    double doppler0;       /* Doppler of row 0, Hz                                                    */
} prc_patch;
typedef struct prc_patch_peak {  /* 32 bytes */
    double lag;            /* samples, sub-cell                                                       */
    double doppler;        /* Hz, sub-cell                                                            */
    float amplitude;       /* |X| at the argmax cell                                                  */
    int32_t d, l;          /* the argmax cell                                                         */
    uint32_t flags;        /* bit 0: Doppler edge, bit 1: lag edge, bit 2: flat patch                 */
} prc_patch_peak;
int prc_xambg_patch_workspace_bytes(const prc_patch_desc* desc, int32_t npatches, size_t* bytes);
int prc_xambg_patch(const prc_patch_desc* desc, const void* ref, const void* srv, const float* window /* or NULL */,
                    const prc_patch* patches, int32_t npatches, void* out, void* workspace, void* stream);
int prc_xambg_patch_peaks(const prc_patch_desc* desc, const prc_patch* patches, int32_t npatches, const void* X,
                          prc_patch_peak* peaks, void* stream);

/* ---- joint least-squares removal of strong echoes (CLEAN on the surveillance stream) ------------------------------------ */
/* A strong moving echo of a noise-like illuminator puts a pedestal 1 / sqrt(B T) below its peak under the whole range-Doppler
 * surface; this entry point estimates such echoes jointly and subtracts them from the surveillance stream.  For frame b there
 * are K = counts[b] atoms (lag D_k, Doppler f_k), in the echo convention of prc_xambg_patch (an echo that
 * prc_xambg_patch_peaks reports at (lag, doppler) is atom (round(lag), doppler)):
 *   a_k[i] = ref[idx(i - D_k)] exp(+j 2 pi f_k i / sample_rate),  i < n;
 *   wrap = 1: idx(m) = m mod n (true modulus, negative lags allowed);  wrap = 0: a_k[i] = 0 where i - D_k is outside [0, n);
 *   ramp = 1 adds the Doppler-slope column s_k[i] = (i / n - 1/2) a_k[i].
 * Columns A = [a_0, s_0, a_1, s_1, ...], C = (1 + ramp) K of them.  G = A^H A + reg I and g = A^H srv are accumulated in
 * float64 (the columns themselves are formed in float32), c = G^-1 g by Cholesky in float64.  One refinement (ramp = 1):
 *   f_k <- f_k + clamp(Im(c_s,k / c_a,k) / (2 pi), +-1/2) sample_rate / n,
 * skipped for an atom whose c_a is zero or not finite (dead air).  refine = R: R refinements, then the final fit (R + 1 Gram and
 * solve passes); then out = srv - A c, rounded to complex64.
 * ref, srv: DEVICE complex64, frame b at element b * frame_stride; out: DEVICE complex64, frame b at b * out_stride;
 * atoms: DEVICE prc_echo_atom [nframes][max_atoms] with counts: DEVICE int32 [nframes] (the capacity layout of prc_plots: a
 * detector can write the list on the device); a count outside 0 .. max_atoms is read as clipped; the list is never written.
 * An atom with |lag| >= n or a Doppler that is not finite is skipped (flag bit 0): the frame is fitted as if it were not listed.
 * fit: DEVICE prc_echo_fit [nframes][max_atoms], record j for atom j: the refined Doppler, c_a, c_s (0 without ramp) and flags
 * (bit 0: skipped, bit 1: a refinement was clamped, bit 2: the frame's solve broke down); records from counts[b] on are zero.
 * info: DEVICE int32 [nframes]: 0, or 1 when a Cholesky pivot was <= 0 -- in float64: not above 2^-40 of its own diagonal entry
 * of G -- or not finite, or a coefficient was not finite (duplicate atoms, or a silent reference, with reg = 0): that frame's
 * out = srv, its fits are zero with bit 2 set.  A frame without a valid atom gets out = srv bit for bit.
 * Every fit record and every info entry is written.
 * Arithmetic: the phase is exact -- the argument frac(f i0 / sample_rate) of every run of 16 samples is reduced in float64, a
 * 16-entry table per atom (from float64) covers the run; no float32 ramp over i.  Partial Gram sums go to `workspace`
 * (prc_echo_cancel_workspace_bytes bytes, DEVICE, 16-byte aligned, not shared by calls in flight) and are added in a fixed
 * order: no atomics, two calls give the same bits, whatever the workspace held.  3 (refine + 1) + 2 kernels on `stream`;
 * neither allocates, copies nor synchronises (the call can be captured).  DESIGN.md section 22 has the measured errors.
 * Memory: frame b of ref / srv is read only inside [b * frame_stride, b * frame_stride + n), the first min(counts[b], max_atoms)
 * records of frame b's atoms; out is written only inside [b * out_stride, b * out_stride + n).  out must not overlap ref or srv.
 * PRC_EINVAL: a bad descriptor header, null pointers, n < 1, nframes < 1, frame_stride or out_stride below n with more than one
 * frame, max_atoms outside 1 .. PRC_ECHO_MAX_ATOMS, refine outside 0 .. PRC_ECHO_MAX_REFINE, wrap or ramp not 0 / 1, refine > 0
 * with ramp = 0, a negative or non-finite reg, a sample_rate that is zero or not finite, a workspace that is not 16-byte aligned.
 * PRC_ESHAPE: n >= 2^31 or more than 65535 frames.  prc_echo_cancel_workspace_bytes is host arithmetic and needs no device. */
#define PRC_ECHO_MAX_ATOMS 32
#define PRC_ECHO_MAX_REFINE 8
typedef struct prc_echo_desc {
    uint32_t struct_size;  /* sizeof(prc_echo_desc) as the host compiled it (see Conventions)              */
    uint32_t magic;        /* PRC_DESC_MAGIC                                                          */
    int64_t n;             /* samples per frame                                                       */
    int64_t frame_stride;  /* elements between frames of ref / srv (>= n when nframes > 1)            */
    int64_t out_stride;    /* elements between frames of out (>= n when nframes > 1)                  */
    int32_t nframes;       /* frames in the stack                                                     */
    int32_t max_atoms;     /* 1 .. PRC_ECHO_MAX_ATOMS records per frame in atoms / fit                */
    int32_t wrap;          /* 1: circular lags, 0: samples outside the frame are zero                 */
    int32_t ramp;          /* 1: a Doppler-slope column beside every atom                             */
    int32_t refine;        /* 0 .. PRC_ECHO_MAX_REFINE Doppler refinements before the final fit (needs ramp) */
    int32_t reserved;      /* 0                                                                       */
    double sample_rate;    /* Hz                                                                      */
    double reg;            /* >= 0, added to the diagonal of G                                        */
} prc_echo_desc;
#define PRC_ECHO_DESC_SIZE_MIN 72u
typedef struct prc_echo_atom {   /* 16 bytes */
    int32_t lag;           /* samples, |lag| < n                                                      */
    int32_t reserved;
    double doppler;        /* Hz                                                                      */
} prc_echo_atom;
typedef struct prc_echo_fit {    /* 48 bytes */
    double doppler;        /* Hz, after the refinements                                               */
    double amp[2];         /* c_a (re, im)                                                            */
    double slope[2];       /* c_s (re, im); 0 without ramp                                            */
    uint32_t flags;        /* bit 0: skipped, bit 1: a refinement was clamped, bit 2: the solve broke down */
    uint32_t reserved;
} prc_echo_fit;
int prc_echo_cancel_workspace_bytes(const prc_echo_desc* desc, size_t* bytes);
int prc_echo_cancel(const prc_echo_desc* desc, const void* ref, const void* srv, const prc_echo_atom* atoms, const int32_t* counts,
                    void* out, prc_echo_fit* fit, int32_t* info, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRCORE_H */
