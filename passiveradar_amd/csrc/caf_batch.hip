// Batches algorithm for OFDM illuminators: range-Doppler maps by a per-batch matched or RECIPROCAL filter (prc_batch_xambg),
// and the cyclic-prefix symbol timing that aligns the batches to the useful part of the symbols (prc_ofdm_timing).
//
// Per batch j (L = 1024 or 4096 samples from start + j hop of both channels, loaded once, coalesced):
//     R = FFT_L(ref batch), S = FFT_L(srv batch)                       forward transforms in registers / LDS
//     W = G conj(R) S / L,  G = 1 (matched) or 1 / max(|R|^2, floor^2 P), P = sum |ref batch|^2
//     c = conj(IFFT_L(W))                                              ONE inverse transform: every lag of the batch
//     y[j][R - d] = w[j] c[d], d = 0 .. range_bins                     tile-major slow-time buffer of the Doppler kernel
// and the column Doppler kernel of caf_doppler.hip turns y into the surface.  The pointwise step runs in the transforms'
// permuted frequency layout (both spectra of a batch sit in the same registers of the same threads), so nothing is reordered.
// L = 1024: one wavefront per batch on fft_wave.h, four batches per workgroup pass; L = 4096: one team of four wavefronts per
// batch on fft_team.h.  P is a wave (team) reduction of the time samples; a silent reference batch has max(...) = 0 and G = 0.
// No atomics, no allocation per call (the twiddle tables are the per-device copies of caf_fft.hip / caf_fft_team.hip, the
// Doppler twiddles a per-device copy kept here), one stream: capturable.
#ifndef FT_NBUF
#define FT_NBUF 1
#endif
#include "caf_internal.h"
#include "fft_team.h"
#include "doppler_col.h"
#include "wave.h"
#include <math.h>
#include <vector>

int fftw_device_tables(const float2** out);   // caf_fft.hip

namespace {

#define CB_WAVES 4            // batches (wavefronts) per workgroup pass of the 1024-point kernel
// wavefronts per SIMD the two kernels are compiled for (A/B builds)
#ifndef CB_WAVE_OCC
#define CB_WAVE_OCC 2
#endif
#ifndef CB_TEAM_OCC
#define CB_TEAM_OCC 2
#endif

struct BatchArgs {
    const float2* ref;
    const float2* srv;
    const float* window;      // float32[freq_bins] or nullptr
    float2* y;                // tile-major slow-time buffer
    const float2* tab;        // twiddle tables of the transform
    int64_t frame_stride;
    int64_t start, hop;
    int64_t y_surface;        // elements per surface of y
    int32_t range_bins, freq_bins;
    int32_t kt_shift;         // log2 of the Doppler kernel's tile width
    int32_t segs;             // consecutive batches (1024: groups of CB_WAVES batches) per workgroup
    float floor2;             // floor^2
};

// element offset of (slow-time sample j, column k) inside a surface of y: tiles of kt columns, y[k / kt][j][k % kt]
__device__ __forceinline__ int64_t cb_y_off(const BatchArgs& a, int j, int k) {
    const int sh = a.kt_shift;
    return (((int64_t)(k >> sh) * a.freq_bins + j) << sh) + (k & ((1 << sh) - 1));
}

__device__ __forceinline__ float cb_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, PRC_WAVE);
    return v;
}

// sum over a thread's 16 samples of |r|^2 (two chains of fused multiply-adds)
__device__ __forceinline__ float cb_energy16(const float2 (&u)[16]) {
    float e = 0.f, o = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        e = fmaf(u[r].x, u[r].x, e);
        e = fmaf(u[r].y, u[r].y, e);
        o = fmaf(u[r + 1].x, u[r + 1].x, o);
        o = fmaf(u[r + 1].y, u[r + 1].y, o);
    }
    return e + o;
}

// u <- G conj(u) v scale: the spectrum whose inverse transform is conj(c); fp2 = floor^2 P (reciprocal filter only)
template <bool RECIP>
__device__ __forceinline__ void cb_pointwise(float2 (&u)[16], const float2 (&v)[16], float fp2, float scale) {
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        float g = scale;
        if (RECIP) {
            const float mag = fmaxf(fmaf(u[m].x, u[m].x, u[m].y * u[m].y), fp2);
            g = mag > 0.f ? scale * (1.0f / mag) : 0.f;
        }
        const float re = fmaf(u[m].x, v[m].x, u[m].y * v[m].y);
        const float im = fmaf(u[m].x, v[m].y, -(u[m].y * v[m].x));
        u[m] = make_float2(re * g, im * g);
    }
}

template <bool RECIP>
__global__ __launch_bounds__(64 * CB_WAVES, CB_WAVE_OCC) void batch_wave_kernel(BatchArgs a) {
    __shared__ __attribute__((aligned(16))) float2 smem[FFTW_TABLE + CB_WAVES * FFTW_TILE];
    float2* tab = smem;
    const int wave_id = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float2* tile = smem + FFTW_TABLE + wave_id * FFTW_TILE;
    fft_load_tables(tab, a.tab);
    __syncthreads();
    const FftLane f = fft_lane_setup();
    const int lane = f.lane;
    const int R = a.range_bins, F = a.freq_bins;
    for (int sg = 0; sg < a.segs; ++sg) {
        const int64_t b = ((int64_t)blockIdx.x * a.segs + sg) * CB_WAVES + wave_id;   // batch over all frames (uniform)
        const int frame = (int)(b / F), j = (int)(b - (int64_t)frame * F);
        const int64_t base = (int64_t)frame * a.frame_stride + a.start + (int64_t)j * a.hop;
        const float2* __restrict__ rp = a.ref + base;
        const float2* __restrict__ sp = a.srv + base;
        float2 u[16], v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) u[r] = rp[64 * r + lane];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = sp[64 * r + lane];
        float fp2 = 0.f;
        if (RECIP) fp2 = a.floor2 * cb_wave_sum(cb_energy16(u));
        fft1024_fwd(u, tile, tab, f);
        fft1024_fwd(v, tile, tab, f);
        // the quad sign the inverse transform wants on its input rides on the filter
        cb_pointwise<RECIP>(u, v, fp2, f.sg * (1.0f / (float)FFTW_P));
        fft1024_inv<true>(u, tile, tab, f);
        const float w = a.window ? a.window[j] : 1.0f;
        float2* __restrict__ y = a.y + (int64_t)frame * a.y_surface;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lag = 64 * r + lane;
            if (lag <= R) y[cb_y_off(a, j, R - lag)] = make_float2(u[r].x * w, -u[r].y * w);
        }
    }
}

template <bool RECIP>
__global__ __launch_bounds__(FT_THREADS, CB_TEAM_OCC) void batch_team_kernel(BatchArgs a) {
    __shared__ __attribute__((aligned(16))) float2 lds[FT_LDS_ELEMS + 2];
    float* psum = reinterpret_cast<float*>(lds + FT_LDS_ELEMS);       // one partial energy per wavefront
    const FtLane f = ft_setup(lds, a.tab);
    const int t = f.t;
    const int R = a.range_bins, F = a.freq_bins;
    for (int sg = 0; sg < a.segs; ++sg) {
        const int64_t b = (int64_t)blockIdx.x * a.segs + sg;          // batch over all frames (uniform)
        const int frame = (int)(b / F), j = (int)(b - (int64_t)frame * F);
        const int64_t base = (int64_t)frame * a.frame_stride + a.start + (int64_t)j * a.hop;
        const float2* __restrict__ rp = a.ref + base;
        const float2* __restrict__ sp = a.srv + base;
        float2 u[16], v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) u[r] = rp[256 * r + t];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = sp[256 * r + t];
        float fp2 = 0.f;
        if (RECIP) {
            const float e = cb_wave_sum(cb_energy16(u));
            if ((t & 63) == 0) psum[t >> 6] = e;
            __syncthreads();
            fp2 = a.floor2 * ((psum[0] + psum[1]) + (psum[2] + psum[3]));
        }
        ft4096_fwd<0>(u, f);
        ft4096_fwd<1>(v, f);
        cb_pointwise<RECIP>(u, v, fp2, 1.0f / (float)FT_P);
        ft4096_inv<0>(u, f);
        ft_team_sync();                                               // the next batch starts at buffer 0 again (and rewrites psum)
        const float w = a.window ? a.window[j] : 1.0f;
        float2* __restrict__ y = a.y + (int64_t)frame * a.y_surface;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lag = 256 * r + t;
            if (lag <= R) y[cb_y_off(a, j, R - lag)] = make_float2(u[r].x * w, -u[r].y * w);
        }
    }
}

// ---- the Doppler kernel's W_F^m table: one device copy per (device, freq_bins), made at the first call that needs it ----
float2* g_dop_tab[16][5] = {{nullptr}};
std::mutex g_dop_mtx;

int dop_slot_of(int F) { return F == 256 ? 0 : F == 512 ? 1 : F == 1024 ? 2 : F == 2048 ? 3 : F == 4096 ? 4 : -1; }

int dop_device_table(int F, const float2** out) {
    int dev = 0;
    PRC_HIP(hipGetDevice(&dev));
    PRC_REQUIRE(dev >= 0 && dev < 16, PRC_EINVAL, "device index %d out of range", dev);
    const int s = dop_slot_of(F);
    std::lock_guard<std::mutex> lk(g_dop_mtx);
    if (!g_dop_tab[dev][s]) {
        std::vector<float2> host((size_t)F);
        dop_make_table(host.data(), F);
        float2* d = nullptr;
        PRC_HIP(hipMalloc(&d, sizeof(float2) * (size_t)F));
        const hipError_t e = hipMemcpy(d, host.data(), sizeof(float2) * (size_t)F, hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(d);
        PRC_HIP(e);
        g_dop_tab[dev][s] = d;
    }
    *out = g_dop_tab[dev][s];
    return PRC_OK;
}

// every check of a descriptor that needs no device, in the order the header documents
int check_desc(prc_batch_xambg_desc* d, const prc_batch_xambg_desc* host, const char* who) {
    static_assert(sizeof(prc_batch_xambg_desc) == PRC_BATCH_XAMBG_DESC_SIZE_MIN,
                  "prc_batch_xambg_desc grew: keep PRC_BATCH_XAMBG_DESC_SIZE_MIN, default the new fields to 0");
    PRC_REQUIRE(host, PRC_EINVAL, "%s: null descriptor", who);
    if (int rc = prc_take_desc(d, host, PRC_BATCH_XAMBG_DESC_SIZE_MIN, who, "prc_batch_xambg_desc")) return rc;
    PRC_REQUIRE(d->filter == PRC_BATCH_MATCHED || d->filter == PRC_BATCH_RECIPROCAL, PRC_EINVAL, "%s: filter = %d: not a prc_batch_filter",
                who, d->filter);
    PRC_REQUIRE(d->filter == PRC_BATCH_MATCHED || (d->floor >= 0.f && d->floor <= 3.0e38f), PRC_EINVAL,
                "%s: floor = %g: not a finite number >= 0", who, (double)d->floor);
    PRC_REQUIRE(d->batch_len == 1024 || d->batch_len == 4096, PRC_EUNSUPPORTED, "%s: batch_len = %d: this build transforms batches of 1024 or 4096 samples",
                who, d->batch_len);
    PRC_REQUIRE(dop_slot_of(d->freq_bins) >= 0, PRC_EUNSUPPORTED, "%s: freq_bins = %d: the column Doppler kernel takes 256, 512, 1024, 2048 or 4096 batches",
                who, d->freq_bins);
    PRC_REQUIRE(d->start >= 0, PRC_ESHAPE, "%s: start = %lld is negative", who, (long long)d->start);
    PRC_REQUIRE(d->hop >= 1, PRC_ESHAPE, "%s: hop = %lld: batches are at least one sample apart", who, (long long)d->hop);
    PRC_REQUIRE(d->range_bins >= 0 && d->range_bins < d->batch_len, PRC_ESHAPE, "%s: range_bins = %d: not in 0 .. batch_len - 1 = %d", who,
                d->range_bins, d->batch_len - 1);
    PRC_REQUIRE(d->n >= 1 && d->n <= PRC_CAF_MAX_N, PRC_ESHAPE, "%s: n = %lld: not in 1 .. %lld samples per frame (PRC_CAF_MAX_N)", who,
                (long long)d->n, (long long)PRC_CAF_MAX_N);
    // hop <= n keeps (freq_bins - 1) hop far inside 64 bits
    PRC_REQUIRE(d->start <= d->n && d->hop <= d->n && d->start + (int64_t)(d->freq_bins - 1) * d->hop + d->batch_len <= d->n, PRC_ESHAPE,
                "%s: the last batch ends at start + (freq_bins - 1) hop + batch_len = %lld + %d * %lld + %d, beyond n = %lld", who,
                (long long)d->start, d->freq_bins - 1, (long long)d->hop, d->batch_len, (long long)d->n);
    return PRC_OK;
}

int check_frames(const prc_batch_xambg_desc& d, int32_t nframes, const char* who) {
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "%s: nframes = %d", who, nframes);
    PRC_REQUIRE((int64_t)nframes * d.freq_bins <= PRC_BATCH_XAMBG_MAX_BATCHES, PRC_ESHAPE,
                "%s: nframes * freq_bins = %lld batches exceed the limit of %lld of one call (PRC_BATCH_XAMBG_MAX_BATCHES)", who,
                (long long)nframes * d.freq_bins, (long long)PRC_BATCH_XAMBG_MAX_BATCHES);
    return PRC_OK;
}

int64_t surface_elems(const prc_batch_xambg_desc& d) {
    const int64_t kt = dop_tile_cols(d.freq_bins), cols = d.range_bins + 1;
    return (int64_t)d.freq_bins * ((cols + kt - 1) / kt) * kt;
}

// ---- symbol timing ----
#define OT_THREADS 256

// one workgroup per candidate offset o: the cyclic-prefix correlation over nsym symbols, float32 products summed in float64
__global__ __launch_bounds__(OT_THREADS) void ofdm_metric_kernel(const float2* __restrict__ ref, int32_t nfft, int32_t cp, int32_t nsym,
                                                                 double* __restrict__ metric) {
    __shared__ double part[2][OT_THREADS / PRC_WAVE];
    const int64_t sym = (int64_t)nfft + cp, o = blockIdx.x;
    const int64_t terms = (int64_t)nsym * cp;
    double re = 0.0, im = 0.0;
    for (int64_t i = threadIdx.x; i < terms; i += OT_THREADS) {
        const int64_t s = i / cp, t = i - s * cp;
        const float2 a = ref[o + s * sym + t], b = ref[o + s * sym + t + nfft];
        // a conj(b): every product of two float32 values is exact in float64
        re += (double)a.x * (double)b.x + (double)a.y * (double)b.y;
        im += (double)a.y * (double)b.x - (double)a.x * (double)b.y;
    }
    re = wave_sum(re);
    im = wave_sum(im);
    if ((threadIdx.x & (PRC_WAVE - 1)) == 0) {
        part[0][threadIdx.x / PRC_WAVE] = re;
        part[1][threadIdx.x / PRC_WAVE] = im;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sr = 0.0, si = 0.0;
        for (int w = 0; w < OT_THREADS / PRC_WAVE; ++w) {
            sr += part[0][w];
            si += part[1][w];
        }
        metric[o] = sqrt(sr * sr + si * si);
    }
}

// one workgroup: the lowest index of the largest metric (a NaN is never larger)
__global__ __launch_bounds__(OT_THREADS) void ofdm_argmax_kernel(const double* __restrict__ metric, int32_t count, int32_t* __restrict__ start) {
    __shared__ double bv[OT_THREADS];
    __shared__ int32_t bi[OT_THREADS];
    double best = -1.0;
    int32_t at = 0;
    for (int32_t i = threadIdx.x; i < count; i += OT_THREADS) {
        const double m = metric[i];
        if (m > best) { best = m; at = i; }
    }
    bv[threadIdx.x] = best;
    bi[threadIdx.x] = at;
    __syncthreads();
    for (int s = OT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double m = bv[threadIdx.x + s];
            const int32_t i = bi[threadIdx.x + s];
            if (m > bv[threadIdx.x] || (m == bv[threadIdx.x] && i < bi[threadIdx.x])) {
                bv[threadIdx.x] = m;
                bi[threadIdx.x] = i;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *start = bi[0];
}

}  // namespace

extern "C" int prc_batch_xambg_workspace_bytes(const prc_batch_xambg_desc* desc, int32_t nframes, size_t* bytes) {
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_batch_xambg_workspace_bytes: null argument");
    *bytes = 0;
    prc_batch_xambg_desc d;
    if (int rc = check_desc(&d, desc, "prc_batch_xambg_workspace_bytes")) return rc;
    if (int rc = check_frames(d, nframes, "prc_batch_xambg_workspace_bytes")) return rc;
    *bytes = sizeof(float2) * (size_t)nframes * (size_t)surface_elems(d);
    return PRC_OK;
}

extern "C" int prc_batch_xambg(const prc_batch_xambg_desc* desc, const void* ref, const void* srv, int64_t frame_stride, const float* window,
                               void* out, int32_t nframes, void* workspace, void* stream) {
    PRC_RANGE("prc_batch_xambg");
    prc_batch_xambg_desc d;
    if (int rc = check_desc(&d, desc, "prc_batch_xambg")) return rc;
    if (int rc = check_frames(d, nframes, "prc_batch_xambg")) return rc;
    if (nframes == 0) return PRC_OK;
    PRC_REQUIRE(ref && srv && out && workspace, PRC_EINVAL, "prc_batch_xambg: null argument");
    PRC_REQUIRE((((uintptr_t)ref | (uintptr_t)srv | (uintptr_t)out | (uintptr_t)workspace) & 7u) == 0 && ((uintptr_t)window & 3u) == 0, PRC_EINVAL,
                "prc_batch_xambg: ref, srv, out and workspace need 8-byte, window 4-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const int F = d.freq_bins, kt = dop_tile_cols(F);
    BatchArgs a;
    a.ref = (const float2*)ref;
    a.srv = (const float2*)srv;
    a.window = window;
    a.y = (float2*)workspace;
    a.frame_stride = frame_stride;
    a.start = d.start;
    a.hop = d.hop;
    a.y_surface = surface_elems(d);
    a.range_bins = d.range_bins;
    a.freq_bins = F;
    a.kt_shift = 31 - __builtin_clz((unsigned)kt);
    a.floor2 = d.floor * d.floor;
    const float2* dop_tw = nullptr;
    if (int rc = dop_device_table(F, &dop_tw)) return rc;
    const int64_t total = (int64_t)nframes * F;                        // a multiple of 256
    // several batches per workgroup amortise the table set-up once there is plenty of work
    a.segs = total >= 16384 ? 4 : (total >= 4096 ? 2 : 1);
    const bool recip = d.filter == PRC_BATCH_RECIPROCAL;
    if (d.batch_len == 1024) {
        if (int rc = fftw_device_tables(&a.tab)) return rc;
        const dim3 grid((unsigned)(total / (CB_WAVES * a.segs)));
        if (recip) hipLaunchKernelGGL((batch_wave_kernel<true>), grid, dim3(64 * CB_WAVES), 0, st, a);
        else hipLaunchKernelGGL((batch_wave_kernel<false>), grid, dim3(64 * CB_WAVES), 0, st, a);
    } else {
        if (int rc = ft_device_tables(&a.tab)) return rc;
        const dim3 grid((unsigned)(total / a.segs));
        if (recip) hipLaunchKernelGGL((batch_team_kernel<true>), grid, dim3(FT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((batch_team_kernel<false>), grid, dim3(FT_THREADS), 0, st, a);
    }
    PRC_LAUNCH_CHECK();
    return dop_launch(a.y, a.y_surface, (float2*)out, dop_tw, F, d.range_bins + 1, nframes, st);
}

extern "C" int prc_ofdm_timing(const void* ref, int64_t n, int32_t nfft, int32_t cp, int32_t nsym, double* metric_out, int32_t* start_out,
                               void* stream) {
    PRC_RANGE("prc_ofdm_timing");
    PRC_REQUIRE(nfft >= 2 && cp >= 1 && cp < nfft && nsym >= 1, PRC_EINVAL, "prc_ofdm_timing: nfft = %d, cp = %d, nsym = %d: nfft >= 2, 1 <= cp < nfft, nsym >= 1",
                nfft, cp, nsym);
    const int64_t sym = (int64_t)nfft + cp;
    PRC_REQUIRE(sym <= 0x7fffffff, PRC_ESHAPE, "prc_ofdm_timing: nfft + cp = %lld candidate offsets exceed 2^31 - 1", (long long)sym);
    PRC_REQUIRE(n >= 0 && ((int64_t)nsym + 1) * sym + nfft <= n, PRC_ESHAPE,
                "prc_ofdm_timing: (nsym + 1) (nfft + cp) + nfft = %lld samples are needed, n = %lld", (long long)(((int64_t)nsym + 1) * sym + nfft),
                (long long)n);
    PRC_REQUIRE(ref && metric_out && start_out, PRC_EINVAL, "prc_ofdm_timing: null argument");
    PRC_REQUIRE(((uintptr_t)ref & 7u) == 0 && ((uintptr_t)metric_out & 7u) == 0 && ((uintptr_t)start_out & 3u) == 0, PRC_EINVAL,
                "prc_ofdm_timing: ref and metric_out need 8-byte, start_out 4-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ofdm_metric_kernel, dim3((unsigned)sym), dim3(OT_THREADS), 0, st, (const float2*)ref, nfft, cp, nsym, metric_out);
    hipLaunchKernelGGL(ofdm_argmax_kernel, dim3(1), dim3(OT_THREADS), 0, st, (const double*)metric_out, (int32_t)sym, start_out);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
