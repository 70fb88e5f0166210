// Welch spectra on device: matplotlib.mlab.psd / csd / specgram for complex input (sides='twosided', pad_to == NFFT), the
// four plt.psd calls of signal_preview.py:51-54, 68-71 and the time-resolved form of the same average.
//
// prc_welch enqueues three kernels on the caller's stream and nothing else:
//   1. welch_twiddle_kernel: W_N^k = exp(-2 pi i k / N), k < N, float64 sincospi rounded once to float32, into the head of
//      the caller's workspace (no plan, no library-owned table, nothing to synchronise).
//   2. welch_kernel<LOG2N, CSD>: one workgroup takes a run of consecutive segments of one output row.  Per segment: the
//      samples are converted while they are loaded (raw int8 / uint8 / int16 / float32 pairs or complex64, any `step`),
//      detrended (float64 mean), windowed and written to LDS; the transform is an in-place decimation-in-frequency
//      radix-4 (one leading radix-2 stage for odd log2 N) held in LDS, whose LAST radix-4 stage stays in registers:
//      |X|^2 (or conj(X) Y) is formed there in float64 and added to float64 accumulators that live in registers for the
//      whole run.  Windowed segments and spectra never leave the CU.  The run's sums go to the workspace in the
//      transform's own (digit-reversed) order, 32 contiguous bytes per thread.
//   3. welch_reduce_kernel: one workgroup per output row and component adds the row's partials in workgroup order, applies
//      mean and scale in float64, undoes the digit reversal and folds np.roll(., -N/2) into an LDS index, and writes the
//      row with contiguous stores.
// How a row's segments are split over workgroups depends on the arguments alone (welch_split), the sums have one order,
// and there is no atomic: two calls give the same bits.
//
// LDS image: element p of the segment lives at p + (p >> 5) (one float2 of padding per 32), which keeps the stride-4 and
// stride-1 exchanges of the last stages off each other's banks; (N + N / 32) * 8 bytes, 66 KB at N = 8192, two
// workgroups per CU.
#include "common.h"

#include <math.h>

namespace {

constexpr int WT = 256;                  // threads per workgroup at N >= 1024 (N / 4 below)
constexpr int64_t WELCH_RUN = 16;         // a row's segments go to workgroups in runs of at least this many ...
constexpr int64_t WELCH_MAX_WGS = 1024;   // ... and to at most this many workgroups

struct WelchArgs {
    const void* x;
    const void* y;
    const float* window;
    const float2* tw;       // W_N^k, k < N
    double* partials;       // [nch][rows][W][ncomp][N], transform order
    int64_t n, stride, hop; // samples per channel, channel stride (complex elements), nfft - noverlap
    int64_t spr;            // segments per row
    int64_t rows;
    int64_t chunk;          // segments per workgroup
    int32_t W;              // workgroups per row
    int32_t step, detrend, dtype;
};

struct Split {
    int64_t chunk, W;
};
// Segments per workgroup and workgroups per row: a function of the row's segment count ALONE, so a batch of channels or
// rows sums exactly as single calls do.  A run of 16 segments amortises the 8 N bytes a workgroup leaves in the workspace
// over at least 32 N bytes of int8 input.
Split welch_split(int64_t spr) {
    int64_t W = ceil_div64(spr, WELCH_RUN);
    if (W > WELCH_MAX_WGS) W = WELCH_MAX_WGS;
    Split s;
    s.chunk = ceil_div64(spr, W);
    s.W = ceil_div64(spr, s.chunk);
    return s;
}

__device__ __forceinline__ int ph(int p) { return p + (p >> 5); }
// threads per workgroup and last-stage butterflies per thread at N = 2^l
constexpr int welch_threads(int l) { return (1 << l) / 4 < WT ? (1 << l) / 4 : WT; }
constexpr int welch_jb(int l) { return (1 << l) / 4 / welch_threads(l); }

template <int DT>
__device__ __forceinline__ float2 welch_sample(const void* base, int64_t e) {
    if (DT == PRC_RAW_I8) {
        const signed char* p = (const signed char*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (DT == PRC_RAW_U8) {
        const unsigned char* p = (const unsigned char*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (DT == PRC_RAW_I16) {
        const short* p = (const short*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (DT == PRC_RAW_F32) {
        const float* p = (const float*)base + 2 * e;
        return make_float2(p[0], p[1]);
    } else {
        return ((const float2*)base)[e];
    }
}

// Samples first + tid + j T of one channel (zero from n on, as mlab pads a short input) into the LDS image, windowed on the
// way when no mean has to come off first; returns the thread's float64 sum of what it loaded.  One scalar branch per segment.
template <int DT, int PER, int T>
__device__ __forceinline__ double2 welch_load(float2* lds, const WelchArgs& a, const void* base, int64_t chan, int64_t first,
                                              int tid) {
    double2 s = make_double2(0.0, 0.0);
#pragma unroll 4
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * T;
        const int64_t g = first + i;
        float2 v = g < a.n ? welch_sample<DT>(base, chan + g * a.step) : make_float2(0.f, 0.f);
        if (a.detrend) {
            s.x += (double)v.x;
            s.y += (double)v.y;
        } else {
            const float w = a.window[i];
            v = make_float2(v.x * w, v.y * w);
        }
        lds[ph(i)] = v;
    }
    return s;
}

// One segment: load, detrend, window, transform.  Leaves the outputs of the last radix-4 stage in r: r[j][m] is the
// element at transform position 4 (tid + j T) + m.  Called by the whole workgroup; starts with a barrier (the LDS image of
// the segment before has been read by then).
template <int LOG2N>
__device__ __forceinline__ void welch_segment(float2 (&r)[welch_jb(LOG2N)][4], const WelchArgs& a, const void* base,
                                              int64_t chan, int64_t first, float2* lds, double2* red) {
    constexpr int N = 1 << LOG2N;
    constexpr int T = welch_threads(LOG2N);
    constexpr int PER = N / T;
    constexpr int JB = welch_jb(LOG2N);
    const int tid = threadIdx.x;

    __syncthreads();
    double2 s;
    switch (a.dtype) {
        case PRC_RAW_I8: s = welch_load<PRC_RAW_I8, PER, T>(lds, a, base, chan, first, tid); break;
        case PRC_RAW_U8: s = welch_load<PRC_RAW_U8, PER, T>(lds, a, base, chan, first, tid); break;
        case PRC_RAW_I16: s = welch_load<PRC_RAW_I16, PER, T>(lds, a, base, chan, first, tid); break;
        case PRC_RAW_F32: s = welch_load<PRC_RAW_F32, PER, T>(lds, a, base, chan, first, tid); break;
        default: s = welch_load<PRC_RAW_C64, PER, T>(lds, a, base, chan, first, tid);
    }
    if (a.detrend) {
        red[tid] = s;                         // (every thread has passed a barrier since it read red[0] of the segment before)
        __syncthreads();
        for (int o = T / 2; o > 0; o >>= 1) { // a fixed tree
            if (tid < o) {
                const double2 u = red[tid + o];
                red[tid].x += u.x;
                red[tid].y += u.y;
            }
            __syncthreads();
        }
        const double mx = red[0].x * (1.0 / N), my = red[0].y * (1.0 / N);
#pragma unroll 4
        for (int j = 0; j < PER; ++j) {       // the thread's own elements: no barrier between the two passes
            const int i = tid + j * T;
            const float2 v = lds[ph(i)];
            const float w = a.window[i];
            lds[ph(i)] = make_float2((float)((double)v.x - mx) * w, (float)((double)v.y - my) * w);
        }
    }
    __syncthreads();

    int L = N;
    if (LOG2N & 1) {
        constexpr int S = N / 2;
#pragma unroll 2
        for (int j = 0; j < S / T; ++j) {
            const int b = tid + j * T;
            const float2 a0 = lds[ph(b)], a1 = lds[ph(b + S)];
            const float2 w = a.tw[b];
            lds[ph(b)] = make_float2(a0.x + a1.x, a0.y + a1.y);
            lds[ph(b + S)] = cmul(make_float2(a0.x - a1.x, a0.y - a1.y), w);
        }
        L = S;
        __syncthreads();
    }
#pragma unroll
    for (int st = 0; st < LOG2N / 2 - 1; ++st) {
        const int S = L >> 2;
        const int ts = N / L;                 // W_L = W_N^(N / L)
#pragma unroll 2
        for (int j = 0; j < JB; ++j) {
            const int b = tid + j * T;
            const int off = b & (S - 1);
            const int p0 = (b - off) * 4 + off;
            const float2 a0 = lds[ph(p0)], a1 = lds[ph(p0 + S)], a2 = lds[ph(p0 + 2 * S)], a3 = lds[ph(p0 + 3 * S)];
            const float2 w1 = a.tw[off * ts], w2 = a.tw[2 * off * ts], w3 = a.tw[3 * off * ts];
            const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
            const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
            lds[ph(p0)] = make_float2(t0.x + t2.x, t0.y + t2.y);
            lds[ph(p0 + S)] = cmul(make_float2(t1.x + t3.y, t1.y - t3.x), w1);
            lds[ph(p0 + 2 * S)] = cmul(make_float2(t0.x - t2.x, t0.y - t2.y), w2);
            lds[ph(p0 + 3 * S)] = cmul(make_float2(t1.x - t3.y, t1.y + t3.x), w3);
        }
        L = S;
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < JB; ++j) {
        const int p0 = 4 * (tid + j * T);
        const float2 a0 = lds[ph(p0)], a1 = lds[ph(p0 + 1)], a2 = lds[ph(p0 + 2)], a3 = lds[ph(p0 + 3)];
        const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y), t3 = make_float2(a1.x - a3.x, a1.y - a3.y);
        r[j][0] = make_float2(t0.x + t2.x, t0.y + t2.y);
        r[j][1] = make_float2(t1.x + t3.y, t1.y - t3.x);
        r[j][2] = make_float2(t0.x - t2.x, t0.y - t2.y);
        r[j][3] = make_float2(t1.x - t3.y, t1.y + t3.x);
    }
}

template <int LOG2N, bool CSD>
__global__ __launch_bounds__(WT, CSD ? 1 : 2) void welch_kernel(WelchArgs a) {
    constexpr int N = 1 << LOG2N;
    constexpr int T = welch_threads(LOG2N);
    constexpr int JB = welch_jb(LOG2N);
    constexpr int NC = CSD ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) float2 welch_lds[];
    __shared__ double2 red[T];
    const int tid = threadIdx.x;

    const int64_t wg = blockIdx.x;
    const int64_t w = wg % a.W;
    const int64_t row = (wg / a.W) % a.rows;
    const int64_t c = wg / a.W / a.rows;
    const int64_t s0 = row * a.spr + w * a.chunk;
    int64_t s1 = s0 + a.chunk;
    if (s1 > (row + 1) * a.spr) s1 = (row + 1) * a.spr;
    const int64_t chan = c * a.stride;

    double acc[NC][JB][4];
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[q][j][m] = 0.0;

    for (int64_t s = s0; s < s1; ++s) {
        float2 X[JB][4];
        welch_segment<LOG2N>(X, a, a.x, chan, s * a.hop, welch_lds, red);
        if (CSD) {
            float2 Y[JB][4];
            welch_segment<LOG2N>(Y, a, a.y, chan, s * a.hop, welch_lds, red);
#pragma unroll
            for (int j = 0; j < JB; ++j)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    // float products are exact in float64: conj(X) X has a zero imaginary part and |X|^2 as its real one
                    const double xr = X[j][m].x, xi = X[j][m].y, yr = Y[j][m].x, yi = Y[j][m].y;
                    acc[0][j][m] += xr * yr + xi * yi;
                    acc[NC - 1][j][m] += xr * yi - xi * yr;
                }
        } else {
#pragma unroll
            for (int j = 0; j < JB; ++j)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const double xr = X[j][m].x, xi = X[j][m].y;
                    acc[0][j][m] += xr * xr + xi * xi;
                }
        }
    }
    double* out = a.partials + (size_t)wg * NC * N;
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int m = 0; m < 4; ++m) out[(size_t)q * N + 4 * (tid + j * T) + m] = acc[q][j][m];
}

__global__ void welch_twiddle_kernel(float2* tw, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s, c;
    sincospi(-2.0 * (double)k / (double)n, &s, &c);
    tw[k] = make_float2((float)c, (float)s);
}

// the frequency bin held at transform position p: the digit a stage resolves FIRST is the least significant of the bin
__device__ __forceinline__ int welch_bin(int p, int log2n) {
    int k = 0, mult = 1, L = 1 << log2n;
    if (log2n & 1) {
        L >>= 1;
        k += ((p / L) & 1) * mult;
        mult <<= 1;
    }
    while (L > 1) {
        L >>= 2;
        k += ((p / L) & 3) * mult;
        mult <<= 2;
    }
    return k;
}

struct ReduceArgs {
    const double* partials;
    double* out;
    int32_t log2n, W, ncomp;
    double count, scale;
};

constexpr int RT = 256;
__global__ __launch_bounds__(RT) void welch_reduce_kernel(ReduceArgs a) {
    __shared__ double line[8192];
    const int N = 1 << a.log2n;
    const size_t row = blockIdx.x;
    const int comp = blockIdx.y;
    const double* part = a.partials + (row * a.W * a.ncomp + comp) * (size_t)N;
    for (int p = threadIdx.x; p < N; p += RT) {
        double s = 0.0;
        for (int w = 0; w < a.W; ++w) s += part[(size_t)w * a.ncomp * N + p];
        const int k = welch_bin(p, a.log2n);
        line[(k + N / 2) & (N - 1)] = s / a.count * a.scale;
    }
    __syncthreads();
    double* out = a.out + row * (size_t)N * a.ncomp + comp;
    for (int c = threadIdx.x; c < N; c += RT) out[(size_t)c * a.ncomp] = line[c];
}

struct Shape {
    int log2n;
    int64_t nseg, rows, spr, count;
};

int welch_check(prc_welch_desc* d, const prc_welch_desc* desc, int64_t n, Shape* sh, const char* who) {
    PRC_REQUIRE(desc, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_WELCH_DESC_SIZE_650, who, "prc_welch_desc");
    if (rc != PRC_OK) return rc;
    int log2n = 0;
    while ((1 << log2n) < d->nfft && log2n < 14) ++log2n;
    PRC_REQUIRE(d->nfft >= 64 && d->nfft <= 8192 && (1 << log2n) == d->nfft, PRC_EINVAL,
                "%s: nfft = %d: not a power of two in 64 .. 8192", who, d->nfft);
    PRC_REQUIRE(d->noverlap >= 0 && d->noverlap < d->nfft, PRC_EINVAL, "%s: noverlap = %d: not in [0, nfft = %d)", who,
                d->noverlap, d->nfft);
    PRC_REQUIRE(d->navg >= 0, PRC_EINVAL, "%s: navg = %d", who, d->navg);
    PRC_REQUIRE(d->detrend == 0 || d->detrend == 1, PRC_EINVAL, "%s: detrend = %d: not 0 (none) or 1 (mean)", who, d->detrend);
    PRC_REQUIRE(d->in_dtype >= PRC_RAW_I8 && d->in_dtype <= PRC_RAW_C64, PRC_EINVAL, "%s: in_dtype = %d: not a prc_raw_dtype",
                who, d->in_dtype);
    PRC_REQUIRE(d->step >= 1, PRC_EINVAL, "%s: step = %d", who, d->step);
    PRC_REQUIRE(n >= 1, PRC_EINVAL, "%s: n = %lld", who, (long long)n);
    sh->log2n = log2n;
    sh->nseg = n < d->nfft ? 1 : (n - d->nfft) / (d->nfft - d->noverlap) + 1;
    PRC_REQUIRE(d->navg <= sh->nseg, PRC_ESHAPE, "%s: navg = %d exceeds the %lld segments of %lld samples", who, d->navg,
                (long long)sh->nseg, (long long)n);
    sh->rows = d->navg == 0 ? 1 : sh->nseg / d->navg;
    sh->spr = d->navg == 0 ? sh->nseg : d->navg;
    sh->count = sh->spr;
    return PRC_OK;
}

template <int LOG2N, bool CSD>
int welch_launch(const WelchArgs& a, int64_t wgs, hipStream_t st) {
    constexpr int N = 1 << LOG2N;
    constexpr int T = welch_threads(LOG2N);
    const size_t lds = sizeof(float2) * (N + N / 32);
    { int rc_ = prc_lds_optin(reinterpret_cast<const void*>(&welch_kernel<LOG2N, CSD>), (int)lds); if (rc_) return rc_; }
    hipLaunchKernelGGL((welch_kernel<LOG2N, CSD>), dim3((uint32_t)wgs), dim3(T), lds, st, a);
    return PRC_OK;
}

template <bool CSD>
int welch_dispatch(int log2n, const WelchArgs& a, int64_t wgs, hipStream_t st) {
    switch (log2n) {
        case 6: return welch_launch<6, CSD>(a, wgs, st);
        case 7: return welch_launch<7, CSD>(a, wgs, st);
        case 8: return welch_launch<8, CSD>(a, wgs, st);
        case 9: return welch_launch<9, CSD>(a, wgs, st);
        case 10: return welch_launch<10, CSD>(a, wgs, st);
        case 11: return welch_launch<11, CSD>(a, wgs, st);
        case 12: return welch_launch<12, CSD>(a, wgs, st);
        default: return welch_launch<13, CSD>(a, wgs, st);
    }
}

}  // namespace

extern "C" int prc_welch_rows(const prc_welch_desc* desc, int64_t n, int64_t* nseg, int64_t* rows) {
    prc_welch_desc d;
    Shape sh;
    const int rc = welch_check(&d, desc, n, &sh, "prc_welch_rows");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nseg && rows, PRC_EINVAL, "prc_welch_rows: null argument");
    *nseg = sh.nseg;
    *rows = sh.rows;
    return PRC_OK;
}

extern "C" int prc_welch_workspace_bytes(const prc_welch_desc* desc, int64_t n, int32_t nch, size_t* bytes) {
    prc_welch_desc d;
    Shape sh;
    const int rc = welch_check(&d, desc, n, &sh, "prc_welch_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nch >= 1, PRC_EINVAL, "prc_welch_workspace_bytes: nch = %d", nch);
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_welch_workspace_bytes: null argument");
    const Split sp = welch_split(sh.spr);
    // the twiddles, then the partial sums of a cross spectrum (two components; an auto spectrum uses the first half)
    *bytes = sizeof(float2) * (size_t)d.nfft + sizeof(double) * 2 * (size_t)d.nfft * (size_t)nch * (size_t)sh.rows * (size_t)sp.W;
    return PRC_OK;
}

extern "C" int prc_welch(const prc_welch_desc* desc, const void* x, const void* y, int64_t n, int64_t stride, int32_t nch,
                         const float* window, void* out, void* workspace, void* stream) {
    PRC_RANGE("prc_welch");
    prc_welch_desc d;
    Shape sh;
    const int rc = welch_check(&d, desc, n, &sh, "prc_welch");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nch >= 1, PRC_EINVAL, "prc_welch: nch = %d", nch);
    const int64_t nrows = (int64_t)nch * sh.rows;
    const Split sp = welch_split(sh.spr);
    const int64_t wgs = nrows * sp.W;
    PRC_REQUIRE(wgs <= (int64_t)0x7fffffff && nrows <= (int64_t)0x7fffffff, PRC_EUNSUPPORTED,
                "prc_welch: %lld output rows in %lld workgroups are more than one launch takes (limit %lld)", (long long)nrows,
                (long long)wgs, (long long)0x7fffffff);
    PRC_REQUIRE(x && window && out && workspace, PRC_EINVAL, "prc_welch: null argument");
    PRC_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)out & 7u) == 0, PRC_EINVAL,
                "prc_welch: out and workspace need 8-byte alignment");
    PRC_REQUIRE(nch == 1 || stride >= 0, PRC_EINVAL, "prc_welch: stride = %lld", (long long)stride);
    hipStream_t st = (hipStream_t)stream;
    const int N = d.nfft;
    float2* tw = (float2*)workspace;
    double* partials = (double*)((char*)workspace + sizeof(float2) * (size_t)N);
    hipLaunchKernelGGL(welch_twiddle_kernel, dim3((N + 255) / 256), dim3(256), 0, st, tw, N);
    PRC_LAUNCH_CHECK();

    WelchArgs a;
    a.x = x;
    a.y = y;
    a.window = window;
    a.tw = tw;
    a.partials = partials;
    a.n = n;
    a.stride = stride;
    a.hop = N - d.noverlap;
    a.spr = sh.spr;
    a.rows = sh.rows;
    a.chunk = sp.chunk;
    a.W = (int32_t)sp.W;
    a.step = d.step;
    a.detrend = d.detrend;
    a.dtype = d.in_dtype;
    const int rl = y ? welch_dispatch<true>(sh.log2n, a, wgs, st) : welch_dispatch<false>(sh.log2n, a, wgs, st);
    if (rl != PRC_OK) return rl;
    PRC_LAUNCH_CHECK();

    ReduceArgs r;
    r.partials = partials;
    r.out = (double*)out;
    r.log2n = sh.log2n;
    r.W = (int32_t)sp.W;
    r.ncomp = y ? 2 : 1;
    r.count = (double)sh.count;
    r.scale = d.scale;
    hipLaunchKernelGGL(welch_reduce_kernel, dim3((uint32_t)nrows, (uint32_t)r.ncomp), dim3(RT), 0, st, r);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
