// Display frames on device: what range_doppler_plot.py:72-92 (and multitarget_kalman_tracker.py:100-120) does to every
// persistence frame before it reaches the screen:
//
//   vmn = np.percentile(data, 35); vmx = 1.5 * np.percentile(data, 99); imshow(data, cmap='gnuplot2', vmin=vmn, vmax=vmx)
//
// prc_display_limits: one 1024-thread workgroup per frame finds BOTH order statistics x(k_lo), x(k_hi) exactly by radix
// select on order-preserving keys (64-bit keys and six 11-bit digit passes for float64 frames, 32-bit keys and three
// passes for float32), two histograms in LDS filled in the same sweep, so a frame is read once per pass and not once per
// rank; then the successors x(k+1) (one more sweep, only when a run of ties does not already cover k+1) and NumPy's _lerp
// with every operation rounded on its own.  The successor is taken even when the fraction t is 0: NumPy forms
// a + (b - a) * 0 all the same, which is NaN when b - a is not finite (a frame holding +Inf).
//
// prc_display_rgba: matplotlib's Normalize + Colormap.__call__ per cell in float64, colours from a 256-entry table that
// travels in the kernel arguments and is held in LDS.  In the "plot" orientation (s = fliplr(data.T)) the transpose goes
// through an LDS tile: the reads run along W, the 4-byte writes along H.
#include "common.h"
#include "order_select.h"
#include "wave.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int DT = 1024;            // threads per limits workgroup
constexpr int DW = DT / PRC_WAVE;   // its wavefronts
constexpr int NBINS = PRC_RADIX_BINS;
constexpr uint32_t NONE = 0xffffffffu;

struct LimitsArgs {
    uint32_t n;             // elements per frame (< 2^31)
    uint32_t k[2];          // numpy's floor(q (n-1)) per rank (n-1 at or above the last index)
    double t[2];            // its fraction
    double hi_scale;
    double* limits;         // [nframes][2]
};

struct LimitsLds {
    uint32_t hist[2][NBINS];
    unsigned long long kred[2][DW];
    uint32_t ured[DW];
    uint32_t sel[2][3];
    uint32_t nan;
};

// hist[d] += 1 for every lane with d != NONE.  The top digit of a key is the sign and most of the exponent, and a rank
// inside a run of ties meets one digit in every pass: lanes that share a digit are counted by a ballot and added once
// (three rounds), what is left goes one atomic per lane.  Called by whole wavefronts.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t d) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(d != NONE);
    for (int it = 0; it < 3 && todo; ++it) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t dl = (uint32_t)__shfl((int)d, leader, PRC_WAVE);
        const unsigned long long m = __ballot(d == dl);
        if (lane == leader) atomicAdd(&h[dl], (uint32_t)__popcll(m));
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[d], 1u);
}

template <typename T>
__global__ __launch_bounds__(DT) void display_limits_kernel(const T* __restrict__ frames, LimitsArgs a) {
    typedef typename PrcKeyOf<T>::type K;
    __shared__ LimitsLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T* x = frames + (size_t)blockIdx.x * (size_t)a.n;
    double* out = a.limits + 2 * (size_t)blockIdx.x;

    K prefix[2] = {0, 0}, pmask = 0;
    uint32_t r[2] = {a.k[0], a.k[1]}, less[2] = {0u, 0u}, eq[2] = {0u, 0u};
    for (int p = 0; p < PrcKeyOf<T>::passes; ++p) {
        const int shift = PrcKeyOf<T>::shift(p), nb = 1 << PrcKeyOf<T>::width(p);
        const uint32_t dm = (uint32_t)nb - 1u;
        for (int b = tid; b < 2 * NBINS; b += DT) (&L.hist[0][0])[b] = 0u;
        if (p == 0 && tid == 0) L.nan = 0u;
        __syncthreads();
        const bool same = prefix[0] == prefix[1];      // the two ranks share every digit so far: one histogram serves both
        for (uint32_t base = 0; base < a.n; base += DT) {
            const uint32_t i = base + tid;
            uint32_t d0 = NONE, d1 = NONE;
            if (i < a.n) {
                const T v = x[i];
                if (p == 0 && v != v) L.nan = 1u;
                const K key = prc_okey(v);
                const uint32_t digit = (uint32_t)(key >> shift) & dm;
                if ((key & pmask) == prefix[0]) d0 = digit;
                if (!same && (key & pmask) == prefix[1]) d1 = digit;
            }
            hist_add(L.hist[0], d0);
            if (!same) hist_add(L.hist[1], d1);
        }
        __syncthreads();
        if (p == 0 && L.nan) {                         // numpy sorts NaN last and returns it for every percentile
            if (tid == 0) { out[0] = __longlong_as_double(0x7ff8000000000000ll); out[1] = out[0]; }
            return;
        }
        prc_resolve_digit(L.hist[0], nb, r[0], L.ured, L.sel[0]);
        prc_resolve_digit(same ? L.hist[0] : L.hist[1], nb, r[1], L.ured, L.sel[1]);
        for (int j = 0; j < 2; ++j) {
            const uint32_t bin = L.sel[j][0], bef = L.sel[j][1];
            eq[j] = L.sel[j][2];
            prefix[j] |= (K)bin << shift;
            r[j] -= bef;
            less[j] += bef;
        }
        pmask |= (K)dm << shift;
        __syncthreads();
    }

    // x(k+1): x(k) again when its run of ties reaches k+1 (or k is the last index), else the smallest key above
    bool need[2];
    for (int j = 0; j < 2; ++j) need[j] = a.k[j] + 1u < a.n && less[j] + eq[j] <= a.k[j] + 1u;
    K succ[2] = {prefix[0], prefix[1]};
    if (need[0] || need[1]) {
        const K top = ~(K)0;
        K m0 = top, m1 = top;
        for (uint32_t i = tid; i < a.n; i += DT) {
            const K key = prc_okey(x[i]);
            if (key > prefix[0] && key < m0) m0 = key;
            if (key > prefix[1] && key < m1) m1 = key;
        }
        m0 = (K)wave_min((unsigned long long)m0);
        m1 = (K)wave_min((unsigned long long)m1);
        if (lane == 0) { L.kred[0][wv] = m0; L.kred[1][wv] = m1; }
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < 2; ++j) {
                unsigned long long m = ~0ull;
                for (int q = 0; q < DW; ++q) m = L.kred[j][q] < m ? L.kred[j][q] : m;
                if (need[j]) succ[j] = (K)m;
            }
        }
    }
    if (tid == 0) {
        const double lo = prc_np_lerp((double)prc_key_value(prefix[0]), (double)prc_key_value(succ[0]), a.t[0]);
        const double hi = prc_np_lerp((double)prc_key_value(prefix[1]), (double)prc_key_value(succ[1]), a.t[1]);
        out[0] = lo;
        out[1] = __dmul_rn(a.hi_scale, hi);
    }
}

// ---------------------------------------------------------------------------------------------------------------
constexpr int CT = 256;         // threads per colour workgroup
constexpr int TILE_W = 32;      // "plot" tile: cells along W (read direction) ...
constexpr int TILE_C = 64;      // ... and along H (write direction)

struct RgbaArgs {
    int32_t H, W, nframes;
    const double* limits;
    uint32_t* out;              // one RGBA pixel per element
    uint32_t lut[256];          // r | g << 8 | b << 16 | a << 24
};

// Normalize(vmin, vmax) then Colormap.__call__ for a float64 value: three separately rounded operations, then the
// under / over / bad rules.  Unordered limits (matplotlib raises) give the bad colour for the whole frame.
struct Mapper {
    double vmin, den;
    int mode;                   // 0: map, 1: every pixel lut[0] (vmin == vmax), 2: every pixel bad (vmin > vmax)
    __device__ Mapper(double lo, double hi) : vmin(lo), den(__dsub_rn(hi, lo)), mode(lo > hi ? 2 : (lo == hi ? 1 : 0)) {}
    __device__ __forceinline__ uint32_t operator()(double v, const uint32_t* lut) const {
        if (mode) return mode == 1 ? lut[0] : 0u;
        const double xa = __dmul_rn(__ddiv_rn(__dsub_rn(v, vmin), den), 256.0);
        if (xa != xa) return 0u;
        if (xa < 0.0) return lut[0];
        if (xa >= 256.0) return lut[255];
        return lut[(int)xa];
    }
};

template <typename T>
__global__ __launch_bounds__(CT) void display_rgba_stored_kernel(const T* __restrict__ frames, RgbaArgs a) {
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = a.lut[threadIdx.x];
    __syncthreads();
    const size_t n = (size_t)a.H * (size_t)a.W;
    const size_t e = (size_t)blockIdx.x * CT + threadIdx.x;
    if (e >= n) return;
    for (int f = blockIdx.y; f < a.nframes; f += gridDim.y) {
        const Mapper map(a.limits[2 * (size_t)f], a.limits[2 * (size_t)f + 1]);
        a.out[(size_t)f * n + e] = map((double)frames[(size_t)f * n + e], lut);
    }
}

// out[r][c] = colour(data[H-1-c][r]): a tile of TILE_W range cells x TILE_C Doppler cells
template <typename T>
__global__ __launch_bounds__(CT) void display_rgba_plot_kernel(const T* __restrict__ frames, RgbaArgs a) {
    __shared__ uint32_t lut[256];
    __shared__ uint32_t tile[TILE_W][TILE_C + 1];
    const int tid = threadIdx.x;
    lut[tid] = a.lut[tid];
    const int tiles_w = (a.W + TILE_W - 1) / TILE_W;
    const int w0 = (int)(blockIdx.x % (uint32_t)tiles_w) * TILE_W;
    const int c0 = (int)(blockIdx.x / (uint32_t)tiles_w) * TILE_C;
    const size_t n = (size_t)a.H * (size_t)a.W;
    for (int f = blockIdx.y; f < a.nframes; f += gridDim.y) {
        __syncthreads();        // the table is there; the tile of the frame before has been read
        const Mapper map(a.limits[2 * (size_t)f], a.limits[2 * (size_t)f + 1]);
        const T* x = frames + (size_t)f * n;
        {
            const int lw = tid & (TILE_W - 1), w = w0 + lw;
            for (int lc = tid / TILE_W; lc < TILE_C; lc += CT / TILE_W) {
                const int c = c0 + lc;
                if (w < a.W && c < a.H) tile[lw][lc] = map((double)x[(size_t)(a.H - 1 - c) * a.W + w], lut);
            }
        }
        __syncthreads();
        {
            const int lc = tid & (TILE_C - 1), c = c0 + lc;
            for (int lw = tid / TILE_C; lw < TILE_W; lw += CT / TILE_C) {
                const int w = w0 + lw;
                if (w < a.W && c < a.H) a.out[(size_t)f * n + (size_t)w * a.H + c] = tile[lw][lc];
            }
        }
    }
}

// gnuplot2 from its closed form at x = np.linspace(0, 1, 256) (arange * step + start, the last point set to stop),
// clipped to [0, 1], as (lut * 255).astype(uint8); alpha 255
void gnuplot2_table(uint32_t* lut) {
    const double step = 1.0 / 255.0;
    for (int i = 0; i < 256; ++i) {
        const double x = i == 255 ? 1.0 : (double)i * step + 0.0;
        double c[3];
        c[0] = x / 0.32 - 0.78125;
        c[1] = 2.0 * x - 0.84;
        c[2] = x < 0.25 ? 4.0 * x : (x < 0.92 ? -2.0 * x + 1.84 : x / 0.08 - 11.5);
        uint32_t px = 0xff000000u;
        for (int j = 0; j < 3; ++j) {
            const double v = c[j] < 0.0 ? 0.0 : (c[j] > 1.0 ? 1.0 : c[j]);
            px |= (uint32_t)(uint8_t)(v * 255.0) << (8 * j);
        }
        lut[i] = px;
    }
}

}  // namespace

extern "C" int prc_display_limits(const void* frames, int32_t dtype, int64_t frame_elems, int32_t nframes, double p_lo,
                                  double p_hi, double hi_scale, double* limits, void* stream) {
    PRC_RANGE("prc_display_limits");
    PRC_REQUIRE(dtype == PRC_REAL_F32 || dtype == PRC_REAL_F64, PRC_EINVAL,
                "prc_display_limits: dtype = %d: not PRC_REAL_F32 (0) or PRC_REAL_F64 (1)", dtype);
    PRC_REQUIRE(p_lo >= 0.0 && p_lo <= 100.0 && p_hi >= 0.0 && p_hi <= 100.0, PRC_EINVAL,
                "prc_display_limits: p_lo = %g, p_hi = %g: not in [0, 100]", p_lo, p_hi);
    PRC_REQUIRE(frame_elems >= 1 && frame_elems <= (int64_t)0x7fffffff, PRC_EINVAL,
                "prc_display_limits: frame_elems = %lld, not in [1, 2^31)", (long long)frame_elems);
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_display_limits: nframes = %d", nframes);
    PRC_REQUIRE(frames && limits, PRC_EINVAL, "prc_display_limits: null argument");
    if (nframes == 0) return PRC_OK;
    LimitsArgs a;
    a.n = (uint32_t)frame_elems;
    prc_percentile_rank(p_lo, a.n, &a.k[0], &a.t[0]);
    prc_percentile_rank(p_hi, a.n, &a.k[1], &a.t[1]);
    a.hi_scale = hi_scale;
    a.limits = limits;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PRC_REAL_F32)
        hipLaunchKernelGGL(display_limits_kernel<float>, dim3(nframes), dim3(DT), 0, st, (const float*)frames, a);
    else
        hipLaunchKernelGGL(display_limits_kernel<double>, dim3(nframes), dim3(DT), 0, st, (const double*)frames, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

extern "C" int prc_display_rgba(const void* frames, int32_t dtype, int32_t H, int32_t W, int32_t nframes,
                                const double* limits, const uint8_t* lut_host, int32_t orient, uint8_t* out,
                                void* stream) {
    PRC_RANGE("prc_display_rgba");
    PRC_REQUIRE(dtype == PRC_REAL_F32 || dtype == PRC_REAL_F64, PRC_EINVAL,
                "prc_display_rgba: dtype = %d: not PRC_REAL_F32 (0) or PRC_REAL_F64 (1)", dtype);
    PRC_REQUIRE(orient == PRC_DISPLAY_PLOT || orient == PRC_DISPLAY_STORED, PRC_EINVAL,
                "prc_display_rgba: orient = %d: not PRC_DISPLAY_PLOT (0) or PRC_DISPLAY_STORED (1)", orient);
    PRC_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)0x7fffffff, PRC_EINVAL,
                "prc_display_rgba: H = %d, W = %d: not >= 1 with H * W < 2^31", H, W);
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_display_rgba: nframes = %d", nframes);
    PRC_REQUIRE(frames && limits && out, PRC_EINVAL, "prc_display_rgba: null argument");
    PRC_REQUIRE(((uintptr_t)out & 3u) == 0, PRC_EINVAL, "prc_display_rgba: out is not aligned to a pixel (4 bytes)");
    if (nframes == 0) return PRC_OK;
    RgbaArgs a;
    a.H = H;
    a.W = W;
    a.nframes = nframes;
    a.limits = limits;
    a.out = reinterpret_cast<uint32_t*>(out);
    if (lut_host) {
        for (int i = 0; i < 256; ++i)
            a.lut[i] = (uint32_t)lut_host[4 * i] | (uint32_t)lut_host[4 * i + 1] << 8 |
                       (uint32_t)lut_host[4 * i + 2] << 16 | (uint32_t)lut_host[4 * i + 3] << 24;
    } else {
        gnuplot2_table(a.lut);
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t gy = (uint32_t)(nframes < 65535 ? nframes : 65535);
    if (orient == PRC_DISPLAY_STORED) {
        const dim3 grid((uint32_t)ceil_div64((int64_t)H * W, CT), gy);
        if (dtype == PRC_REAL_F32)
            hipLaunchKernelGGL(display_rgba_stored_kernel<float>, grid, dim3(CT), 0, st, (const float*)frames, a);
        else
            hipLaunchKernelGGL(display_rgba_stored_kernel<double>, grid, dim3(CT), 0, st, (const double*)frames, a);
    } else {
        const dim3 grid((uint32_t)(ceil_div64(W, TILE_W) * ceil_div64(H, TILE_C)), gy);
        if (dtype == PRC_REAL_F32)
            hipLaunchKernelGGL(display_rgba_plot_kernel<float>, grid, dim3(CT), 0, st, (const float*)frames, a);
        else
            hipLaunchKernelGGL(display_rgba_plot_kernel<double>, grid, dim3(CT), 0, st, (const double*)frames, a);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
