// Order statistics for one workgroup: the pieces the display limits, the tracker's threshold, plot extraction and OS-CFAR
// share -- order-preserving keys, the radix digit plan, the histogram scan that finds a rank's bin, NumPy's percentile rank
// and _lerp, and a whole-workgroup bitonic sort.  The pass loops that fill the histograms stay in their units (display.hip
// sweeps two ranks at once with ballot-merged adds, track.hip selects under a predicate): they differ on purpose.
#pragma once
#include "common.h"

#include <math.h>

// ---- order-preserving keys: a < b as floats <=> key(a) < key(b) as unsigned integers (NaNs are just keys: those with the
// sign bit clear sort above +Inf).  prc_okey_raw keeps -0 below +0; prc_okey takes -0 as +0 first, so a rank inside a run of
// zeros of either sign is one key, as np.sort / np.percentile see one value.  Everything that ranks VALUES uses prc_okey;
// cfar_os.hip uses prc_okey_raw, because its noise output is the selected key turned back and may have to be -0. ----
__host__ __device__ __forceinline__ uint32_t prc_okey_bits(uint32_t b) {
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ unsigned long long prc_okey_bits(unsigned long long b) {
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ uint32_t prc_okey_raw(float v) { return prc_okey_bits(__builtin_bit_cast(uint32_t, v)); }
__host__ __device__ __forceinline__ unsigned long long prc_okey_raw(double v) {
    return prc_okey_bits(__builtin_bit_cast(unsigned long long, v));
}
__host__ __device__ __forceinline__ uint32_t prc_okey(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    return prc_okey_bits(b == 0x80000000u ? 0u : b);
}
__host__ __device__ __forceinline__ unsigned long long prc_okey(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return prc_okey_bits(b == 0x8000000000000000ull ? 0ull : b);
}
__host__ __device__ __forceinline__ float prc_key_value(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__host__ __device__ __forceinline__ double prc_key_value(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// ---- radix digit plan of a select: digits of at most 11 bits (PRC_RADIX_BINS histogram bins), most significant first ----
constexpr int PRC_RADIX_BINS = 2048;
template <typename T> struct PrcKeyOf;
template <> struct PrcKeyOf<float> {
    typedef uint32_t type;
    static constexpr int passes = 3;
    static constexpr int shift(int p) { return p == 0 ? 21 : (p == 1 ? 10 : 0); }
    static constexpr int width(int p) { return p == 2 ? 10 : 11; }
};
template <> struct PrcKeyOf<double> {
    typedef unsigned long long type;
    static constexpr int passes = 6;
    static constexpr int shift(int p) { return p == 5 ? 0 : 53 - 11 * p; }
    static constexpr int width(int p) { return p == 5 ? 9 : 11; }
};
typedef PrcKeyOf<float> PrcKeys32;      // the plan of any 32-bit key (track.hip also selects on flat indices with it)

// In histogram hist[0..nb), find the bin holding rank r (0-based, ascending): thread t owns bins 2t, 2t+1.  For a
// workgroup of 1024 threads and nb <= 2048; wave_tot: 16 words of LDS scratch (one per wavefront).  Leaves bin, (count
// below it), (count in it) in sel[0..2]; ends with a barrier.
__device__ inline void prc_resolve_digit(const uint32_t* hist, int nb, uint32_t r, uint32_t* wave_tot, uint32_t* sel) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t h0 = 2 * tid < nb ? hist[2 * tid] : 0u;
    const uint32_t h1 = 2 * tid + 1 < nb ? hist[2 * tid + 1] : 0u;
    uint32_t inc = h0 + h1;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o, PRC_WAVE);
        if (lane >= o) inc += y;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int q = 0; q < wv; ++q) before += wave_tot[q];
    const uint32_t excl = before + inc - (h0 + h1);
    if (r >= excl && r < excl + h0) {
        sel[0] = 2 * tid; sel[1] = excl; sel[2] = h0;
    } else if (r >= excl + h0 && r < excl + h0 + h1) {
        sel[0] = 2 * tid + 1; sel[1] = excl + h0; sel[2] = h1;
    }
    __syncthreads();
}

// numpy's _lerp: every operation rounded on its own
__device__ __forceinline__ double prc_np_lerp(double a, double b, double t) {
    const double d = __dsub_rn(b, a);
    return t >= 0.5 ? __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t))) : __dadd_rn(a, __dmul_rn(d, t));
}

// numpy's linear percentile (host): q = p / 100, virtual index (n-1) q, its floor k and fraction t; at or above the last
// index both order statistics are the last one
inline void prc_percentile_rank(double p, uint32_t n, uint32_t* k, double* t) {
    const double q = p / 100.0;
    const double vi = (double)(n - 1) * q;
    if (vi >= (double)(n - 1)) {
        *k = n - 1;
        *t = 0.0;
    } else {
        const double fl = floor(vi);
        *k = (uint32_t)fl;
        *t = vi - fl;
    }
}

// bitonic sort of K[0..P) (P a power of two) by the whole workgroup of NT threads, ascending or descending, V (or nullptr)
// carried along.  Global: K and V are in global memory, and __threadfence goes before the barrier that ends every phase.
template <int NT, bool Global, bool Desc>
__device__ void prc_bitonic(unsigned long long* K, uint32_t* V, uint32_t P) {
    for (unsigned long long k = 2; k <= P; k <<= 1) {
        for (uint32_t j = (uint32_t)(k >> 1); j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += NT) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const unsigned long long u = K[i], w = K[l];
                    const bool first = (i & k) == 0;
                    const bool swap = Desc ? (first ? (u < w) : (u > w)) : (first ? (u > w) : (u < w));
                    if (swap) {
                        K[i] = w; K[l] = u;
                        if (V) { const uint32_t t = V[i]; V[i] = V[l]; V[l] = t; }
                    }
                }
            }
            if (Global) __threadfence();
            __syncthreads();
        }
    }
}
