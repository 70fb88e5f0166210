// The rest of signal_utils.py on device: decimate (:11-13: scipy.signal.decimate(x, q, 20 q, ftype='fir'), zero phase, zero
// padding), channel_preprocessing (:80-85: deinterleave_IQ -> frequency_shift -> decimate in ONE launch), shift (:34-47)
// and normalize (:7-9).
//
// prc_fir_decimate: y[j] = sum_k h[k] xt[j q + half - k], half = (ntaps - 1) / 2, xt = the converted (and, with mix, rotated)
// samples, zero outside [0, n).  Two forms, chosen from q and ntaps alone:
//
//   TILE (ntaps == 20 q + 1, 2 <= q <= PRC_FIRDEC_TILE_MAX_Q = 59): one wavefront per workgroup computes FD_TO = 256
//   consecutive outputs of one channel.  The (256 + 20) q samples the tile needs are loaded with consecutive lanes on
//   consecutive samples (eight unconditional loads in flight per lane), converted and rotated ONCE, and written to LDS
//   phase-major: X_p[m] = xt[m q - p], p < q, so that
//     y[j] = sum_{p < q} sum_i h[i q + p] X_p[j + 10 - i]        (i = 0 .. 19, and i = 20 for p = 0),
//   q short filters at the output rate whose taps h[i q + p] are wave-uniform (scalar loads, used straight from SGPRs by
//   v_pk_fma_f32 on the (re, im) pair).  A lane owns FD_R = 4 consecutive outputs and reads, per phase, the 24 entries
//   X_p[j0 - 10 .. j0 + 13] they share into registers: 24 LDS entries per 4 x 20 packed multiply-adds, requested one
//   phase ahead of their use.  Row entry m lives at m + (m >> 2) -- one float2 of padding per lane's four -- so that lane
//   l reads at float2 index 5 l + const: 32 distinct even banks per 32-lane group of an 8-byte read, no conflict (a
//   sample-major tile read at stride q would be a many-way conflict for every even q).  A row is 345 float2 (odd, so the
//   staging writes of consecutive lanes, one row apart, spread over the banks): 2760 q bytes per tile, 27 KB at q = 10 (five
//   workgroups per CU); q = 59 is the last q whose tile fits the 160 KiB of a CU.  The halo a tile recomputes is 20 q of
//   its 276 q samples.  (Measured against this: two float2 of padding per four, rows of 414, so that a lane's entries are
//   aligned pairs read by ds_read_b128 instead of the ds_read2_b64 the compiler makes of these -- 3312 q bytes, four
//   workgroups per CU at q = 10, 18 % slower on the complex64 stream and 17 % on int8 with rotation.)
//
//   DIRECT (everything else: q >= 60, q = 1, or another odd ntaps): one wavefront per output, lane l takes taps
//   l, l + 64, ... (consecutive lanes on consecutive samples, descending), each lane sums its own terms in order and a
//   fixed xor tree (32, 16, 8, 4, 2, 1) adds the lanes.  Every sample is converted (and rotated) once per output it
//   reaches, 20 times as often as in the tile form, which is why the tile form runs as far as its tile fits.
//
// Both sum in float32 with fused multiply-adds in one fixed order and use no atomics: two calls give the same bits.
// Sample indices are int64 throughout (a 600 s int8 recording is 2.88 GB); the per-tile index that is divided by q is below
// 276 * 59 and uses a 32-bit reciprocal.
#include "common.h"

#include <math.h>

namespace {

constexpr int FD_T = 64;                         // one wavefront per workgroup
constexpr int FD_R = 4;                          // consecutive outputs per lane
constexpr int FD_TO = FD_T * FD_R;               // outputs per tile
constexpr int FD_HALF = 10;                      // (ntaps - 1) / (2 q) of decimate's filter
constexpr int FD_PER = 2 * FD_HALF;              // taps per phase (one more for phase 0)
constexpr int FD_M = FD_TO + FD_PER;             // entries per phase row
constexpr int FD_WIN = FD_R + FD_PER;            // entries of a row one lane reads
__host__ __device__ constexpr int fd_pad(int m) { return m + (m >> 2); }
constexpr int FD_ROW = 345;                      // float2 per row: fd_pad(FD_M - 1) + 1 = 344, made odd
static_assert(fd_pad(FD_M - 1) + 1 <= FD_ROW && (FD_ROW & 1), "row length");
static_assert((size_t)PRC_FIRDEC_TILE_MAX_Q * FD_ROW * sizeof(float2) <= 160 * 1024, "the largest tile fits the LDS of a CU");
static_assert((size_t)(PRC_FIRDEC_TILE_MAX_Q + 1) * FD_ROW * sizeof(float2) > 160 * 1024, "PRC_FIRDEC_TILE_MAX_Q is the last q that fits");

constexpr int FD_DIRECT_T = 256;                 // direct form: four wavefronts, one output each per round
constexpr int64_t FD_DIRECT_MAX_WGS = 1 << 20;

typedef float fd_v2f __attribute__((ext_vector_type(2)));

struct FirdecArgs {
    const void* x;
    const float* taps;
    float2* out;
    int64_t n, n_out;          // samples and outputs per channel
    int64_t step, stride;      // complex elements
    int64_t out_step, out_stride;
    int32_t q, ntaps;
    uint32_t qinv;             // ceil(2^32 / q): floor(u / q) == umulhi(u, qinv) for u q < 2^32
    PhaseRamp pr;
};

template <int SRC>
__device__ __forceinline__ float2 fd_load(const void* base, int64_t e) {
    if (SRC == PRC_RAW_I8) {
        const signed char* p = (const signed char*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (SRC == PRC_RAW_U8) {
        const unsigned char* p = (const unsigned char*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (SRC == PRC_RAW_I16) {
        const short* p = (const short*)base + 2 * e;
        return make_float2((float)p[0], (float)p[1]);
    } else if (SRC == PRC_RAW_F32) {
        const float* p = (const float*)base + 2 * e;
        return make_float2(p[0], p[1]);
    } else {
        return ((const float2*)base)[e];
    }
}

// xt[i] of one channel: zero outside [0, n), else the converted sample, rotated as prc_frequency_shift rotates it.  The load
// itself is unconditional, from the nearest sample inside [0, n): a batch of them issues back to back, with no branch between.
template <int SRC, bool ROT>
__device__ __forceinline__ float2 fd_sample(const FirdecArgs& a, int64_t chan, int64_t i) {
    const bool inside = i >= 0 && i < a.n;
    const int64_t ic = i < 0 ? 0 : (i < a.n ? i : a.n - 1);
    float2 v = fd_load<SRC>(a.x, chan + ic * a.step);
    if (ROT) v = cmul(v, phase_rot(a.pr, ic));
    return inside ? v : make_float2(0.f, 0.f);
}

// one phase of the tile form: the 24 row entries a lane's four outputs share, and the phase's 20 wave-uniform taps
struct FdPhase {
    fd_v2f w[FD_WIN];
    float h[FD_PER];
};
__device__ __forceinline__ void fd_phase_load(FdPhase& f, const fd_v2f* row, const float* hp, int q) {
#pragma unroll
    for (int c = 0; c < FD_WIN; ++c) f.w[c] = row[c + (c >> 2)];
#pragma unroll
    for (int i = 0; i < FD_PER; ++i) f.h[i] = hp[i * q];
}
__device__ __forceinline__ void fd_phase_mac(fd_v2f (&acc)[FD_R], const FdPhase& f) {
#pragma unroll
    for (int i = 0; i < FD_PER; ++i)
#pragma unroll
        for (int r = 0; r < FD_R; ++r) acc[r] = __builtin_elementwise_fma((fd_v2f)(f.h[i]), f.w[r + FD_PER - i], acc[r]);
}

template <int SRC, bool ROT>
__global__ __launch_bounds__(FD_T) void firdec_tile_kernel(FirdecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 fd_lds[];
    const int lane = threadIdx.x;
    const int q = a.q;
    const int64_t j0 = (int64_t)blockIdx.x * FD_TO;          // first output of the tile
    const int64_t chan = (int64_t)blockIdx.y * a.stride;

    // row entry mm of phase p holds xt[(j0 - 10 + mm) q - p]: the tile's samples are the contiguous run from `first`
    const int64_t first = (j0 - FD_HALF) * q - (q - 1);
    const int total = FD_M * q;
#pragma unroll 8
    for (int u = lane; u < total; u += FD_T) {
        const float2 v = fd_sample<SRC, ROT>(a, chan, first + u);
        const int mm = (int)__umulhi((unsigned)u, a.qinv);   // u / q
        const int p = q - 1 - (u - mm * q);
        fd_lds[p * FD_ROW + fd_pad(mm)] = v;
    }
    __syncthreads();

    // (re, im) pairs on the packed-f32 multiply-add: one v_pk_fma_f32 per tap and output, each half an IEEE fma
    fd_v2f acc[FD_R];
#pragma unroll
    for (int r = 0; r < FD_R; ++r) acc[r] = (fd_v2f)(0.f);
    // output j0 + 4 lane + r, tap i of phase p: row entry 4 lane + r + 20 - i, at fd_pad(.) = 5 lane + c + (c >> 2), c = r + 20 - i
    // phases two at a time: the row entries and taps of the next phase are requested before the multiply-adds of this one
    // start (registers A and B in turn), so neither the LDS nor the scalar loads are waited for
    const fd_v2f* row = (const fd_v2f*)fd_lds + 5 * lane;
    const float* hp = a.taps;
    const float hlast = hp[FD_PER * q];                      // h[20 q]: the 21st tap of phase 0
    FdPhase A, B;
    fd_phase_load(A, row, hp, q);
    for (int p = 0; p < q; p += 2, row += 2 * FD_ROW, hp += 2) {
        const bool two = p + 1 < q;
        if (two) fd_phase_load(B, row + FD_ROW, hp + 1, q);
        fd_phase_mac(acc, A);
        if (p == 0) {
#pragma unroll
            for (int r = 0; r < FD_R; ++r) acc[r] = __builtin_elementwise_fma((fd_v2f)(hlast), A.w[r], acc[r]);
        }
        if (two) {
            if (p + 2 < q) fd_phase_load(A, row + 2 * FD_ROW, hp + 2, q);
            fd_phase_mac(acc, B);
        }
    }
    float2* out = a.out + (int64_t)blockIdx.y * a.out_stride;
#pragma unroll
    for (int r = 0; r < FD_R; ++r) {
        const int64_t j = j0 + FD_R * lane + r;
        if (j < a.n_out) out[j * a.out_step] = make_float2(acc[r].x, acc[r].y);
    }
}

template <int SRC, bool ROT>
__global__ __launch_bounds__(FD_DIRECT_T) void firdec_direct_kernel(FirdecArgs a) {
    const int lane = threadIdx.x & (PRC_WAVE - 1);
    const int64_t waves = (int64_t)gridDim.x * (FD_DIRECT_T / PRC_WAVE);
    const int64_t chan = (int64_t)blockIdx.y * a.stride;
    float2* out = a.out + (int64_t)blockIdx.y * a.out_stride;
    const int half = (a.ntaps - 1) / 2;
    for (int64_t j = (int64_t)blockIdx.x * (FD_DIRECT_T / PRC_WAVE) + (threadIdx.x / PRC_WAVE); j < a.n_out; j += waves) {
        const int64_t top = j * a.q + half;                  // the sample tap 0 meets
        float2 s = make_float2(0.f, 0.f);
        for (int k = lane; k < a.ntaps; k += PRC_WAVE) {
            const float2 v = fd_sample<SRC, ROT>(a, chan, top - k);
            const float h = a.taps[k];
            s.x = fmaf(h, v.x, s.x);
            s.y = fmaf(h, v.y, s.y);
        }
#pragma unroll
        for (int off = PRC_WAVE / 2; off > 0; off >>= 1) {   // every lane ends with the same sum
            s.x += __shfl_xor(s.x, off);
            s.y += __shfl_xor(s.y, off);
        }
        if (lane == 0) out[j * a.out_step] = s;
    }
}

template <int SRC, bool ROT>
int firdec_launch(const FirdecArgs& a, bool tile, int32_t nch, hipStream_t st) {
    if (tile) {
        const size_t lds = sizeof(float2) * (size_t)FD_ROW * (size_t)a.q;
        { int rc_ = prc_lds_optin(reinterpret_cast<const void*>(&firdec_tile_kernel<SRC, ROT>), (int)lds); if (rc_) return rc_; }
        const int64_t tiles = ceil_div64(a.n_out, FD_TO);
        hipLaunchKernelGGL((firdec_tile_kernel<SRC, ROT>), dim3((uint32_t)tiles, (uint32_t)nch), dim3(FD_T), lds, st, a);
    } else {
        int64_t wgs = ceil_div64(a.n_out, FD_DIRECT_T / PRC_WAVE);
        if (wgs > FD_DIRECT_MAX_WGS) wgs = FD_DIRECT_MAX_WGS;
        hipLaunchKernelGGL((firdec_direct_kernel<SRC, ROT>), dim3((uint32_t)wgs, (uint32_t)nch), dim3(FD_DIRECT_T), 0, st, a);
    }
    return PRC_OK;
}

template <bool ROT>
int firdec_dispatch(int dtype, const FirdecArgs& a, bool tile, int32_t nch, hipStream_t st) {
    switch (dtype) {
        case PRC_RAW_I8: return firdec_launch<PRC_RAW_I8, ROT>(a, tile, nch, st);
        case PRC_RAW_U8: return firdec_launch<PRC_RAW_U8, ROT>(a, tile, nch, st);
        case PRC_RAW_I16: return firdec_launch<PRC_RAW_I16, ROT>(a, tile, nch, st);
        case PRC_RAW_F32: return firdec_launch<PRC_RAW_F32, ROT>(a, tile, nch, st);
        default: return firdec_launch<PRC_RAW_C64, ROT>(a, tile, nch, st);
    }
}

// ---- shift: a flat copy at an offset of whole rows, zeros where nothing arrives -------------------------------------
template <class V>
__global__ __launch_bounds__(256) void shift_kernel(const V* __restrict__ x, V* __restrict__ y, int64_t total, int64_t off) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t s = i - off;
        V v = {};
        if (s >= 0 && s < total) v = x[s];
        y[i] = v;
    }
}

template <class V>
void shift_launch(const void* x, void* y, int64_t bytes, int64_t off_bytes, hipStream_t st) {
    const int64_t total = bytes / (int64_t)sizeof(V), off = off_bytes / (int64_t)sizeof(V);
    int64_t wgs = ceil_div64(total, 256);
    if (wgs > 8192) wgs = 8192;
    hipLaunchKernelGGL(shift_kernel<V>, dim3((uint32_t)wgs), dim3(256), 0, st, (const V*)x, (V*)y, total, off);
}

// ---- normalize: y = x / mean|x| -----------------------------------------------------------------------------------------
constexpr int NZ_T = 256;
constexpr int64_t NZ_PER_WG = 8192;      // a workgroup sums at least this many elements ...
constexpr int64_t NZ_MAX_WGS = 256;      // ... and there are at most this many (one per lane of the final sum)

int64_t normalize_wgs(int64_t n) {
    int64_t w = ceil_div64(n, NZ_PER_WG);
    return w > NZ_MAX_WGS ? NZ_MAX_WGS : (w < 1 ? 1 : w);
}

// a fixed tree over the workgroup's 256 values; the result is in red[0]
__device__ __forceinline__ void nz_tree(double* red, int tid) {
    __syncthreads();
    for (int o = NZ_T / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
}

template <bool CPLX>
__global__ __launch_bounds__(NZ_T) void normalize_sum_kernel(const void* __restrict__ x, int64_t n, int64_t chunk, double* __restrict__ partials) {
    __shared__ double red[NZ_T];
    const int tid = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    int64_t hi = lo + chunk;
    if (hi > n) hi = n;
    double s = 0.0;
    for (int64_t i = lo + tid; i < hi; i += NZ_T) {
        if (CPLX) {
            const float2 v = ((const float2*)x)[i];
            s += (double)hypotf(v.x, v.y);
        } else {
            s += (double)fabsf(((const float*)x)[i]);
        }
    }
    red[tid] = s;
    nz_tree(red, tid);
    if (tid == 0) partials[blockIdx.x] = red[0];
}

template <bool CPLX>
__global__ __launch_bounds__(NZ_T) void normalize_scale_kernel(const void* x, void* y, int64_t n, const double* __restrict__ partials,
                                                               int nparts) {
    __shared__ double red[NZ_T];
    const int tid = threadIdx.x;
    red[tid] = tid < nparts ? partials[tid] : 0.0;
    nz_tree(red, tid);
    const float mean = (float)(red[0] / (double)n);
    const int64_t stride = (int64_t)gridDim.x * NZ_T;
    for (int64_t i = (int64_t)blockIdx.x * NZ_T + tid; i < n; i += stride) {
        if (CPLX) {
            const float2 v = ((const float2*)x)[i];
            ((float2*)y)[i] = make_float2(v.x / mean, v.y / mean);
        } else {
            ((float*)y)[i] = ((const float*)x)[i] / mean;
        }
    }
}

}  // namespace

extern "C" int prc_fir_decimate(const prc_firdec_desc* desc, const float* taps, const void* x, int64_t n, int64_t step,
                                int64_t stride, int32_t nch, void* out, int64_t out_step, int64_t out_stride, void* stream) {
    PRC_RANGE("prc_fir_decimate");
    static_assert(sizeof(prc_firdec_desc) == PRC_FIRDEC_DESC_SIZE_660, "prc_firdec_desc grew: keep PRC_FIRDEC_DESC_SIZE_660, default the new fields to 0");
    PRC_REQUIRE(desc, PRC_EINVAL, "prc_fir_decimate: null descriptor");
    prc_firdec_desc d;
    if (int rc = prc_take_desc(&d, desc, PRC_FIRDEC_DESC_SIZE_660, "prc_fir_decimate", "prc_firdec_desc")) return rc;
    PRC_REQUIRE(d.q >= 1, PRC_EINVAL, "prc_fir_decimate: q = %d", d.q);
    PRC_REQUIRE(d.ntaps >= 1 && (d.ntaps & 1), PRC_EINVAL, "prc_fir_decimate: ntaps = %d: not a positive odd number", d.ntaps);
    PRC_REQUIRE(d.ntaps < (1 << 24), PRC_ESHAPE, "prc_fir_decimate: ntaps = %d: 2^24 or more", d.ntaps);
    PRC_REQUIRE(d.raw_dtype >= PRC_RAW_I8 && d.raw_dtype <= PRC_RAW_C64, PRC_EINVAL, "prc_fir_decimate: raw_dtype = %d: not a prc_raw_dtype",
                d.raw_dtype);
    PRC_REQUIRE(d.mix == 0 || d.mix == 1, PRC_EINVAL, "prc_fir_decimate: mix = %d: not 0 or 1", d.mix);
    PRC_REQUIRE(!d.mix || d.fs != 0.0, PRC_EINVAL, "prc_fir_decimate: fs = 0 with mix");
    PRC_REQUIRE(n >= 0, PRC_EINVAL, "prc_fir_decimate: n = %lld", (long long)n);
    PRC_REQUIRE(step >= 1 && out_step >= 1, PRC_EINVAL, "prc_fir_decimate: step = %lld, out_step = %lld", (long long)step, (long long)out_step);
    PRC_REQUIRE(nch >= 1 && nch <= 65535, PRC_EINVAL, "prc_fir_decimate: nch = %d: not in 1 .. 65535", nch);
    PRC_REQUIRE(nch == 1 || (stride >= 0 && out_stride >= 0), PRC_EINVAL, "prc_fir_decimate: stride = %lld, out_stride = %lld",
                (long long)stride, (long long)out_stride);
    PRC_REQUIRE(taps && x && out, PRC_EINVAL, "prc_fir_decimate: null argument");
    PRC_REQUIRE(((uintptr_t)out & 7u) == 0 && ((uintptr_t)taps & 3u) == 0, PRC_EINVAL, "prc_fir_decimate: out needs 8-byte, taps 4-byte alignment");
    if (n == 0) return PRC_OK;

    FirdecArgs a;
    a.x = x;
    a.taps = taps;
    a.out = (float2*)out;
    a.n = n;
    a.n_out = ceil_div64(n, d.q);
    a.step = step;
    a.stride = stride;
    a.out_step = out_step;
    a.out_stride = out_stride;
    a.q = d.q;
    a.ntaps = d.ntaps;
    a.qinv = d.q >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)d.q - 1) / (uint64_t)d.q) : 0u;
    // the ramp of prc_frequency_shift (ls.hip, make_ramp), enabled whatever fc is
    a.pr.a32 = (float)(2.0 * 3.14159265358979323846 * d.fc);
    a.pr.rcp32 = d.mix ? 1.0f / (float)d.fs : 0.f;
    a.pr.off32 = (float)d.phase_offset;
    a.pr.enabled = d.mix;
    const bool tile = d.q >= 2 && d.q <= PRC_FIRDEC_TILE_MAX_Q && (int64_t)d.ntaps == (int64_t)FD_PER * d.q + 1;
    PRC_REQUIRE(!tile || ceil_div64(a.n_out, FD_TO) <= (int64_t)0x7fffffff, PRC_EUNSUPPORTED,
                "prc_fir_decimate: %lld outputs are more than one launch takes", (long long)a.n_out);
    const int rc = d.mix ? firdec_dispatch<true>(d.raw_dtype, a, tile, nch, (hipStream_t)stream)
                         : firdec_dispatch<false>(d.raw_dtype, a, tile, nch, (hipStream_t)stream);
    if (rc != PRC_OK) return rc;
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

extern "C" int prc_shift(const void* x, void* y, int64_t rows, int64_t row_bytes, int64_t shift, void* stream) {
    PRC_RANGE("prc_shift");
    PRC_REQUIRE(x && y, PRC_EINVAL, "prc_shift: null argument");
    PRC_REQUIRE(rows >= 0 && row_bytes >= 1, PRC_EINVAL, "prc_shift: rows = %lld, row_bytes = %lld", (long long)rows, (long long)row_bytes);
    PRC_REQUIRE(row_bytes <= (int64_t)1 << 40 && rows <= ((int64_t)1 << 62) / row_bytes, PRC_EINVAL, "prc_shift: rows * row_bytes overflows");
    if (rows == 0) return PRC_OK;
    if (shift > rows) shift = rows;
    if (shift < -rows) shift = -rows;
    const int64_t bytes = rows * row_bytes, off = shift * row_bytes;
    hipStream_t st = (hipStream_t)stream;
    // the widest unit that divides the row and both addresses (the offset is whole rows, so it divides that too)
    const uintptr_t low = (uintptr_t)x | (uintptr_t)y | (uintptr_t)row_bytes;
    if ((low & 15u) == 0) shift_launch<prc_v4u>(x, y, bytes, off, st);
    else if ((low & 7u) == 0) shift_launch<prc_v2u>(x, y, bytes, off, st);
    else if ((low & 3u) == 0) shift_launch<uint32_t>(x, y, bytes, off, st);
    else if ((low & 1u) == 0) shift_launch<uint16_t>(x, y, bytes, off, st);
    else shift_launch<uint8_t>(x, y, bytes, off, st);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

extern "C" int prc_normalize_workspace_bytes(int64_t n, size_t* bytes) {
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_normalize_workspace_bytes: null argument");
    PRC_REQUIRE(n >= 1, PRC_EINVAL, "prc_normalize_workspace_bytes: n = %lld", (long long)n);
    *bytes = sizeof(double) * (size_t)normalize_wgs(n);
    return PRC_OK;
}

extern "C" int prc_normalize(const void* x, void* y, int64_t n, int32_t is_complex, void* workspace, void* stream) {
    PRC_RANGE("prc_normalize");
    PRC_REQUIRE(x && y && workspace, PRC_EINVAL, "prc_normalize: null argument");
    PRC_REQUIRE(n >= 1, PRC_EINVAL, "prc_normalize: n = %lld", (long long)n);
    PRC_REQUIRE(is_complex == 0 || is_complex == 1, PRC_EINVAL, "prc_normalize: is_complex = %d", is_complex);
    PRC_REQUIRE(((uintptr_t)workspace & 7u) == 0, PRC_EINVAL, "prc_normalize: workspace needs 8-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const int64_t wgs = normalize_wgs(n);
    const int64_t chunk = ceil_div64(n, wgs);
    double* partials = (double*)workspace;
    int64_t swgs = ceil_div64(n, NZ_T * 4);
    if (swgs > 4096) swgs = 4096;
    if (is_complex) {
        hipLaunchKernelGGL(normalize_sum_kernel<true>, dim3((uint32_t)wgs), dim3(NZ_T), 0, st, x, n, chunk, partials);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(normalize_scale_kernel<true>, dim3((uint32_t)swgs), dim3(NZ_T), 0, st, x, y, n, partials, (int)wgs);
    } else {
        hipLaunchKernelGGL(normalize_sum_kernel<false>, dim3((uint32_t)wgs), dim3(NZ_T), 0, st, x, n, chunk, partials);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(normalize_scale_kernel<false>, dim3((uint32_t)swgs), dim3(NZ_T), 0, st, x, y, n, partials, (int)wgs);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
