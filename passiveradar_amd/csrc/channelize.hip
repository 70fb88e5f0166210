// Uniform polyphase filter bank: K of M channels centred at k Fs / M, decimated by D, out of ONE pass over the raw samples.
//
//   y[i][j] = sum_{t < L} h[t] x[j D + c - t] w^((k_i (start + j D + c - t)) mod M),   w = exp(-2 pi i / M),  c = (L - 1) / 2,
//
// x zero outside [0, n), j < ceil(n / D).  With t = i M + p the exponent splits into k (start + j D + c) - k p (mod M):
//
//   y[k][j] = w^(k (start + j D + c) mod M)  sum_{p < M} w^(-k p mod M)  u_p[j],     u_p[j] = sum_i h[i M + p] x[j D + c - i M - p]
//
// so the FIR (the u_p) is computed once per output time and shared by every channel, the rotation is an M-point DFT at the
// OUTPUT rate with twiddles from a table (cos / sin of 2 pi r / M, float64 on the host, rounded to float32), and every phase
// index is an integer reduced modulo M: the phase is exact at any stream index.  D need not equal, divide or be divided by M.
//
//   TILE: one wavefront per workgroup computes CH_TO = 256 consecutive output times.  The (256 + ceil(c/D) + floor(c/D) + 1) D
//   samples the tile needs are loaded with consecutive lanes on consecutive samples, converted (NOT rotated) and written to LDS
//   sample-phase-major modulo D: X_b[m] = x[(m0 + m) D + b].  For a tap (i, p), c - i M - p = a D + b with a, b wave-uniform
//   (kept by scalar increments: no division in the loop), and the sample output j meets is entry j + a of row b.  A lane owns
//   the CH_R = 4 outputs lane, lane + 64, lane + 128, lane + 192 of the tile, so lane l reads float2 index l + const of a row:
//   64 consecutive 8-byte entries, conflict-free for any (D, M), with no padding inside a row; rows are an odd number of
//   float2 long so that the staging writes of consecutive lanes, one row apart, spread over the banks.  The tap is a scalar
//   load and one v_pk_fma_f32 per output serves (re, im).  After each p the CG channels of the group add w^(-k p) u_p into
//   their own complex accumulator (the twiddle is a scalar load from the table, its index kept by adding k modulo M); at the
//   end every output is multiplied by w^(k (start + j D + c)), a per-lane table index.  More than CG channels run as further
//   groups over the SAME staged tile: the raw samples are read once per call, the FIR once per group of eight.
//   (Measured against this: a tap table in LDS in front of the rows, tap-phase-major slots of (tap, byte offset of the row
//   entry) read four at a time one quad ahead, so that the loop has no scalar arithmetic and no scalar loads -- 45 instead
//   of 110 instructions per four taps, 6 % faster at K = 1 and 2 on the 600 s recording, 20 % and 13 % SLOWER at K = 8 and
//   12, and the table takes LDS from the rows: the switch to the direct form moves from D = 74 to 69.  Not kept.)
//
//   DIRECT (a tile that does not fit PRC_CHANNELIZE_TILE_MAX_BYTES of LDS: large D, long custom taps; or forced by
//   PRC_OPT_CHANNELIZE_FORM): one wavefront per output time and channel, lane l takes taps l, l + 64, ..., multiplies each
//   sample by its exact table twiddle, sums its own terms in order, and the xor tree 32, 16, 8, 4, 2, 1 (the tree of wave.h)
//   adds the lanes.
//
// Order of the sums (tests/channelize_oracle.py restates both): tile -- p ascending, i ascending inside, every channel on its
// own; direct -- taps ascending per lane, then the tree.  Every multiply-add is an explicit fma: the bits of a channel do not
// depend on the group size it was compiled into, on which other channels were requested or in what order, and two calls give
// the same bits.  No atomics, no inline assembly; nothing is allocated and nothing synchronises.
#include "common.h"

namespace {

constexpr int CH_T = 64;                  // one wavefront per workgroup
constexpr int CH_R = 4;                   // outputs per lane, CH_T apart
constexpr int CH_TO = CH_T * CH_R;        // output times per tile
constexpr int CH_Q = 4;                   // taps of a phase requested together
constexpr int CH_G = 8;                   // channels per group at most (CH_G * CH_R complex accumulators per lane)
static_assert(PRC_CHANNELIZE_TILE_MAX_BYTES <= 160 * 1024, "the largest tile fits the LDS of a CU");
static_assert(PRC_CHANNELIZE_MAX_SEL % CH_G == 0, "whole groups");

constexpr int CH_DIRECT_T = 256;          // direct form: four wavefronts, one output each per round
constexpr int64_t CH_DIRECT_MAX_WGS = 1 << 20;

typedef float ch_v2f __attribute__((ext_vector_type(2)));

struct ChanArgs {
    const void* x;
    int64_t n, n_out, out_stride;
    int32_t M, D, L, K;
    int32_t c;                 // (L - 1) / 2
    int32_t a_lo;              // ceil(c / D): row entry 0 of a tile is output j0 - a_lo
    int32_t ne, row;           // entries a tile needs per row: CH_TO + a_lo + floor(c / D) + 1; the row length, ne made odd
    int32_t qm, rm;            // M / D, M % D: a tap M further on is qm entries and rm rows back
    int32_t s0m;               // (start + c) mod M
    int32_t dm;                // D mod M
    uint32_t dinv, minv;       // ceil(2^32 / D), ceil(2^32 / M): floor(u / q) == umulhi(u, qinv) for u q < 2^32
};
// The tables and the result are kernel parameters of their own, __restrict__: the tile kernel stores a group's rows before it
// loads the next group's taps and twiddles, and only what is known not to alias those stores stays on the scalar unit.
struct ChanPtrs {
    const float* taps;
    const float2* tw;          // tw[r] = (cos, sin)(2 pi r / M): w^e = conj(tw[e])
    const int32_t* chans;
    float2* out;
};
#define CH_PTR_PARAMS const float* __restrict__ taps, const float2* __restrict__ tw, const int32_t* __restrict__ chans, float2* __restrict__ out

// the loader of preproc.hip (fd_load): one complex sample of any raw type, element alignment only
template <int SRC>
__device__ __forceinline__ float2 ch_load(const void* base, int64_t e) {
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

// x[i], zero outside [0, n).  The load itself is unconditional, from the nearest sample inside: a batch issues back to back.
template <int SRC>
__device__ __forceinline__ float2 ch_sample(const ChanArgs& a, int64_t i) {
    const bool inside = i >= 0 && i < a.n;
    const int64_t ic = i < 0 ? 0 : (i < a.n ? i : a.n - 1);
    const float2 v = ch_load<SRC>(a.x, ic);
    return inside ? v : make_float2(0.f, 0.f);
}

// x mod M for x M < 2^32
__device__ __forceinline__ uint32_t ch_mod(uint32_t x, uint32_t M, uint32_t minv) { return x - __umulhi(x, minv) * M; }

// channel i of the call as a number in [0, M): k and k - M are the same channel, and any int32 is safe
__device__ __forceinline__ int ch_fold(int k, int M) {
    k %= M;
    return k < 0 ? k + M : k;
}

// acc w^e = acc conj(tw[e])
__device__ __forceinline__ float2 ch_mul_conj(float2 v, float2 t) {
    return make_float2(fmaf(v.x, t.x, v.y * t.y), fmaf(v.y, t.x, -(v.x * t.y)));
}

template <int SRC, int CG>
__global__ __launch_bounds__(CH_T) void chan_tile_kernel(ChanArgs a, CH_PTR_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) float2 ch_lds[];
    const int lane = threadIdx.x;
    const int D = a.D, M = a.M;
    const int64_t j0 = (int64_t)blockIdx.x * CH_TO;          // first output time of the tile

    // row b, entry m holds x[(j0 - a_lo + m) D + b]: the tile's samples are one contiguous run from `first`
    const int64_t first = (j0 - a.a_lo) * D;
    const int total = a.ne * D;
#pragma unroll 8
    for (int u = lane; u < total; u += CH_T) {
        const float2 v = ch_sample<SRC>(a, first + u);
        const int m = D == 1 ? u : (int)__umulhi((unsigned)u, a.dinv);   // u / D
        const int b = u - m * D;
        ch_lds[b * a.row + m] = v;
    }
    __syncthreads();

    // (start + j D + c) mod M of the lane's outputs: j mod M from the tile's own remainder, then integer steps
    uint32_t tm[CH_R];
    {
        const uint32_t j0m = ch_mod(((uint32_t)blockIdx.x % (uint32_t)M) * (uint32_t)(CH_TO % M), M, a.minv);
        uint32_t jm = ch_mod(j0m + (uint32_t)lane, M, a.minv);
#pragma unroll
        for (int r = 0; r < CH_R; ++r) {
            tm[r] = ch_mod((uint32_t)a.s0m + jm * (uint32_t)a.dm, M, a.minv);
            jm = ch_mod(jm + (uint32_t)(CH_T % M), M, a.minv);
        }
    }

    const ch_v2f* lds = (const ch_v2f*)ch_lds + lane;
    const int pmax = a.L < M ? a.L : M;                      // tap phases p >= L are empty
    for (int g0 = 0; g0 < a.K; g0 += CG) {
        int kf[CG], ti[CG];                                  // the channel, and (k p) mod M
#pragma unroll
        for (int g = 0; g < CG; ++g) {
            kf[g] = ch_fold(chans[g0 + g < a.K ? g0 + g : a.K - 1], M);   // a ragged last group repeats the last channel, unstored
            ti[g] = 0;
        }
        float2 acc[CG][CH_R];
#pragma unroll
        for (int g = 0; g < CG; ++g)
#pragma unroll
            for (int r = 0; r < CH_R; ++r) acc[g][r] = make_float2(0.f, 0.f);

        // tap p meets sample offset c - p = ap D + bp (floor division); one p further on is one row back
        int ap = a.c / D, bp = a.c - ap * D;
        int cnt = (a.L - 1) / M + 1, wrap = (a.L - 1) % M;   // taps of phase p: one fewer from p = (L - 1) mod M + 1 on
        for (int p = 0; p < pmax; ++p) {
            ch_v2f u[CH_R];
#pragma unroll
            for (int r = 0; r < CH_R; ++r) u[r] = (ch_v2f)(0.f);
            int ai = ap + a.a_lo, bi = bp;                   // entry of output j0 + lane: lane + ai, in row bi
            // four taps of the phase at a time, the next four requested before these are used (an index past the last tap
            // loads the last tap and is not used): the scalar loads are waited for once per four, behind the LDS reads
            const int last = a.L - 1;
            float h[CH_Q];
#pragma unroll
            for (int q = 0; q < CH_Q; ++q) h[q] = taps[min(p + q * M, last)];
            int t = p, left = cnt;
            for (; left >= CH_Q; left -= CH_Q, t += CH_Q * M) {
                float hn[CH_Q];
#pragma unroll
                for (int q = 0; q < CH_Q; ++q) hn[q] = taps[min(t + (CH_Q + q) * M, last)];
#pragma unroll
                for (int q = 0; q < CH_Q; ++q) {
                    const ch_v2f* row = lds + bi * a.row + ai;
#pragma unroll
                    for (int r = 0; r < CH_R; ++r) u[r] = __builtin_elementwise_fma((ch_v2f)(h[q]), row[r * CH_T], u[r]);
                    ai -= a.qm;
                    bi -= a.rm;
                    if (bi < 0) { bi += D; ai -= 1; }
                }
#pragma unroll
                for (int q = 0; q < CH_Q; ++q) h[q] = hn[q];
            }
#pragma unroll
            for (int q = 0; q < CH_Q - 1; ++q) {
                if (q < left) {
                    const ch_v2f* row = lds + bi * a.row + ai;
#pragma unroll
                    for (int r = 0; r < CH_R; ++r) u[r] = __builtin_elementwise_fma((ch_v2f)(h[q]), row[r * CH_T], u[r]);
                    ai -= a.qm;
                    bi -= a.rm;
                    if (bi < 0) { bi += D; ai -= 1; }
                }
            }
#pragma unroll
            for (int g = 0; g < CG; ++g) {
                const float2 w = tw[ti[g]];                  // w^(-k p) = tw[(k p) mod M]
#pragma unroll
                for (int r = 0; r < CH_R; ++r) cmac(acc[g][r], w, make_float2(u[r].x, u[r].y));
                ti[g] += kf[g];
                if (ti[g] >= M) ti[g] -= M;
            }
            bp -= 1;
            if (bp < 0) { bp += D; ap -= 1; }
            if (p == wrap) cnt -= 1;
        }

#pragma unroll
        for (int r = 0; r < CH_R; ++r) {
            const int64_t j = j0 + r * CH_T + lane;
            if (j < a.n_out) {
#pragma unroll
                for (int g = 0; g < CG; ++g) {
                    if (g0 + g < a.K) {
                        const float2 w = tw[ch_mod((uint32_t)kf[g] * tm[r], M, a.minv)];
                        out[(int64_t)(g0 + g) * a.out_stride + j] = ch_mul_conj(acc[g][r], w);
                    }
                }
            }
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(CH_DIRECT_T) void chan_direct_kernel(ChanArgs a, CH_PTR_PARAMS) {
    const int lane = threadIdx.x & (PRC_WAVE - 1);
    const int M = a.M;
    const int64_t waves = (int64_t)gridDim.x * (CH_DIRECT_T / PRC_WAVE);
    const uint32_t kf = (uint32_t)ch_fold(chans[blockIdx.y], M);
    float2* row = out + (int64_t)blockIdx.y * a.out_stride;
    for (int64_t j = (int64_t)blockIdx.x * (CH_DIRECT_T / PRC_WAVE) + (threadIdx.x / PRC_WAVE); j < a.n_out; j += waves) {
        const int64_t top = j * a.D + a.c;                   // the sample tap 0 meets
        const uint32_t base = ch_mod((uint32_t)a.s0m + (uint32_t)(j % M) * (uint32_t)a.dm, M, a.minv);   // (start + top) mod M
        float2 s = make_float2(0.f, 0.f);
        for (int t = lane; t < a.L; t += PRC_WAVE) {
            const float2 v = ch_sample<SRC>(a, top - t);
            const float h = taps[t];
            int em = (int)base - (int)ch_mod((uint32_t)t, M, a.minv);                 // (start + top - t) mod M
            if (em < 0) em += M;
            const float2 z = ch_mul_conj(v, tw[ch_mod(kf * (uint32_t)em, M, a.minv)]);
            s.x = fmaf(h, z.x, s.x);
            s.y = fmaf(h, z.y, s.y);
        }
#pragma unroll
        for (int off = PRC_WAVE / 2; off > 0; off >>= 1) {   // every lane ends with the same sum
            s.x += __shfl_xor(s.x, off, PRC_WAVE);
            s.y += __shfl_xor(s.y, off, PRC_WAVE);
        }
        if (lane == 0) row[j] = s;
    }
}

template <int SRC, int CG>
int chan_tile_launch(const ChanArgs& a, const ChanPtrs& p, size_t lds, hipStream_t st) {
    { int rc_ = prc_lds_optin(reinterpret_cast<const void*>(&chan_tile_kernel<SRC, CG>), (int)lds); if (rc_) return rc_; }
    const int64_t tiles = ceil_div64(a.n_out, CH_TO);
    hipLaunchKernelGGL((chan_tile_kernel<SRC, CG>), dim3((uint32_t)tiles), dim3(CH_T), lds, st, a, p.taps, p.tw, p.chans, p.out);
    return PRC_OK;
}

template <int SRC>
int chan_launch(const ChanArgs& a, const ChanPtrs& p, bool tile, size_t lds, hipStream_t st) {
    if (tile) {
        // the smallest group that holds the call, eight at most: a lone channel does not pay for seven
        if (a.K == 1) return chan_tile_launch<SRC, 1>(a, p, lds, st);
        if (a.K == 2) return chan_tile_launch<SRC, 2>(a, p, lds, st);
        if (a.K <= 4) return chan_tile_launch<SRC, 4>(a, p, lds, st);
        return chan_tile_launch<SRC, CH_G>(a, p, lds, st);
    }
    int64_t wgs = ceil_div64(a.n_out, CH_DIRECT_T / PRC_WAVE);
    if (wgs > CH_DIRECT_MAX_WGS) wgs = CH_DIRECT_MAX_WGS;
    hipLaunchKernelGGL((chan_direct_kernel<SRC>), dim3((uint32_t)wgs, (uint32_t)a.K), dim3(CH_DIRECT_T), 0, st, a, p.taps, p.tw, p.chans, p.out);
    return PRC_OK;
}

uint32_t recip32(int32_t q) { return q >= 2 ? (uint32_t)(((1ull << 32) + (uint64_t)q - 1) / (uint64_t)q) : 0u; }

}  // namespace

extern "C" int prc_channelize(const prc_channelize_desc* desc, const float* taps, const void* twiddles, const int32_t* channels,
                              const void* x, int64_t n, void* out, int64_t out_stride, void* stream) {
    PRC_RANGE("prc_channelize");
    static_assert(sizeof(prc_channelize_desc) == PRC_CHANNELIZE_DESC_SIZE_680,
                  "prc_channelize_desc grew: keep PRC_CHANNELIZE_DESC_SIZE_680, default the new fields to 0");
    PRC_REQUIRE(desc, PRC_EINVAL, "prc_channelize: null descriptor");
    prc_channelize_desc d;
    if (int rc = prc_take_desc(&d, desc, PRC_CHANNELIZE_DESC_SIZE_680, "prc_channelize", "prc_channelize_desc")) return rc;
    PRC_REQUIRE(d.nchan >= 2 && d.nchan <= PRC_CHANNELIZE_MAX_CHAN, PRC_EINVAL, "prc_channelize: nchan = %d: not in 2 .. %d", d.nchan,
                PRC_CHANNELIZE_MAX_CHAN);
    PRC_REQUIRE(d.dec >= 1, PRC_EINVAL, "prc_channelize: dec = %d", d.dec);
    PRC_REQUIRE(d.ntaps >= 1 && (d.ntaps & 1), PRC_EINVAL, "prc_channelize: ntaps = %d: not a positive odd number", d.ntaps);
    PRC_REQUIRE(d.ntaps < (1 << 24), PRC_ESHAPE, "prc_channelize: ntaps = %d: 2^24 or more", d.ntaps);
    PRC_REQUIRE(d.raw_dtype >= PRC_RAW_I8 && d.raw_dtype <= PRC_RAW_C64, PRC_EINVAL, "prc_channelize: raw_dtype = %d: not a prc_raw_dtype",
                d.raw_dtype);
    PRC_REQUIRE(d.nsel >= 1 && d.nsel <= PRC_CHANNELIZE_MAX_SEL, PRC_EINVAL, "prc_channelize: nsel = %d: not in 1 .. %d", d.nsel,
                PRC_CHANNELIZE_MAX_SEL);
    PRC_REQUIRE(n >= 0, PRC_EINVAL, "prc_channelize: n = %lld", (long long)n);
    PRC_REQUIRE(n <= ((int64_t)1 << 62) / d.dec, PRC_EINVAL, "prc_channelize: n = %lld with dec = %d overflows", (long long)n, d.dec);
    const int64_t n_out = ceil_div64(n, d.dec);
    PRC_REQUIRE(d.nsel == 1 || out_stride >= n_out, PRC_EINVAL, "prc_channelize: out_stride = %lld is below the %lld outputs of a row",
                (long long)out_stride, (long long)n_out);
    PRC_REQUIRE(taps && twiddles && channels && x && out, PRC_EINVAL, "prc_channelize: null argument");
    PRC_REQUIRE(((uintptr_t)out & 7u) == 0 && ((uintptr_t)twiddles & 7u) == 0 && ((uintptr_t)taps & 3u) == 0 && ((uintptr_t)channels & 3u) == 0,
                PRC_EINVAL, "prc_channelize: out and twiddles need 8-byte, taps and channels 4-byte alignment");
    if (n == 0) return PRC_OK;

    const int M = d.nchan, D = d.dec;
    ChanArgs a;
    const ChanPtrs p = {taps, (const float2*)twiddles, channels, (float2*)out};
    a.x = x;
    a.n = n;
    a.n_out = n_out;
    a.out_stride = out_stride;
    a.M = M;
    a.D = D;
    a.L = d.ntaps;
    a.K = d.nsel;
    a.c = (d.ntaps - 1) / 2;
    a.a_lo = (a.c + D - 1) / D;
    const int64_t ne = (int64_t)CH_TO + a.a_lo + a.c / D + 1;
    const int64_t row = ne | 1;
    a.ne = (int32_t)ne;
    a.row = (int32_t)row;
    a.qm = M / D;
    a.rm = M % D;
    const int64_t s0 = (d.start % M + a.c % M) % M;          // d.start may be negative: fold the remainder up
    a.s0m = (int32_t)(s0 < 0 ? s0 + M : s0);
    a.dm = D % M;
    a.dinv = recip32(D);
    a.minv = recip32(M);
    const int64_t lds = row * D * (int64_t)sizeof(float2);
    const bool tile = lds <= PRC_CHANNELIZE_TILE_MAX_BYTES && prc_opt(PRC_OPT_CHANNELIZE_FORM) == 0 &&
                      ceil_div64(n_out, CH_TO) <= (int64_t)0x7fffffff;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    switch (d.raw_dtype) {
        case PRC_RAW_I8: rc = chan_launch<PRC_RAW_I8>(a, p, tile, (size_t)lds, st); break;
        case PRC_RAW_U8: rc = chan_launch<PRC_RAW_U8>(a, p, tile, (size_t)lds, st); break;
        case PRC_RAW_I16: rc = chan_launch<PRC_RAW_I16>(a, p, tile, (size_t)lds, st); break;
        case PRC_RAW_F32: rc = chan_launch<PRC_RAW_F32>(a, p, tile, (size_t)lds, st); break;
        default: rc = chan_launch<PRC_RAW_C64>(a, p, tile, (size_t)lds, st); break;
    }
    if (rc != PRC_OK) return rc;
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
