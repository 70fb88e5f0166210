// Joint least-squares removal of strong echoes at arbitrary (lag, Doppler) -- CLEAN on the surveillance stream (include/prcore.h:
// prc_echo_cancel states the definition).  For frame b and its K valid atoms (lag D_k, Doppler f_k)
//   a_k[i] = ref[idx(i - D_k)] exp(+j 2 pi f_k i / Fs),  s_k[i] = (i/n - 1/2) a_k[i]  (ramp),  A = [a_0, s_0, a_1, s_1, ...],
//   G = A^H A + reg I,  g = A^H srv,  c = G^-1 g,  out = srv - A c,
// with `refine` Gauss-Newton updates f_k += clamp(Im(c_s / c_a) / (2 pi), +-1/2) Fs / n before the final fit.
//
// echo_prep_kernel: one thread per frame compacts the valid atoms of the caller's list into a working copy in the workspace
//   (the caller's list is never written) and clears the frame's state.
// echo_gram_kernel, grid (chunk of whole tiles, frame): per 128-sample tile the C modulated columns and srv go to LDS as complex
//   float32, sample-major [i][P] with P = C + 1 odd-padded.  The phase of sample i is seed(run of 16) * w(i mod 16): the seed's
//   argument frac(f i0 / Fs) is reduced in float64 (f i0 as an exact product, as xambg_patch.hip), w is a 16-entry table per
//   atom from float64 -- no float32 ramp over i and no rotation chain.  The (C + 1)(C + 2) / 2 pairs (p, q <= p) of the triangle
//   are dealt to `lp` pair slots (a power of two, NPT pairs each); the 256 / lp slices of a slot take every (256 / lp)-th
//   sample.  A thread adds conj(col_p) col_q in float64 registers over its chunk.  LDS reads: the lanes of a slice read
//   consecutive q of one or two rows p at one sample -- consecutive 8-byte words (and a broadcast), conflict-free but where a
//   32-lane group straddles two rows longer than 32.  Slices add by xor butterflies inside a wavefront (wave.h) and through
//   LDS across wavefronts, in slice order; partials go to the workspace.
// echo_reduce_kernel adds the chunks in chunk order in float64.
// echo_solve_kernel, one wavefront per frame: the packed lower triangle in LDS in float64, Cholesky by columns (lane i owns
//   row i), forward and back substitution with the right-hand side in registers, one broadcast per column; the Doppler update
//   of the working copy, or -- the final fit -- the fit records and info.
// echo_apply_kernel, 1024-sample tiles: out[i] = srv[i] - sum_k (c_a + c_s (i/n - 1/2)) a_k[i], phasors as above, float32.
// No atomics; every workspace word that is read was written earlier in the same call.
#include "common.h"
#include "wave.h"

#include <cmath>

namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_TILE = 128;                      // samples of a Gram tile
constexpr int EC_RUN = 16;                        // samples that share a float64 seed
constexpr int EC_ATILE = 1024;                    // samples of an apply tile
constexpr int EC_MAXA = PRC_ECHO_MAX_ATOMS;
constexpr int EC_MAXC = 2 * EC_MAXA;              // columns of A
constexpr int EC_WGS = 1024;                      // Gram workgroups aimed at over all frames
constexpr double EC_PIVOT_FLOOR = 0x1p-40;        // of the pivot's own diagonal entry of G: below it a pivot is rounding, not
                                                  // signal (duplicate atoms give a few 2^-52; a cond(G) of 1e11 still passes)
constexpr double EC_2PI = 6.283185307179586476925286766559;

struct EcWs {                                     // the caller's workspace, carved
    int32_t* nvalid;          // [nframes]
    int32_t* status;          // [nframes] 1: the solve broke down
    int32_t* lag;             // [nframes][M] compacted
    int32_t* slot;            // [nframes][M] caller's index -> compacted index, -1: not valid
    uint32_t* flags;          // [nframes][M] compacted: bit 1 once a refinement was clamped
    double* f;                // [nframes][M] compacted, refined in place
    double2* coef;            // [nframes][2 M]
    double2* gram;            // [nframes][npairs]
    double2* part;            // [nframes][nchunks][npairs]
};

struct EcArgs {
    const float2* ref;
    const float2* srv;
    const prc_echo_atom* atoms;
    const int32_t* counts;
    float2* out;
    prc_echo_fit* fit;
    int32_t* info;
    EcWs w;
    int64_t n, frame_stride, out_stride, ntiles, tiles_per_chunk;
    double sample_rate, reg;
    int nframes, M, wrap, ramp, nchunks, npairs, lp, last;
};

__device__ __forceinline__ int ec_count(const EcArgs& a, int b) {
    const int c = a.counts[b];
    return c < 0 ? 0 : (c > a.M ? a.M : c);
}
__device__ __forceinline__ bool ec_valid(const prc_echo_atom& t, int64_t n) {
    return (int64_t)t.lag > -n && (int64_t)t.lag < n && __builtin_isfinite(t.doppler);
}
// Doppler in turns per sample, in [-1/2, 1/2]
__device__ __forceinline__ double ec_turns(double f, double fs) {
    double t = f / fs;
    return t - rint(t);
}
// exp(j 2 pi frac(ft i)), the product exact
__device__ __forceinline__ float2 ec_seed(double ft, int64_t i) {
    const double di = (double)i, hi = ft * di, lo = fma(ft, di, -hi);
    double s, c;
    sincospi(2.0 * ((hi - rint(hi)) + lo), &s, &c);
    return make_float2((float)c, (float)s);
}
// ref[idx(i - D)] of the definition
__device__ __forceinline__ float2 ec_ref(const float2* __restrict__ ref, int64_t i, int D, int64_t n, int wrap) {
    int64_t m = i - D;
    if (wrap) {
        if (m < 0) m += n;
        if (m >= n) m -= n;
    } else if (m < 0 || m >= n) {
        return make_float2(0.f, 0.f);
    }
    return ref[m];
}
// pair t of the triangle: t = p (p + 1) / 2 + q, q <= p
__device__ __forceinline__ void ec_pair(int t, int& p, int& q) {
    p = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (p * (p + 1) / 2 > t) --p;
    while ((p + 1) * (p + 2) / 2 <= t) ++p;
    q = t - p * (p + 1) / 2;
}

__global__ __launch_bounds__(EC_THREADS) void echo_prep_kernel(EcArgs a) {
    const int b = (int)(blockIdx.x * EC_THREADS + threadIdx.x);
    if (b >= a.nframes) return;
    const int cnt = ec_count(a, b);
    const size_t o = (size_t)b * a.M;
    int k = 0;
    for (int j = 0; j < a.M; ++j) {
        int s = -1;
        if (j < cnt) {
            const prc_echo_atom t = a.atoms[o + j];
            if (ec_valid(t, a.n)) {
                a.w.lag[o + k] = t.lag;
                a.w.f[o + k] = t.doppler;
                a.w.flags[o + k] = 0u;
                s = k++;
            }
        }
        a.w.slot[o + j] = s;
    }
    a.w.nvalid[b] = k;
    a.w.status[b] = 0;
}

template <int NPT>
__global__ __launch_bounds__(EC_THREADS) void echo_gram_kernel(EcArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ec_lds[];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int K = a.w.nvalid[b];
    if (K == 0 || a.w.status[b]) return;
    const int cols = a.ramp ? 2 : 1, C = cols * K, P = C + 1, Pp = P | 1;
    const int npairs = P * (P + 1) / 2;
    // tables first (their size does not depend on the frame), then the tile, which the slice sums reuse
    double* FT = reinterpret_cast<double*>(ec_lds);                              // EC_MAXA
    float2* W = reinterpret_cast<float2*>(FT + EC_MAXA);                         // EC_MAXA * EC_RUN
    float2* SEED = W + EC_MAXA * EC_RUN;                                         // EC_MAXA * EC_TILE / EC_RUN
    int* LAG = reinterpret_cast<int*>(SEED + EC_MAXA * (EC_TILE / EC_RUN));      // EC_MAXA
    float2* T = reinterpret_cast<float2*>(LAG + EC_MAXA);                        // EC_TILE * Pp
    double2* RED = reinterpret_cast<double2*>(T);                                // EC_THREADS * NPT

    const float2* __restrict__ ref = a.ref + (int64_t)b * a.frame_stride;
    const float2* __restrict__ srv = a.srv + (int64_t)b * a.frame_stride;
    const size_t ao = (size_t)b * a.M;
    if (tid < K) {
        FT[tid] = ec_turns(a.w.f[ao + tid], a.sample_rate);
        LAG[tid] = a.w.lag[ao + tid];
    }
    __syncthreads();
    for (int e = tid; e < K * EC_RUN; e += EC_THREADS) {
        double s, c;
        sincospi(2.0 * FT[e / EC_RUN] * (double)(e % EC_RUN), &s, &c);
        W[e] = make_float2((float)c, (float)s);
    }

    const int lp = a.lp, slot = tid & (lp - 1), slice = tid / lp, nslices = EC_THREADS / lp;
    int op[NPT], oq[NPT];
    bool on[NPT];
    double2 acc[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
        const int t = slot + lp * u;
        int p = 0, q = 0;
        on[u] = t < npairs;
        if (on[u]) ec_pair(t, p, q);
        op[u] = p;
        oq[u] = q;
        acc[u] = make_double2(0.0, 0.0);
    }

    const double rn = 1.0 / (double)a.n;
    const int64_t t_first = (int64_t)chunk * a.tiles_per_chunk;
    const int64_t t_last = t_first + a.tiles_per_chunk < a.ntiles ? t_first + a.tiles_per_chunk : a.ntiles;
    for (int64_t t = t_first; t < t_last; ++t) {
        const int64_t t0 = t * EC_TILE;
        const int cnt = a.n - t0 < EC_TILE ? (int)(a.n - t0) : EC_TILE;
        for (int e = tid; e < K * (EC_TILE / EC_RUN); e += EC_THREADS)
            SEED[e] = ec_seed(FT[e / (EC_TILE / EC_RUN)], t0 + (int64_t)(e % (EC_TILE / EC_RUN)) * EC_RUN);
        __syncthreads();
        for (int e = tid; e < (K + 1) * EC_TILE; e += EC_THREADS) {
            const int k = e / EC_TILE, i = e % EC_TILE;
            const int64_t gi = t0 + i;
            float2* row = T + i * Pp;
            if (k == K) {
                row[C] = i < cnt ? srv[gi] : make_float2(0.f, 0.f);
                continue;
            }
            float2 v = make_float2(0.f, 0.f);
            if (i < cnt) {
                const float2 ph = cmul(SEED[k * (EC_TILE / EC_RUN) + i / EC_RUN], W[k * EC_RUN + i % EC_RUN]);
                v = cmul(ec_ref(ref, gi, LAG[k], a.n, a.wrap), ph);
            }
            row[cols * k] = v;
            if (a.ramp) {
                const float x = (float)((double)gi * rn - 0.5);
                row[2 * k + 1] = make_float2(v.x * x, v.y * x);
            }
        }
        __syncthreads();
        for (int i = slice; i < cnt; i += nslices) {
            const float2* row = T + i * Pp;
#pragma unroll
            for (int u = 0; u < NPT; ++u) {
                if (!on[u]) continue;
                const float2 A = row[op[u]], B = row[oq[u]];
                const double ax = A.x, ay = A.y, bx = B.x, by = B.y;
                acc[u].x = fma(ax, bx, fma(ay, by, acc[u].x));
                acc[u].y = fma(ax, by, fma(-ay, bx, acc[u].y));
            }
        }
        __syncthreads();
    }

    // the slices of a slot: inside a wavefront by butterflies, across wavefronts through LDS in slice order
    if (lp < PRC_WAVE) {
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            acc[u].x = wave_sum_mod(acc[u].x, lp);
            acc[u].y = wave_sum_mod(acc[u].y, lp);
        }
    }
    const int stride = lp < PRC_WAVE ? PRC_WAVE : lp, groups = EC_THREADS / stride;
    if (groups > 1) {
#pragma unroll
        for (int u = 0; u < NPT; ++u) RED[u * EC_THREADS + tid] = acc[u];
        __syncthreads();
    }
    if (tid < lp) {
        double2* w = a.w.part + ((size_t)b * a.nchunks + chunk) * a.npairs;
#pragma unroll
        for (int u = 0; u < NPT; ++u) {
            if (!on[u]) continue;
            double2 s = acc[u];
            for (int g = 1; g < groups; ++g) {
                const double2 o = RED[u * EC_THREADS + g * stride + tid];
                s.x += o.x;
                s.y += o.y;
            }
            w[slot + lp * u] = s;
        }
    }
}

__global__ __launch_bounds__(EC_THREADS) void echo_reduce_kernel(EcArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * EC_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.nframes * a.npairs) return;
    const int b = (int)(idx / a.npairs), t = (int)(idx % a.npairs);
    const int K = a.w.nvalid[b];
    if (K == 0 || a.w.status[b]) return;
    const int P = (a.ramp ? 2 : 1) * K + 1;
    if (t >= P * (P + 1) / 2) return;
    const double2* w = a.w.part + (size_t)b * a.nchunks * a.npairs + t;
    double2 s = make_double2(0.0, 0.0);
    for (int c = 0; c < a.nchunks; ++c) {
        const double2 o = w[(size_t)c * a.npairs];
        s.x += o.x;
        s.y += o.y;
    }
    a.w.gram[(size_t)b * a.npairs + t] = s;
}

__device__ __forceinline__ double2 ec_bcast(double2 v, int lane) { return make_double2(__shfl(v.x, lane), __shfl(v.y, lane)); }

__global__ __launch_bounds__(PRC_WAVE) void echo_solve_kernel(EcArgs a) {
    __shared__ double2 L[EC_MAXC * (EC_MAXC + 1) / 2];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int K = a.w.nvalid[b];
    const int cols = a.ramp ? 2 : 1, C = cols * K, ntri = C * (C + 1) / 2;
    const size_t ao = (size_t)b * a.M;
    bool broken = a.w.status[b] != 0;
    double2 c = make_double2(0.0, 0.0);

    if (K > 0 && !broken) {
        const double2* G = a.w.gram + (size_t)b * a.npairs;
        for (int e = lane; e < ntri; e += PRC_WAVE) L[e] = G[e];
        double2 rhs = make_double2(0.0, 0.0);            // lane i: g_i, then y_i, then c_i
        if (lane < C) rhs = zconj(G[ntri + lane]);
        __syncthreads();
        const int ri = lane * (lane + 1) / 2;
        // Cholesky G + reg I = L L^H by columns
        for (int j = 0; j < C && !broken; ++j) {
            const int rj = j * (j + 1) / 2;
            double2 s = make_double2(0.0, 0.0);
            double g0 = 0.0;
            if (lane >= j && lane < C) {
                s = L[ri + j];
                if (lane == j) g0 = s.x = s.x + a.reg;
                for (int k = 0; k < j; ++k) s = zsub(s, zmul(L[ri + k], zconj(L[rj + k])));
            }
            const double d = __shfl(s.x, j), d0 = __shfl(g0, j);
            if (!(d > EC_PIVOT_FLOOR * d0) || !__builtin_isfinite(d)) {
                broken = true;
                break;
            }
            const double r = sqrt(d);
            if (lane == j) L[ri + j] = make_double2(r, 0.0);
            else if (lane > j && lane < C) L[ri + j] = make_double2(s.x / r, s.y / r);
            __syncthreads();
        }
        if (!broken) {
            for (int j = 0; j < C; ++j) {                // L y = g
                const int rj = j * (j + 1) / 2;
                const double2 yj = zscale(ec_bcast(rhs, j), 1.0 / L[rj + j].x);
                if (lane == j) rhs = yj;
                else if (lane > j && lane < C) rhs = zsub(rhs, zmul(L[ri + j], yj));
            }
            for (int j = C - 1; j >= 0; --j) {           // L^H c = y
                const int rj = j * (j + 1) / 2;
                const double2 cj = zscale(ec_bcast(rhs, j), 1.0 / L[rj + j].x);
                if (lane == j) rhs = cj;
                else if (lane < j) rhs = zsub(rhs, zmul(zconj(L[rj + lane]), cj));
            }
            c = rhs;
            if (!(__builtin_isfinite(c.x) && __builtin_isfinite(c.y)) && lane < C) broken = true;
            broken = __any(broken);
        }
        if (broken) {
            c = make_double2(0.0, 0.0);
            if (lane == 0) a.w.status[b] = 1;
        }
    }

    // atom k of the compacted list: lane k takes (c_a, c_s) from lanes cols k, cols k + 1
    const int src = lane < K ? cols * lane : 0;
    const double2 ca = ec_bcast(c, src), cs = a.ramp ? ec_bcast(c, src + 1) : make_double2(0.0, 0.0);
    if (!a.last) {
        if (lane < K && !broken) {
            const bool fin = __builtin_isfinite(ca.x) && __builtin_isfinite(ca.y);
            if (fin && (ca.x != 0.0 || ca.y != 0.0)) {
                double dc = zdiv(cs, ca).y / EC_2PI;      // cells
                if (__builtin_isfinite(dc)) {
                    if (dc > 0.5 || dc < -0.5) {
                        dc = dc > 0.0 ? 0.5 : -0.5;
                        a.w.flags[ao + lane] |= 2u;
                    }
                    a.w.f[ao + lane] += dc * a.sample_rate / (double)a.n;
                }
            }
        }
        return;
    }
    if (lane < C) a.w.coef[(size_t)b * EC_MAXC + lane] = c;
    if (lane == 0) a.info[b] = broken ? 1 : 0;
    // the fit records, in the caller's order: every record of the frame is written
    const int cnt = ec_count(a, b);
    for (int j0 = 0; j0 < a.M; j0 += PRC_WAVE) {
        const int j = j0 + lane;
        const int s = j < a.M ? a.w.slot[ao + j] : -1;
        const int from = s >= 0 ? s : 0;
        const double2 fa = ec_bcast(ca, from), fs = ec_bcast(cs, from);
        if (j >= a.M) continue;
        prc_echo_fit r;
        memset(&r, 0, sizeof(r));
        if (j < cnt) {
            if (s < 0) r.flags |= 1u;
            if (broken) r.flags |= 4u;
            if (s >= 0 && !broken) {
                r.doppler = a.w.f[ao + s];
                r.amp[0] = fa.x; r.amp[1] = fa.y;
                r.slope[0] = fs.x; r.slope[1] = fs.y;
                r.flags |= a.w.flags[ao + s];
            }
        }
        a.fit[ao + j] = r;
    }
}

__global__ __launch_bounds__(EC_THREADS) void echo_apply_kernel(EcArgs a) {
    __shared__ double FT[EC_MAXA];
    __shared__ float2 W[EC_MAXA * EC_RUN];
    __shared__ float2 SEED[EC_MAXA * (EC_ATILE / EC_RUN)];
    __shared__ float2 CA[EC_MAXA], CS[EC_MAXA];
    __shared__ int LAG[EC_MAXA];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * EC_ATILE;
    const float2* __restrict__ ref = a.ref + (int64_t)b * a.frame_stride;
    const float2* __restrict__ srv = a.srv + (int64_t)b * a.frame_stride;
    float2* __restrict__ out = a.out + (int64_t)b * a.out_stride;
    const int K = a.w.status[b] ? 0 : a.w.nvalid[b];
    if (K == 0) {                                        // nothing to subtract: the bits of srv
        for (int i = tid; i < EC_ATILE && t0 + i < a.n; i += EC_THREADS) out[t0 + i] = srv[t0 + i];
        return;
    }
    const int cols = a.ramp ? 2 : 1;
    const size_t ao = (size_t)b * a.M;
    if (tid < K) {
        FT[tid] = ec_turns(a.w.f[ao + tid], a.sample_rate);
        LAG[tid] = a.w.lag[ao + tid];
        const double2 ca = a.w.coef[(size_t)b * EC_MAXC + cols * tid];
        const double2 cs = a.ramp ? a.w.coef[(size_t)b * EC_MAXC + 2 * tid + 1] : make_double2(0.0, 0.0);
        CA[tid] = make_float2((float)ca.x, (float)ca.y);
        CS[tid] = make_float2((float)cs.x, (float)cs.y);
    }
    __syncthreads();
    for (int e = tid; e < K * EC_RUN; e += EC_THREADS) {
        double s, c;
        sincospi(2.0 * FT[e / EC_RUN] * (double)(e % EC_RUN), &s, &c);
        W[e] = make_float2((float)c, (float)s);
    }
    for (int e = tid; e < K * (EC_ATILE / EC_RUN); e += EC_THREADS)
        SEED[e] = ec_seed(FT[e / (EC_ATILE / EC_RUN)], t0 + (int64_t)(e % (EC_ATILE / EC_RUN)) * EC_RUN);
    __syncthreads();
    const double rn = 1.0 / (double)a.n;
    for (int i = tid; i < EC_ATILE && t0 + i < a.n; i += EC_THREADS) {
        const int64_t gi = t0 + i;
        const float x = (float)((double)gi * rn - 0.5);
        float2 sum = make_float2(0.f, 0.f);
        for (int k = 0; k < K; ++k) {
            const float2 ph = cmul(SEED[k * (EC_ATILE / EC_RUN) + i / EC_RUN], W[k * EC_RUN + i % EC_RUN]);
            const float2 v = cmul(ec_ref(ref, gi, LAG[k], a.n, a.wrap), ph);
            const float2 cf = make_float2(fmaf(CS[k].x, x, CA[k].x), fmaf(CS[k].y, x, CA[k].y));
            cmac(sum, cf, v);
        }
        const float2 s = srv[gi];
        out[gi] = make_float2(s.x - sum.x, s.y - sum.y);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct EcShape {
    int64_t ntiles, tiles_per_chunk;
    int nchunks, npairs, npt, lp;
    size_t lds, off[9], bytes;
};

int ec_check(prc_echo_desc* d, const prc_echo_desc* desc, EcShape* sh, const char* who) {
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_ECHO_DESC_SIZE_MIN, who, "prc_echo_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->n >= 1, PRC_EINVAL, "%s: n = %lld < 1", who, (long long)d->n);
    PRC_REQUIRE(d->n <= (int64_t)0x7fffffff, PRC_ESHAPE, "%s: n = %lld: frames of 2^31 samples or more are not supported", who,
                (long long)d->n);
    PRC_REQUIRE(d->nframes >= 1, PRC_EINVAL, "%s: nframes = %d < 1", who, d->nframes);
    PRC_REQUIRE(d->nframes <= 65535, PRC_ESHAPE, "%s: nframes = %d: more than 65535 frames in one call", who, d->nframes);
    PRC_REQUIRE(d->nframes == 1 || (d->frame_stride >= d->n && d->out_stride >= d->n), PRC_EINVAL,
                "%s: frame_stride = %lld, out_stride = %lld below n = %lld with %d frames", who, (long long)d->frame_stride,
                (long long)d->out_stride, (long long)d->n, d->nframes);
    PRC_REQUIRE(d->max_atoms >= 1 && d->max_atoms <= PRC_ECHO_MAX_ATOMS, PRC_EINVAL, "%s: max_atoms = %d outside 1 .. %d", who,
                d->max_atoms, PRC_ECHO_MAX_ATOMS);
    PRC_REQUIRE(d->wrap == 0 || d->wrap == 1, PRC_EINVAL, "%s: wrap = %d, not 0 or 1", who, d->wrap);
    PRC_REQUIRE(d->ramp == 0 || d->ramp == 1, PRC_EINVAL, "%s: ramp = %d, not 0 or 1", who, d->ramp);
    PRC_REQUIRE(d->refine >= 0 && d->refine <= PRC_ECHO_MAX_REFINE, PRC_EINVAL, "%s: refine = %d outside 0 .. %d", who, d->refine,
                PRC_ECHO_MAX_REFINE);
    PRC_REQUIRE(d->refine == 0 || d->ramp == 1, PRC_EINVAL, "%s: refine = %d needs the Doppler-slope columns (ramp = 1)", who,
                d->refine);
    PRC_REQUIRE(std::isfinite(d->reg) && d->reg >= 0.0, PRC_EINVAL, "%s: reg = %g, not finite and >= 0", who, d->reg);
    PRC_REQUIRE(std::isfinite(d->sample_rate) && d->sample_rate != 0.0, PRC_EINVAL, "%s: sample_rate must be finite and non-zero",
                who);
    const int P = (1 + d->ramp) * d->max_atoms + 1;
    sh->npairs = P * (P + 1) / 2;
    sh->npt = sh->npairs <= EC_THREADS ? 1 : (sh->npairs <= 3 * EC_THREADS ? 3 : 9);
    const int slots = (sh->npairs + sh->npt - 1) / sh->npt;
    sh->lp = 1;
    while (sh->lp < slots) sh->lp <<= 1;
    sh->ntiles = ceil_div64(d->n, EC_TILE);
    const int64_t want = std::min<int64_t>(sh->ntiles, std::max<int64_t>(1, ceil_div64(EC_WGS, d->nframes)));
    sh->tiles_per_chunk = ceil_div64(sh->ntiles, want);
    sh->nchunks = (int)ceil_div64(sh->ntiles, sh->tiles_per_chunk);
    const size_t tables = sizeof(double) * EC_MAXA + sizeof(float2) * EC_MAXA * (EC_RUN + EC_TILE / EC_RUN) + sizeof(int) * EC_MAXA;
    sh->lds = tables + std::max(sizeof(float2) * EC_TILE * (size_t)(P | 1), sizeof(double2) * EC_THREADS * (size_t)sh->npt);
    // the workspace, every array on a 16-byte boundary
    const size_t nf = (size_t)d->nframes, M = (size_t)d->max_atoms;
    const size_t sizes[9] = {4 * nf, 4 * nf, 4 * nf * M, 4 * nf * M, 4 * nf * M, 8 * nf * M, 16 * nf * EC_MAXC, 16 * nf * (size_t)sh->npairs,
                             16 * nf * (size_t)sh->nchunks * (size_t)sh->npairs};
    size_t o = 0;
    for (int i = 0; i < 9; ++i) {
        sh->off[i] = o;
        o += (sizes[i] + 15) & ~(size_t)15;
    }
    sh->bytes = o;
    return PRC_OK;
}

template <int NPT>
int ec_gram(const EcArgs& a, const EcShape& sh, hipStream_t st) {
    if (sh.lds > 65536) {
        const int rc = prc_lds_optin(reinterpret_cast<const void*>(&echo_gram_kernel<NPT>), (int)sh.lds);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(echo_gram_kernel<NPT>, dim3((unsigned)sh.nchunks, (unsigned)a.nframes), dim3(EC_THREADS), sh.lds, st, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

}  // namespace

extern "C" int prc_echo_cancel_workspace_bytes(const prc_echo_desc* desc, size_t* bytes) {
    prc_echo_desc d;
    EcShape sh;
    const int rc = ec_check(&d, desc, &sh, "prc_echo_cancel_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(bytes != nullptr, PRC_EINVAL, "prc_echo_cancel_workspace_bytes: null pointer");
    *bytes = sh.bytes;
    return PRC_OK;
}

extern "C" int prc_echo_cancel(const prc_echo_desc* desc, const void* ref, const void* srv, const prc_echo_atom* atoms,
                               const int32_t* counts, void* out, prc_echo_fit* fit, int32_t* info, void* workspace, void* stream) {
    PRC_RANGE("prc_echo_cancel");
    prc_echo_desc d;
    EcShape sh;
    const int rc = ec_check(&d, desc, &sh, "prc_echo_cancel");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(ref && srv && atoms && counts && out && fit && info && workspace, PRC_EINVAL, "prc_echo_cancel: null pointer");
    PRC_REQUIRE(((uintptr_t)workspace & 15u) == 0, PRC_EINVAL, "prc_echo_cancel: the workspace is not 16-byte aligned");
    EcArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = static_cast<const float2*>(ref);
    a.srv = static_cast<const float2*>(srv);
    a.atoms = atoms;
    a.counts = counts;
    a.out = static_cast<float2*>(out);
    a.fit = fit;
    a.info = info;
    char* w = static_cast<char*>(workspace);
    a.w.nvalid = reinterpret_cast<int32_t*>(w + sh.off[0]);
    a.w.status = reinterpret_cast<int32_t*>(w + sh.off[1]);
    a.w.lag = reinterpret_cast<int32_t*>(w + sh.off[2]);
    a.w.slot = reinterpret_cast<int32_t*>(w + sh.off[3]);
    a.w.flags = reinterpret_cast<uint32_t*>(w + sh.off[4]);
    a.w.f = reinterpret_cast<double*>(w + sh.off[5]);
    a.w.coef = reinterpret_cast<double2*>(w + sh.off[6]);
    a.w.gram = reinterpret_cast<double2*>(w + sh.off[7]);
    a.w.part = reinterpret_cast<double2*>(w + sh.off[8]);
    a.n = d.n;
    a.frame_stride = d.frame_stride;
    a.out_stride = d.out_stride;
    a.ntiles = sh.ntiles;
    a.tiles_per_chunk = sh.tiles_per_chunk;
    a.sample_rate = d.sample_rate;
    a.reg = d.reg;
    a.nframes = d.nframes;
    a.M = d.max_atoms;
    a.wrap = d.wrap;
    a.ramp = d.ramp;
    a.nchunks = sh.nchunks;
    a.npairs = sh.npairs;
    a.lp = sh.lp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(echo_prep_kernel, dim3((unsigned)((d.nframes + EC_THREADS - 1) / EC_THREADS)), dim3(EC_THREADS), 0, st, a);
    PRC_LAUNCH_CHECK();
    for (int pass = 0; pass <= d.refine; ++pass) {
        a.last = pass == d.refine;
        const int grc = sh.npt == 1 ? ec_gram<1>(a, sh, st) : (sh.npt == 3 ? ec_gram<3>(a, sh, st) : ec_gram<9>(a, sh, st));
        if (grc != PRC_OK) return grc;
        hipLaunchKernelGGL(echo_reduce_kernel, dim3((unsigned)ceil_div64((int64_t)d.nframes * sh.npairs, EC_THREADS)), dim3(EC_THREADS),
                           0, st, a);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(echo_solve_kernel, dim3((unsigned)d.nframes), dim3(PRC_WAVE), 0, st, a);
        PRC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(echo_apply_kernel, dim3((unsigned)ceil_div64(d.n, EC_ATILE), (unsigned)d.nframes), dim3(EC_THREADS), 0, st, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
