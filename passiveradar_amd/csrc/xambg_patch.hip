// Exact cross-ambiguity patches ("zoom") and sub-cell peak refinement (prcore.h: prc_xambg_patch, prc_xambg_patch_peaks).
//
//   X[d][l] = sum_i w[i] ref[i] conj(srv[idx(i + lag0 + l)]) exp(+j 2 pi (doppler0 + d step) i / Fs)
//
// Data movement as caf_direct.hip: a workgroup streams 1024-sample tiles of one (patch, 64 lags, 16 Dopplers) through
// LDS; P[i] = w*ref is broadcast-read, S[i + lag] is read with consecutive lanes on consecutive lags (conflict-free
// ds_read_b64), the wrap / zero rule is applied once, at the load.  Every thread forms the lag product p = P conj(S) once per
// sample and feeds 16 Doppler accumulators with one complex multiply-add each: a Horner run h = h conj(z_d) + p over
// XP_RUN samples, z_d = exp(j 2 pi f_d / Fs) wave-uniform (scalar registers), two Dopplers per packed-f32 multiply-add.  A run of K float32 steps drifts by about
// K 2^-24, so a run is 16 samples and ends in a multiplication by exp(j 2 pi frac(f_d i_last / Fs)) whose argument is
// reduced in float64: the seeds do not depend on the lag and are computed once per workgroup and tile, into LDS.
// Runs add in float32 inside a tile, tiles in float64 in registers, the four wavefronts (which split a tile in quarters)
// through LDS in float64, and the workgroups of one cell through the caller's workspace, added by a second kernel in
// float64 in chunk order.  No atomics anywhere: the bits of a result depend on the arguments alone.
// A patch of at most 32 lags (a detector's 16 x 16) would leave most lanes idle, so there the kernel runs with 16 lags per
// wavefront (LPW = 16): the four 16-lane slices of a wavefront take every fourth run of its quarter (consecutive runs are
// 128 bytes apart in S: the two slices of a 32-lane half read disjoint banks) and are added by two float64 shuffles.
#include "common.h"
#include <cmath>

#define XP_TILE 1024
#define XP_THREADS 256
#define XP_RUN 16                       // samples per Horner run
#define XP_RUNS (XP_TILE / XP_RUN)      // runs per tile
#define XP_DG 16                        // Doppler accumulators per thread
#define XP_LG 64                        // most lags per workgroup: one per lane
#define XP_NARROW 32                    // up to this many lags a workgroup takes 16 lags, four sample slices per wavefront
#define XP_MAX_CHUNKS 64                // workgroups (= workspace partials) per cell
#define XP_WAVE_SAMPLES (XP_TILE / (XP_THREADS / 64))

typedef float xp_v2f __attribute__((ext_vector_type(2)));   // one operand of a packed-f32 instruction

struct XpArgs {
    const float2* ref;
    const float2* srv;
    const float* window;
    const prc_patch* patches;
    double2* ws;               // [npatches][nchunks][ndoppler][nlags]
    int64_t n, frame_stride, ntiles, tiles_per_chunk;
    double sample_rate, step;
    int nframes, nlags, ndoppler, wrap, nlg, nchunks, patch0;
};

// a record of a device-built list is not trusted: a patch that fails this is skipped (zeros), never read for
__device__ __forceinline__ bool xp_valid(const prc_patch& p, int nframes, int64_t n) {
    return p.frame >= 0 && p.frame < nframes && (int64_t)p.lag0 > -n && (int64_t)p.lag0 < n && __builtin_isfinite(p.doppler0);
}

template <int LPW>
__global__ __launch_bounds__(XP_THREADS) void xambg_patch_kernel(XpArgs a) {
    constexpr int SUBS = 64 / LPW;                                   // sample slices per wavefront
    // one array: the staging buffers of the tile loop, then the cross-wave sums
    __shared__ __attribute__((aligned(16))) unsigned char smem[3 * XP_DG * 64 * sizeof(double2)];
    float2* P = reinterpret_cast<float2*>(smem);                    // XP_TILE
    float2* S = P + XP_TILE;                                         // XP_TILE + XP_LG
    float2* SEED = S + XP_TILE + XP_LG;                              // XP_RUNS * XP_DG
    double* FT = reinterpret_cast<double*>(SEED + XP_RUNS * XP_DG);  // XP_DG: Doppler in turns per sample, in [-1/2, 1/2]
    float2* Z = reinterpret_cast<float2*>(FT + XP_DG);               // XP_DG: conj(z_d)
    double2* RED = reinterpret_cast<double2*>(smem);                 // 3 * XP_DG * 64
    static_assert(sizeof(float2) * (2 * XP_TILE + XP_LG + XP_RUNS * XP_DG + XP_DG) + sizeof(double) * XP_DG <= sizeof(smem), "LDS");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int ll = lane % LPW;                                       // the lane's lag within the group
    const int sub = lane / LPW;                                      // its slice of the wavefront's runs
    const int chunk = blockIdx.x;
    const int lg = blockIdx.y % a.nlg;
    const int dg = blockIdx.y / a.nlg;
    const int ip = a.patch0 + blockIdx.z;
    const prc_patch pt = a.patches[ip];
    if (!xp_valid(pt, a.nframes, a.n)) return;          // the reduce kernel writes this patch's zeros
    const float2* __restrict__ ref = a.ref + (int64_t)pt.frame * a.frame_stride;
    const float2* __restrict__ srv = a.srv + (int64_t)pt.frame * a.frame_stride;
    const int L0 = lg * LPW;
    const int D0 = dg * XP_DG;

    if (tid < XP_DG) {
        double f = (pt.doppler0 + (double)(D0 + tid) * a.step) / a.sample_rate;
        f -= rint(f);
        double s, c;
        sincospi(2.0 * f, &s, &c);
        FT[tid] = f;
        Z[tid] = make_float2((float)c, (float)-s);
    }
    __syncthreads();
    // two Dopplers per packed multiply-add: (cos, cos'), (sin, sin') of the pair, wave-uniform
    xp_v2f zc[XP_DG / 2], zs[XP_DG / 2];
#pragma unroll
    for (int d = 0; d < XP_DG; ++d) {
        zc[d / 2][d % 2] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Z[d].x)));
        zs[d / 2][d % 2] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Z[d].y)));
    }

    double2 accd[XP_DG];
#pragma unroll
    for (int d = 0; d < XP_DG; ++d) accd[d] = make_double2(0.0, 0.0);

    const int64_t t_first = (int64_t)chunk * a.tiles_per_chunk;
    int64_t t_last = t_first + a.tiles_per_chunk;
    if (t_last > a.ntiles) t_last = a.ntiles;
    for (int64_t t = t_first; t < t_last; ++t) {
        const int64_t t0 = t * XP_TILE;
        const int64_t rem = a.n - t0;
        const int cnt = rem < XP_TILE ? (int)rem : XP_TILE;
        // P = w * ref, zero beyond the frame
        for (int i = tid; i < XP_TILE; i += XP_THREADS) {
            float2 v = make_float2(0.f, 0.f);
            if (i < cnt) {
                v = ref[t0 + i];
                if (a.window) {
                    const float g = a.window[t0 + i];
                    v.x *= g;
                    v.y *= g;
                }
            }
            P[i] = v;
        }
        // S[i] = srv[idx(t0 + i + lag0 + L0)]: circular inside the frame, or zero outside it
        int64_t base = t0 + (int64_t)pt.lag0 + L0;
        if (a.wrap) {
            base %= a.n;
            if (base < 0) base += a.n;
        }
        for (int i = tid; i < XP_TILE + LPW; i += XP_THREADS) {
            int64_t m = base + i;
            float2 v = make_float2(0.f, 0.f);
            if (a.wrap) {
                if (m >= a.n) {
                    m -= a.n;
                    if (m >= a.n) m %= a.n;      // a frame shorter than the tile
                }
                v = srv[m];
            } else if (m >= 0 && m < a.n) {
                v = srv[m];
            }
            S[i] = v;
        }
        // seeds: exp(j 2 pi frac(f_d * i_last)) of every run, argument reduced in float64 (f i as an exact product)
        for (int k = tid; k < XP_RUNS * XP_DG; k += XP_THREADS) {
            const int r = k / XP_DG, d = k % XP_DG;
            const double il = (double)(t0 + r * XP_RUN + (XP_RUN - 1));
            const double f = FT[d];
            const double hi = f * il;
            const double lo = fma(f, il, -hi);
            const double fr = (hi - rint(hi)) + lo;
            double s, c;
            sincospi(2.0 * fr, &s, &c);
            SEED[k] = make_float2((float)c, (float)s);
        }
        __syncthreads();

        const int i0 = wave * XP_WAVE_SAMPLES;
        if (i0 < cnt) {
            float2 acct[XP_DG];
#pragma unroll
            for (int d = 0; d < XP_DG; ++d) acct[d] = make_float2(0.f, 0.f);
            const float2* Sl = S + ll;
            for (int r = sub; r < XP_WAVE_SAMPLES / XP_RUN; r += SUBS) {
                const int ib = i0 + r * XP_RUN;
                if (ib - sub * XP_RUN >= cnt) break;      // wave-uniform; P is zero from cnt on
                xp_v2f hx[XP_DG / 2], hy[XP_DG / 2];     // real and imaginary parts of a pair of Dopplers
#pragma unroll
                for (int d = 0; d < XP_DG / 2; ++d) hx[d] = hy[d] = xp_v2f{0.f, 0.f};
#pragma unroll 4
                for (int k = 0; k < XP_RUN; ++k) {
                    const float2 p = P[ib + k];
                    const float2 s = Sl[ib + k];
                    // p * conj(s), each part in both halves
                    const float qr = fmaf(p.y, s.y, p.x * s.x);
                    const float qi = fmaf(-p.x, s.y, p.y * s.x);
                    const xp_v2f qx = {qr, qr}, qy = {qi, qi};
#pragma unroll
                    for (int d = 0; d < XP_DG / 2; ++d) {
                        xp_v2f nx = __builtin_elementwise_fma(hx[d], zc[d], qx);
                        xp_v2f ny = __builtin_elementwise_fma(hx[d], zs[d], qy);
                        nx = __builtin_elementwise_fma(-hy[d], zs[d], nx);
                        ny = __builtin_elementwise_fma(hy[d], zc[d], ny);
                        hx[d] = nx;
                        hy[d] = ny;
                    }
                }
                const float2* sd = SEED + (wave * (XP_WAVE_SAMPLES / XP_RUN) + r) * XP_DG;
#pragma unroll
                for (int d = 0; d < XP_DG; ++d) cmac(acct[d], make_float2(hx[d / 2][d % 2], hy[d / 2][d % 2]), sd[d]);
            }
#pragma unroll
            for (int d = 0; d < XP_DG; ++d) {
                accd[d].x += (double)acct[d].x;
                accd[d].y += (double)acct[d].y;
            }
        }
        __syncthreads();
    }

    // the slices of a wavefront (every lane ends with the same bits), then the four wavefronts in wave order, in float64
#pragma unroll
    for (int sh = LPW; sh < 64; sh <<= 1) {
#pragma unroll
        for (int d = 0; d < XP_DG; ++d) {
            accd[d].x += __shfl_xor(accd[d].x, sh);
            accd[d].y += __shfl_xor(accd[d].y, sh);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int d = 0; d < XP_DG; ++d) RED[((wave - 1) * XP_DG + d) * 64 + lane] = accd[d];
    }
    __syncthreads();
    if (wave == 0) {
        const int l = L0 + ll;
        const int64_t cells = (int64_t)a.ndoppler * a.nlags;
        double2* w = a.ws + ((int64_t)ip * a.nchunks + chunk) * cells;
#pragma unroll
        for (int d = 0; d < XP_DG; ++d) {
            double2 s = accd[d];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const double2 o = RED[(v * XP_DG + d) * 64 + lane];
                s.x += o.x;
                s.y += o.y;
            }
            if (sub == 0 && l < a.nlags && D0 + d < a.ndoppler) w[(int64_t)(D0 + d) * a.nlags + l] = s;
        }
    }
}

// out[ip][cell] = the chunk sums of the cell, added in chunk order in float64, rounded once
__global__ __launch_bounds__(XP_THREADS) void xambg_patch_reduce_kernel(XpArgs a, float2* out) {
    const int64_t cells = (int64_t)a.ndoppler * a.nlags;
    const int64_t cell = (int64_t)blockIdx.x * XP_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const int ip = a.patch0 + blockIdx.y;
    const prc_patch pt = a.patches[ip];
    float2 r = make_float2(0.f, 0.f);
    if (xp_valid(pt, a.nframes, a.n)) {
        const double2* w = a.ws + (int64_t)ip * a.nchunks * cells + cell;
        double2 s = make_double2(0.0, 0.0);
        for (int c = 0; c < a.nchunks; ++c) {
            const double2 o = w[(int64_t)c * cells];
            s.x += o.x;
            s.y += o.y;
        }
        r = make_float2((float)s.x, (float)s.y);
    }
    out[(int64_t)ip * cells + cell] = r;
}

__device__ __forceinline__ double xp_mag2(float2 v) { return (double)v.x * (double)v.x + (double)v.y * (double)v.y; }

// off = (y- - y+) / (2 (y- - 2 y0 + y+)), clamped to +-1/2, 0 for a zero denominator
__device__ __forceinline__ double xp_parabola(double ym, double y0, double yp) {
    const double den = (ym - 2.0 * y0) + yp;
    if (den == 0.0) return 0.0;
    double off = 0.5 * (ym - yp) / den;
    if (off > 0.5) off = 0.5;
    if (off < -0.5) off = -0.5;
    if (!(off == off)) off = 0.0;
    return off;
}

__global__ __launch_bounds__(64) void xambg_patch_peaks_kernel(const prc_patch* patches, const float2* X, prc_patch_peak* peaks,
                                                              int nlags, int ndoppler, double step, int patch0) {
    const int lane = threadIdx.x;
    const int ip = patch0 + blockIdx.x;
    const int cells = ndoppler * nlags;
    const float2* Xp = X + (int64_t)ip * cells;
    double best = -1.0, least = INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < cells; c += 64) {
        const double m = xp_mag2(Xp[c]);
        if (m > best) {            // ascending c: the first of equal cells stays
            best = m;
            bi = c;
        }
        if (m < least) least = m;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const double ob = __shfl_xor(best, sh);
        const int oi = __shfl_xor(bi, sh);
        const double ol = __shfl_xor(least, sh);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
        if (ol < least) least = ol;
    }
    if (lane != 0) return;
    const prc_patch pt = patches[ip];
    const bool flat = bi == 0x7fffffff || !(best > least);
    if (flat) bi = 0;
    const int d = bi / nlags, l = bi % nlags;
    uint32_t flags = flat ? 4u : 0u;
    if (d == 0 || d == ndoppler - 1) flags |= 1u;
    if (l == 0 || l == nlags - 1) flags |= 2u;
    const double y0 = sqrt(xp_mag2(Xp[bi]));
    double off_d = 0.0, off_l = 0.0;
    if (!flat && !(flags & 1u)) off_d = xp_parabola(sqrt(xp_mag2(Xp[bi - nlags])), y0, sqrt(xp_mag2(Xp[bi + nlags])));
    if (!flat && !(flags & 2u)) off_l = xp_parabola(sqrt(xp_mag2(Xp[bi - 1])), y0, sqrt(xp_mag2(Xp[bi + 1])));
    prc_patch_peak pk;
    pk.lag = (double)pt.lag0 + ((double)l + off_l);
    pk.doppler = pt.doppler0 + ((double)d + off_d) * step;
    pk.amplitude = (float)y0;
    pk.d = d;
    pk.l = l;
    pk.flags = flags;
    peaks[ip] = pk;
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct XpShape {
    int64_t ntiles, tiles_per_chunk;
    int nchunks, nlg, ndg, lpw;
};

static int xp_check(prc_patch_desc* d, const prc_patch_desc* desc, int32_t npatches, bool peaks_only, XpShape* sh, const char* who) {
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_PATCH_DESC_SIZE_680, who, "prc_patch_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->nlags >= 1 && d->nlags <= PRC_PATCH_MAX_LAGS, PRC_EINVAL, "%s: nlags = %d outside 1 .. %d", who, d->nlags,
                PRC_PATCH_MAX_LAGS);
    PRC_REQUIRE(d->ndoppler >= 1 && d->ndoppler <= PRC_PATCH_MAX_DOPPLER, PRC_EINVAL, "%s: ndoppler = %d outside 1 .. %d", who,
                d->ndoppler, PRC_PATCH_MAX_DOPPLER);
    PRC_REQUIRE(std::isfinite(d->doppler_step), PRC_EINVAL, "%s: doppler_step is not finite", who);
    PRC_REQUIRE(npatches >= 0, PRC_EINVAL, "%s: npatches = %d", who, npatches);
    if (peaks_only) return PRC_OK;
    PRC_REQUIRE(d->n >= 1, PRC_EINVAL, "%s: n = %lld < 1", who, (long long)d->n);
    PRC_REQUIRE(d->nframes >= 1, PRC_EINVAL, "%s: nframes = %d < 1", who, d->nframes);
    PRC_REQUIRE(d->nframes == 1 || d->frame_stride >= d->n, PRC_EINVAL, "%s: frame_stride = %lld < n = %lld with %d frames", who,
                (long long)d->frame_stride, (long long)d->n, d->nframes);
    PRC_REQUIRE(d->wrap == 0 || d->wrap == 1, PRC_EINVAL, "%s: wrap = %d, not 0 or 1", who, d->wrap);
    PRC_REQUIRE(std::isfinite(d->sample_rate) && d->sample_rate != 0.0, PRC_EINVAL, "%s: sample_rate must be finite and non-zero",
                who);
    sh->ntiles = ceil_div64(d->n, XP_TILE);
    const int64_t want = sh->ntiles < XP_MAX_CHUNKS ? sh->ntiles : XP_MAX_CHUNKS;
    sh->tiles_per_chunk = ceil_div64(sh->ntiles, want);
    sh->nchunks = (int)ceil_div64(sh->ntiles, sh->tiles_per_chunk);
    sh->lpw = d->nlags <= XP_NARROW ? 16 : XP_LG;
    sh->nlg = (d->nlags + sh->lpw - 1) / sh->lpw;
    sh->ndg = (d->ndoppler + XP_DG - 1) / XP_DG;
    return PRC_OK;
}

extern "C" int prc_xambg_patch_workspace_bytes(const prc_patch_desc* desc, int32_t npatches, size_t* bytes) {
    prc_patch_desc d;
    XpShape sh;
    const int rc = xp_check(&d, desc, npatches, false, &sh, "prc_xambg_patch_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(bytes != nullptr, PRC_EINVAL, "prc_xambg_patch_workspace_bytes: null pointer");
    // at most 2^31 * 64 * 2^22 * 16 = 2^63: one patch fewer than that fits a size_t
    const unsigned __int128 b = (unsigned __int128)(npatches > 0 ? npatches : 1) * (unsigned)sh.nchunks * (unsigned)d.ndoppler *
                                (unsigned)d.nlags * sizeof(double2);
    PRC_REQUIRE(b <= (unsigned __int128)SIZE_MAX / 2, PRC_EINVAL, "prc_xambg_patch_workspace_bytes: size overflow");
    *bytes = (size_t)b;
    return PRC_OK;
}

extern "C" int prc_xambg_patch(const prc_patch_desc* desc, const void* ref, const void* srv, const float* window,
                               const prc_patch* patches, int32_t npatches, void* out, void* workspace, void* stream) {
    PRC_RANGE("prc_xambg_patch");
    prc_patch_desc d;
    XpShape sh;
    const int rc = xp_check(&d, desc, npatches, false, &sh, "prc_xambg_patch");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(ref && srv && patches && out && workspace, PRC_EINVAL, "prc_xambg_patch: null pointer");
    if (npatches == 0) return PRC_OK;
    XpArgs a;
    a.ref = static_cast<const float2*>(ref);
    a.srv = static_cast<const float2*>(srv);
    a.window = window;
    a.patches = patches;
    a.ws = static_cast<double2*>(workspace);
    a.n = d.n;
    a.frame_stride = d.frame_stride;
    a.ntiles = sh.ntiles;
    a.tiles_per_chunk = sh.tiles_per_chunk;
    a.sample_rate = d.sample_rate;
    a.step = d.doppler_step;
    a.nframes = d.nframes;
    a.nlags = d.nlags;
    a.ndoppler = d.ndoppler;
    a.wrap = d.wrap;
    a.nlg = sh.nlg;
    a.nchunks = sh.nchunks;
    const int64_t cells = (int64_t)d.ndoppler * d.nlags;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int p0 = 0; p0 < npatches; p0 += 65535) {      // grid.y / grid.z hold 65535
        const int np = npatches - p0 < 65535 ? npatches - p0 : 65535;
        a.patch0 = p0;
        const dim3 grid((unsigned)sh.nchunks, (unsigned)(sh.nlg * sh.ndg), (unsigned)np);
        if (sh.lpw == 16)
            hipLaunchKernelGGL(xambg_patch_kernel<16>, grid, dim3(XP_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL(xambg_patch_kernel<XP_LG>, grid, dim3(XP_THREADS), 0, st, a);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(xambg_patch_reduce_kernel, dim3((unsigned)ceil_div64(cells, XP_THREADS), (unsigned)np), dim3(XP_THREADS),
                           0, st, a, static_cast<float2*>(out));
        PRC_LAUNCH_CHECK();
    }
    return PRC_OK;
}

extern "C" int prc_xambg_patch_peaks(const prc_patch_desc* desc, const prc_patch* patches, int32_t npatches, const void* X,
                                     prc_patch_peak* peaks, void* stream) {
    PRC_RANGE("prc_xambg_patch_peaks");
    prc_patch_desc d;
    const int rc = xp_check(&d, desc, npatches, true, nullptr, "prc_xambg_patch_peaks");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(patches && X && peaks, PRC_EINVAL, "prc_xambg_patch_peaks: null pointer");
    if (npatches == 0) return PRC_OK;
    hipLaunchKernelGGL(xambg_patch_peaks_kernel, dim3((unsigned)npatches), dim3(64), 0, static_cast<hipStream_t>(stream), patches,
                       static_cast<const float2*>(X), peaks, d.nlags, d.ndoppler, d.doppler_step, 0);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
