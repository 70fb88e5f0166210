// ECA_Filter: the extensive cancellation algorithm (Colone et al.) in LS_Filter_Toeplitz's convention -- the taps of ALL Doppler
// bins of LS_Filter_Multiple (clutter_removal.py:162-187) from ONE least-squares problem, where the chain solves one bin after
// another on the previous bin's output (one Gauss-Seidel sweep over subspaces that are far from orthogonal).
//
// B bins f_a, T = filterLen + peek taps per bin.  Regressors  r_a = roll(ref ramp_a, -peek),  ramp_a the float32-phase ramp of
// frequency_shift (signal_utils.py:24-27; phase_rot of common.h, evaluated at the sample's index BEFORE the roll: shift, then
// roll, as the chain does), r_a = roll(ref, -peek) when f_a = 0.  Linear lags, zero outside [0, n):
//     R_k[a][c] = sum_m r_c[m] conj(r_a[m-k])   (0 <= k < T;  R_-k = R_k^H),      y_k[a] = sum_m srv[m] conj(r_a[m-k]),
//     sum_j R_{i-j} x_j = y_i   (x_j in C^B; G Hermitian block-Toeplitz, reg added to the diagonal of R_0),
//     out = srv - sum_a (r_a * w_a)[0:n],  w_a[j] = x_j[a]     (linear FIR with zero history: np.convolve(...)[0:N]).
// With B = 1 this is LS_Filter_Toeplitz.
//
// Kernels, per block:
//   1. eca_corr_kernel    R and y in float64.  The regressors are rotated on the fly (B sincosf per staged sample; nothing of
//                         size n is written).  One workgroup per (chunk of samples, lagged bin a): r_a's lag window and the B + 1
//                         streams r_0 .. r_{B-1}, srv of a 256-sample tile are staged in LDS as doubles; lags across lanes,
//                         B + 1 sums per lane and lag group.  Every float32 x float32 product is exact in float64.
//   2. eca_reduce_kernel  adds the chunks' partial sums in chunk order, adds reg (no floating-point atomics anywhere: results
//                         are bit-identical run to run and do not depend on the batch).
//   3. eca_levinson_kernel  block Levinson, O(T^2 B^3), one workgroup per block, a fixed number of steps; forward and backward
//                         block predictors A, C (two copies each, so a step reads one and writes the other), x in the workspace,
//                         the B x B state (E_f, E_b, their Cholesky factors, reflection blocks) in LDS.
//   4. eca_apply_kernel   one launch, every bin: the taps stay complex128 (uniform loads), the window of each r_a is staged in
//                         LDS as doubles, fp64 FMAs, one rounding to float32 on the way out.
// Breakdown: a pivot of E_f or E_b that is not above 2^-40 R_0[i][i], or a non-finite one, or a non-finite tap, flags the block
// (info 1): zero taps, out = srv bit for bit, nothing non-finite is stored.  Nothing is read back: the call is capturable.
#include "common.h"
#include <math.h>

#define ECA_THREADS 256
#define ECA_LEV_THREADS 1024                // the block Levinson workgroup: its sums over j are latency-bound, so as many lanes as there are
#define ECA_LEV_PARTS 32                    // threads per output of those sums, at most (they are then added one after another)
#define ECA_TILE 256                        // samples staged per pass of the correlation (one per thread and stream)
#define ECA_LG 2                            // lag groups of 64 per pass
#define ECA_LAGS (64 * ECA_LG)
#define ECA_MIN_CHUNK 4096                  // samples per workgroup of the correlation, at least; and
#define ECA_MAX_CHUNKS 64                   // partial sums per block, lag and pair, at most
#define ECA_MAX_BINS 8
#define ECA_MAX_UNKNOWNS 4096               // nbins * T
#define ECA_OPT 4                           // outputs per thread of the apply kernel
#define ECA_SPAN (ECA_THREADS * ECA_OPT)
#define ECA_TAP_TILE 1024                   // taps per staged window of the apply kernel
#define ECA_PIVOT_FLOOR 0x1p-40             // of R_0's diagonal: below it a pivot is rounding, not signal (duplicate bins give
                                            // a few 2^-52; a cond(G) of 1e11 still passes)

// workspace: [taps: nblocks x B x T double2][per block: partial, R, y, A (2 copies), C (2 copies), x]
struct EcaLayout {
    size_t taps, blocks;                     // byte offsets of the shared region and of block 0
    size_t partial, R, y, A, C, x, per_block;   // byte offsets inside a block's region, and its size
    int64_t chunk;
    int nchunk;
};

static size_t eca_up(size_t x) { return (x + 255) & ~(size_t)255; }

static EcaLayout eca_layout(int64_t n, int T, int B, int nblocks) {
    EcaLayout l;
    int64_t chunk = ceil_div64(ceil_div64(n, ECA_MAX_CHUNKS), ECA_TILE) * ECA_TILE;       // a function of n alone
    l.chunk = chunk < ECA_MIN_CHUNK ? ECA_MIN_CHUNK : chunk;
    l.nchunk = (int)ceil_div64(n, l.chunk);
    l.taps = 0;
    l.blocks = eca_up(sizeof(double2) * (size_t)nblocks * B * T);
    size_t o = 0;
    l.partial = o; o += eca_up(sizeof(double2) * (size_t)l.nchunk * B * (B + 1) * T);
    l.R = o;       o += eca_up(sizeof(double2) * (size_t)T * B * B);
    l.y = o;       o += eca_up(sizeof(double2) * (size_t)T * B);
    l.A = o;       o += eca_up(sizeof(double2) * (size_t)2 * T * B * B);
    l.C = o;       o += eca_up(sizeof(double2) * (size_t)2 * T * B * B);
    l.x = o;       o += eca_up(sizeof(double2) * (size_t)T * B);
    l.per_block = o;
    return l;
}

struct EcaArgs {
    const float2* ref;
    const float2* srv;
    float2* out;
    int64_t stride, out_stride, n;
    int32_t T, peek, B, nblocks;
    unsigned char* ws;
    EcaLayout l;
    double reg;
    PhaseRamp pr[ECA_MAX_BINS];
    double2* taps_out;       // [nblocks][B][T] or null
    int32_t* info_out;       // [nblocks] or null
};

__device__ __forceinline__ unsigned char* eca_block(const EcaArgs& a, int b) { return a.ws + a.l.blocks + (size_t)b * a.l.per_block; }

// r_a[m], 0 <= m < n: the sample that the roll brings to m, rotated by the ramp at its own index (freq_shift_kernel of ls.hip)
__device__ __forceinline__ double2 eca_reg(const float2* __restrict__ ref, int64_t m, int64_t n, int peek, const PhaseRamp& pr) {
    int64_t idx = m + peek;
    if (idx >= n) idx -= n;
    float2 v = ref[idx];
    if (pr.enabled) v = cmul(v, phase_rot(pr, idx));
    return make_double2((double)v.x, (double)v.y);
}

// ---- 1. correlations in float64 ------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(ECA_THREADS) void eca_corr_kernel(EcaArgs a) {
    __shared__ double2 P[NB + 1][ECA_TILE];                       // r_c[m], c < NB, then srv[m]; afterwards the wavefronts' sums
    __shared__ double2 S[ECA_TILE + ECA_LAGS];                    // S[i] = r_a[t0 - L0 - (ECA_LAGS - 1) + i]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, ia = blockIdx.y, b = blockIdx.z;
    const float2* __restrict__ ref = a.ref + (int64_t)b * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)b * a.stride;
    const int64_t n = a.n, m_begin = (int64_t)chunk * a.l.chunk;
    const int64_t m_end = m_begin + a.l.chunk < n ? m_begin + a.l.chunk : n;
    const int T = a.T, peek = a.peek;
    const PhaseRamp pra = a.pr[ia];
    double2* part = reinterpret_cast<double2*>(eca_block(a, b) + a.l.partial) + ((size_t)chunk * NB + ia) * (NB + 1) * T;
    for (int L0 = 0; L0 < T; L0 += ECA_LAGS) {
        double2 acc[NB + 1][ECA_LG];
#pragma unroll
        for (int c = 0; c <= NB; ++c)
#pragma unroll
            for (int g = 0; g < ECA_LG; ++g) acc[c][g] = make_double2(0.0, 0.0);
        for (int64_t t0 = m_begin; t0 < m_end; t0 += ECA_TILE) {
            const int cnt = m_end - t0 < ECA_TILE ? (int)(m_end - t0) : ECA_TILE;
#pragma unroll
            for (int c = 0; c < NB; ++c)
                P[c][tid] = tid < cnt ? eca_reg(ref, t0 + tid, n, peek, a.pr[c]) : make_double2(0.0, 0.0);
            {
                double2 v = make_double2(0.0, 0.0);
                if (tid < cnt) {
                    const float2 f = srv[t0 + tid];
                    v = make_double2((double)f.x, (double)f.y);
                }
                P[NB][tid] = v;
            }
            for (int i = tid; i < ECA_TILE + ECA_LAGS - 1; i += ECA_THREADS) {
                const int64_t m = t0 - L0 - (ECA_LAGS - 1) + i;  // zero before the block; past it only under samples that are zero in P
                S[i] = (m >= 0 && m < n) ? eca_reg(ref, m, n, peek, pra) : make_double2(0.0, 0.0);
            }
            __syncthreads();
            const int j0 = wave * (ECA_TILE / 4);
            const int j1 = j0 + ECA_TILE / 4 < cnt ? j0 + ECA_TILE / 4 : cnt;
#pragma unroll 2
            for (int j = j0; j < j1; ++j) {
                double2 q[ECA_LG];
#pragma unroll
                for (int g = 0; g < ECA_LG; ++g) q[g] = S[j + (ECA_LAGS - 1) - (64 * g + lane)];       // r_a[m - k], k = L0 + 64 g + lane
#pragma unroll
                for (int c = 0; c <= NB; ++c) {
                    const double2 p = P[c][j];
#pragma unroll
                    for (int g = 0; g < ECA_LG; ++g) {           // acc += p conj(q)
                        acc[c][g].x = fma(p.x, q[g].x, acc[c][g].x);
                        acc[c][g].x = fma(p.y, q[g].y, acc[c][g].x);
                        acc[c][g].y = fma(p.y, q[g].x, acc[c][g].y);
                        acc[c][g].y = fma(-p.x, q[g].y, acc[c][g].y);
                    }
                }
            }
            __syncthreads();
        }
        double2* red = &P[0][0];                                 // (NB + 1) x ECA_LAGS sums, the wavefronts in a fixed order
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int c = 0; c <= NB; ++c)
#pragma unroll
                    for (int g = 0; g < ECA_LG; ++g) {
                        const int t = (c * ECA_LG + g) * 64 + lane;
                        double2 v = acc[c][g];
                        if (w) { v.x += red[t].x; v.y += red[t].y; }
                        red[t] = v;
                    }
            }
            __syncthreads();
        }
        for (int t = tid; t < (NB + 1) * ECA_LAGS; t += ECA_THREADS) {
            const int c = t / ECA_LAGS, lag = L0 + (t - c * ECA_LAGS);
            if (lag < T) part[(size_t)c * T + lag] = red[t];
        }
        __syncthreads();
    }
}
static_assert(ECA_LAGS <= ECA_TILE, "the wavefront sums reuse the tile of the streams");
static_assert(ECA_TILE == ECA_THREADS, "one staged sample per thread and stream");

// ---- 2. partials in chunk order -> R[k][a][c] (+ reg on R_0's diagonal), y[k][a] -----------------------------------------
__global__ __launch_bounds__(ECA_THREADS) void eca_reduce_kernel(EcaArgs a) {
    const int b = blockIdx.y, B = a.B, T = a.T;
    const int e = blockIdx.x * ECA_THREADS + threadIdx.x;
    if (e >= B * (B + 1) * T) return;
    const int k = e % T, c = (e / T) % (B + 1), ia = e / (T * (B + 1));
    const double2* part = reinterpret_cast<const double2*>(eca_block(a, b) + a.l.partial);
    double2 v = make_double2(0.0, 0.0);
    for (int ch = 0; ch < a.l.nchunk; ++ch) {
        const double2 u = part[(size_t)ch * B * (B + 1) * T + e];
        v.x += u.x;
        v.y += u.y;
    }
    if (c < B) {
        if (k == 0 && c == ia) v.x += a.reg;
        reinterpret_cast<double2*>(eca_block(a, b) + a.l.R)[((size_t)k * B + ia) * B + c] = v;
    } else {
        reinterpret_cast<double2*>(eca_block(a, b) + a.l.y)[(size_t)k * B + ia] = v;
    }
}

// ---- 3. block Levinson ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void zfma(double2& acc, double2 p, double2 q) {           // acc += p q
    acc.x = fma(p.x, q.x, fma(-p.y, q.y, acc.x));
    acc.y = fma(p.x, q.y, fma(p.y, q.x, acc.y));
}
__device__ __forceinline__ void zfms(double2& acc, double2 p, double2 q) {           // acc -= p q
    acc.x = fma(-p.x, q.x, fma(p.y, q.y, acc.x));
    acc.y = fma(-p.x, q.y, fma(-p.y, q.x, acc.y));
}

// L L^H = E (Hermitian positive definite; its lower triangle is read), one thread.  false: a pivot at or below the floor, or
// a non-finite one
__device__ bool eca_chol(const double2* E, double2* L, int B, const double* d0) {
    for (int j = 0; j < B; ++j) {
        double s = E[j * B + j].x;
        for (int k = 0; k < j; ++k) s -= L[j * B + k].x * L[j * B + k].x + L[j * B + k].y * L[j * B + k].y;
        if (!(s > ECA_PIVOT_FLOOR * d0[j]) || !(s < INFINITY)) return false;
        const double d = sqrt(s);
        L[j * B + j] = make_double2(d, 0.0);
        for (int i = j + 1; i < B; ++i) {
            double2 v = E[i * B + j];
            for (int k = 0; k < j; ++k) zfms(v, L[i * B + k], zconj(L[j * B + k]));
            L[i * B + j] = make_double2(v.x / d, v.y / d);
        }
    }
    return true;
}
// X[:, col] <- (L L^H)^-1 X[:, col] in place (X has ld columns), one thread
__device__ void eca_chol_solve(const double2* L, int B, double2* X, int ld, int col) {
    for (int i = 0; i < B; ++i) {
        double2 v = X[i * ld + col];
        for (int k = 0; k < i; ++k) zfms(v, L[i * B + k], X[k * ld + col]);
        const double d = L[i * B + i].x;
        X[i * ld + col] = make_double2(v.x / d, v.y / d);
    }
    for (int i = B - 1; i >= 0; --i) {
        double2 v = X[i * ld + col];
        for (int k = i + 1; k < B; ++k) zfms(v, zconj(L[k * B + i]), X[k * ld + col]);
        const double d = L[i * B + i].x;
        X[i * ld + col] = make_double2(v.x / d, v.y / d);
    }
}

// State: A_j, C_j (j <= m), E_f, E_b, x_j.  A_0 = C_0 = I, E_f = E_b = R_0, x_0 = R_0^-1 y_0; for m = 0 .. T-2
//   D_f = sum_j R_{m+1-j} A_j,  D_b = sum_j R_{-1-j} C_j,  rho = y_{m+1} - sum_j R_{m+1-j} x_j          (j <= m)
//   K_A = E_b^-1 D_f,  K_B = E_f^-1 D_b,  A <- [A; 0] - [0; C] K_A,  C <- [0; C] - [A; 0] K_B  (both from the old A, C)
//   E_f <- E_f - D_b K_A,  E_b <- E_b - D_f K_B  (both from the old values),  x <- [x; 0] + C E_b^-1 rho  (new C, E_b)
__global__ __launch_bounds__(ECA_LEV_THREADS) void eca_levinson_kernel(EcaArgs a) {
    constexpr int M = ECA_MAX_BINS, MM = M * M;
    __shared__ double2 Ef[MM], Eb[MM], Lf[MM], Lb[MM], KA[MM], KB[MM], Df[MM], Db[MM], rho[M], psum[ECA_LEV_THREADS];
    __shared__ double d0[M];
    __shared__ int bad;
    const int tid = threadIdx.x, b = blockIdx.x, B = a.B, BB = B * B, T = a.T;
    const double2* R = reinterpret_cast<const double2*>(eca_block(a, b) + a.l.R);
    const double2* y = reinterpret_cast<const double2*>(eca_block(a, b) + a.l.y);
    double2* Abuf = reinterpret_cast<double2*>(eca_block(a, b) + a.l.A);
    double2* Cbuf = reinterpret_cast<double2*>(eca_block(a, b) + a.l.C);
    double2* x = reinterpret_cast<double2*>(eca_block(a, b) + a.l.x);
    const size_t half = (size_t)T * BB;                          // one copy of A (or C)
    if (tid < BB) {
        const double2 v = R[tid];
        Ef[tid] = v;
        Eb[tid] = v;
        const double2 id = make_double2(tid / B == tid % B ? 1.0 : 0.0, 0.0);
        Abuf[tid] = id;
        Cbuf[tid] = id;
    }
    if (tid < B) {
        d0[tid] = R[tid * B + tid].x;
        rho[tid] = y[tid];
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid == 0) {
        if (eca_chol(Ef, Lf, B, d0)) {
            for (int i = 0; i < BB; ++i) Lb[i] = Lf[i];
            eca_chol_solve(Lf, B, rho, 1, 0);
            for (int i = 0; i < B; ++i) x[i] = rho[i];
        } else {
            bad = 1;
        }
    }
    __syncthreads();
    const int nout = 2 * BB + B, parts = ECA_LEV_THREADS / nout < ECA_LEV_PARTS ? ECA_LEV_THREADS / nout : ECA_LEV_PARTS;   // nout <= 136
    int cur = 0;
    for (int m = 0; m + 1 < T && !bad; ++m) {
        const double2* A = Abuf + cur * half;
        const double2* C = Cbuf + cur * half;
        double2* An = Abuf + (cur ^ 1) * half;
        double2* Cn = Cbuf + (cur ^ 1) * half;
        // D_f, D_b and R x: every output by `parts` threads over interleaved j, then the parts in order
        if (tid < nout * parts) {
            const int o = tid % nout, p = tid / nout;
            double2 s = make_double2(0.0, 0.0);
            if (o < BB) {
                const int r = o / B, c = o % B;
                for (int j = p; j <= m; j += parts) {
                    const double2* Rk = R + (size_t)(m + 1 - j) * BB;
                    const double2* Aj = A + (size_t)j * BB;
                    for (int i = 0; i < B; ++i) zfma(s, Rk[r * B + i], Aj[i * B + c]);
                }
            } else if (o < 2 * BB) {
                const int r = (o - BB) / B, c = (o - BB) % B;
                for (int j = p; j <= m; j += parts) {
                    const double2* Rk = R + (size_t)(1 + j) * BB;            // R_{-1-j} = R_{1+j}^H
                    const double2* Cj = C + (size_t)j * BB;
                    for (int i = 0; i < B; ++i) zfma(s, zconj(Rk[i * B + r]), Cj[i * B + c]);
                }
            } else {
                const int r = o - 2 * BB;
                for (int j = p; j <= m; j += parts) {
                    const double2* Rk = R + (size_t)(m + 1 - j) * BB;
                    const double2* xj = x + (size_t)j * B;
                    for (int i = 0; i < B; ++i) zfma(s, Rk[r * B + i], xj[i]);
                }
            }
            psum[tid] = s;
        }
        __syncthreads();
        if (tid < nout) {
            double2 s = psum[tid];
            for (int p = 1; p < parts; ++p) s = zadd(s, psum[p * nout + tid]);
            if (tid < BB) Df[tid] = s;
            else if (tid < 2 * BB) Db[tid - BB] = s;
            else rho[tid - 2 * BB] = zsub(y[(size_t)(m + 1) * B + (tid - 2 * BB)], s);
        }
        __syncthreads();
        if (tid < B) {                                           // K_A = E_b^-1 D_f, a column per thread
            for (int i = 0; i < B; ++i) KA[i * B + tid] = Df[i * B + tid];
            eca_chol_solve(Lb, B, KA, B, tid);
        } else if (tid >= 64 && tid < 64 + B) {                  // K_B = E_f^-1 D_b
            const int c = tid - 64;
            for (int i = 0; i < B; ++i) KB[i * B + c] = Db[i * B + c];
            eca_chol_solve(Lf, B, KB, B, c);
        }
        __syncthreads();
        for (int e = tid; e < (m + 2) * BB; e += ECA_LEV_THREADS) {
            const int j = e / BB, rc = e - j * BB, r = rc / B, c = rc - r * B;
            const bool ha = j <= m, hc = j >= 1;                 // [A; 0] has block j, [0; C] has block j
            const double2* Aj = A + (size_t)j * BB;
            const double2* Cj = C + (size_t)(j - 1) * BB;
            double2 va = ha ? Aj[rc] : make_double2(0.0, 0.0);
            double2 vc = hc ? Cj[rc] : make_double2(0.0, 0.0);
            if (hc)
                for (int i = 0; i < B; ++i) zfms(va, Cj[r * B + i], KA[i * B + c]);
            if (ha)
                for (int i = 0; i < B; ++i) zfms(vc, Aj[r * B + i], KB[i * B + c]);
            An[e] = va;
            Cn[e] = vc;
        }
        if (tid < BB) {                                          // E_f -= D_b K_A: an element reads only itself of E_f
            const int r = tid / B, c = tid % B;
            double2 v = Ef[tid];
            for (int i = 0; i < B; ++i) zfms(v, Db[r * B + i], KA[i * B + c]);
            Ef[tid] = v;
        } else if (tid >= 64 && tid < 64 + BB) {                 // E_b -= D_f K_B
            const int t = tid - 64, r = t / B, c = t % B;
            double2 v = Eb[t];
            for (int i = 0; i < B; ++i) zfms(v, Df[r * B + i], KB[i * B + c]);
            Eb[t] = v;
        }
        __syncthreads();
        if (tid == 0) {
            if (!eca_chol(Ef, Lf, B, d0)) bad = 1;
        } else if (tid == 64) {
            if (eca_chol(Eb, Lb, B, d0)) eca_chol_solve(Lb, B, rho, 1, 0);
            else bad = 1;
        }
        __syncthreads();
        if (!bad) {
            for (int e = tid; e < (m + 2) * B; e += ECA_LEV_THREADS) {           // x_j += C_j (E_b^-1 rho)
                const int j = e / B, r = e - j * B;
                double2 v = j <= m ? x[e] : make_double2(0.0, 0.0);
                const double2* Cj = Cn + (size_t)j * BB;
                for (int i = 0; i < B; ++i) zfma(v, Cj[r * B + i], rho[i]);
                x[e] = v;
            }
        }
        cur ^= 1;
        __syncthreads();
    }
    for (int e = tid; e < T * B; e += ECA_LEV_THREADS) {
        const double2 v = x[e];
        if (!bad && (!(fabs(v.x) < INFINITY) || !(fabs(v.y) < INFINITY))) bad = 1;     // only ever set
    }
    __syncthreads();
    const int flagged = bad;
    double2* tw = reinterpret_cast<double2*>(a.ws + a.l.taps) + (size_t)b * B * T;
    for (int e = tid; e < T * B; e += ECA_LEV_THREADS) {
        const int j = e / B, ia = e - j * B;
        const double2 v = flagged ? make_double2(0.0, 0.0) : x[e];
        tw[(size_t)ia * T + j] = v;
        if (a.taps_out) a.taps_out[((size_t)b * B + ia) * T + j] = v;
    }
    if (tid == 0 && a.info_out) a.info_out[b] = flagged;
}

// ---- 4. out = srv - sum_a (r_a * w_a)[0:n] --------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(ECA_THREADS) void eca_apply_kernel(EcaArgs a) {
    __shared__ double2 W[ECA_SPAN + ECA_TAP_TILE - 1];           // W[i] = r_a[n0 - k0 - halo + i]
    const int tid = threadIdx.x, b = blockIdx.y, T = a.T;
    const int64_t n0 = (int64_t)blockIdx.x * ECA_SPAN;
    const float2* __restrict__ ref = a.ref + (int64_t)b * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)b * a.stride;
    double2 acc[ECA_OPT];
#pragma unroll
    for (int o = 0; o < ECA_OPT; ++o) acc[o] = make_double2(0.0, 0.0);
#pragma unroll
    for (int ia = 0; ia < NB; ++ia) {
        const double2* __restrict__ taps = reinterpret_cast<const double2*>(a.ws + a.l.taps) + ((size_t)b * NB + ia) * T;
        for (int k0 = 0; k0 < T; k0 += ECA_TAP_TILE) {
            const int tk = T - k0 < ECA_TAP_TILE ? T - k0 : ECA_TAP_TILE, halo = tk - 1;
            __syncthreads();                                     // the previous window is dead
            for (int i = tid; i < ECA_SPAN + halo; i += ECA_THREADS) {
                const int64_t m = n0 - k0 - halo + i;            // zero history, nothing past the block
                W[i] = (m >= 0 && m < a.n) ? eca_reg(ref, m, a.n, a.peek, a.pr[ia]) : make_double2(0.0, 0.0);
            }
            __syncthreads();
            const double2* Wl = W + tid + halo;
#pragma unroll 2
            for (int k = 0; k < tk; ++k) {
                const double2 w = taps[k0 + k];
#pragma unroll
                for (int o = 0; o < ECA_OPT; ++o) zfma(acc[o], w, Wl[o * ECA_THREADS - k]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < ECA_OPT; ++o) {
        const int64_t m = n0 + tid + o * ECA_THREADS;
        if (m < a.n) {
            const float2 s = srv[m];
            a.out[(int64_t)b * a.out_stride + m] = make_float2((float)((double)s.x - acc[o].x), (float)((double)s.y - acc[o].y));
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static int eca_check_sizes(const char* who, int64_t n, int32_t filter_len, int32_t peek, int32_t nbins, int32_t nblocks) {
    PRC_REQUIRE(filter_len >= 0 && peek >= 0 && nblocks > 0 && n > 0, PRC_EINVAL,
                "%s: non-positive size (n %lld, filter_len %d, peek %d, nblocks %d)", who, (long long)n, filter_len, peek, nblocks);
    PRC_REQUIRE(nbins >= 1 && nbins <= ECA_MAX_BINS, PRC_EINVAL, "%s: %d Doppler bins, need 1 .. %d", who, nbins, ECA_MAX_BINS);
    PRC_REQUIRE(n < ((int64_t)1 << 31), PRC_ESHAPE, "%s: n = %lld exceeds the limit of %lld samples per block", who, (long long)n,
                (long long)(((int64_t)1 << 31) - 1));
    PRC_REQUIRE(nblocks <= PRC_MAX_BATCH, PRC_ESHAPE, "%s: nblocks = %d exceeds the limit of %d blocks (PRC_MAX_BATCH)", who, nblocks,
                PRC_MAX_BATCH);
    const int64_t T = (int64_t)filter_len + peek;
    PRC_REQUIRE(T >= 1 && T < n && T * nbins <= ECA_MAX_UNKNOWNS, PRC_EINVAL,
                "%s: filter_len + peek = %lld taps, need 1 <= taps < n (%lld) and nbins * taps <= %d", who, (long long)T, (long long)n,
                ECA_MAX_UNKNOWNS);
    return PRC_OK;
}

extern "C" int prc_eca_workspace_bytes(int64_t n, int32_t filter_len, int32_t peek, int32_t nbins, int32_t nblocks, size_t* bytes) {
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_eca_workspace_bytes: null argument");
    { const int rc = eca_check_sizes("prc_eca_workspace_bytes", n, filter_len, peek, nbins, nblocks); if (rc) return rc; }
    const EcaLayout l = eca_layout(n, filter_len + peek, nbins, nblocks);
    *bytes = l.blocks + (size_t)nblocks * l.per_block;
    return PRC_OK;
}

// optional stage timing (tools/eca_bench.py): events around correlate | solve | apply of one execute, which then also waits
// for the apply kernel
static std::mutex g_eca_prof_mtx;
static int g_eca_prof_on = 0;
static double g_eca_prof_ms[3] = {0.0, 0.0, 0.0};

extern "C" int prc_eca_set_profiling(int32_t enable) {
    std::lock_guard<std::mutex> lk(g_eca_prof_mtx);
    g_eca_prof_on = enable != 0;
    return PRC_OK;
}

extern "C" int prc_eca_get_profile(double* ms) {
    PRC_REQUIRE(ms, PRC_EINVAL, "prc_eca_get_profile: null argument");
    std::lock_guard<std::mutex> lk(g_eca_prof_mtx);
    for (int i = 0; i < 3; ++i) ms[i] = g_eca_prof_ms[i];
    return PRC_OK;
}

#define ECA_FOR_NB(NBV, STMT)                                                                                  \
    switch (NBV) {                                                                                             \
        case 1: { constexpr int NB = 1; STMT; } break;                                                         \
        case 2: { constexpr int NB = 2; STMT; } break;                                                         \
        case 3: { constexpr int NB = 3; STMT; } break;                                                         \
        case 4: { constexpr int NB = 4; STMT; } break;                                                         \
        case 5: { constexpr int NB = 5; STMT; } break;                                                         \
        case 6: { constexpr int NB = 6; STMT; } break;                                                         \
        case 7: { constexpr int NB = 7; STMT; } break;                                                         \
        default: { constexpr int NB = 8; STMT; } break;                                                        \
    }

extern "C" int prc_eca_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t filter_len, int32_t peek,
                               double sample_rate, const double* doppler_bins_host, int32_t nbins, double reg, int32_t nblocks,
                               void* out, int64_t out_stride, void* taps_out, int32_t* info_out, void* workspace, void* stream_) {
    PRC_RANGE("prc_eca_execute");
    PRC_REQUIRE(ref && srv && out && workspace && doppler_bins_host, PRC_EINVAL, "prc_eca_execute: null argument");
    { const int rc = eca_check_sizes("prc_eca_execute", n, filter_len, peek, nbins, nblocks); if (rc) return rc; }
    PRC_REQUIRE(stride >= n && out_stride >= n, PRC_EINVAL, "prc_eca_execute: stride shorter than n");
    PRC_REQUIRE(reg >= 0.0 && reg < INFINITY, PRC_EINVAL, "prc_eca_execute: reg = %g, need a finite reg >= 0", reg);
    PRC_REQUIRE(sample_rate != 0.0 && sample_rate == sample_rate, PRC_EINVAL, "prc_eca_execute: sample_rate = %g", sample_rate);
    PRC_REQUIRE(((uintptr_t)workspace & 15) == 0, PRC_EINVAL, "prc_eca_execute: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int T = filter_len + peek, B = nbins;
    EcaArgs a;
    a.ref = (const float2*)ref;
    a.srv = (const float2*)srv;
    a.out = (float2*)out;
    a.stride = stride;
    a.out_stride = out_stride;
    a.n = n;
    a.T = T;
    a.peek = peek;
    a.B = B;
    a.nblocks = nblocks;
    a.ws = (unsigned char*)workspace;
    a.l = eca_layout(n, T, B, nblocks);
    a.reg = reg;
    for (int i = 0; i < ECA_MAX_BINS; ++i) {                     // the ramp of prc_frequency_shift (make_ramp of ls.hip)
        const double fc = i < B ? doppler_bins_host[i] : 0.0;
        a.pr[i].a32 = (float)(2.0 * 3.14159265358979323846 * fc);
        a.pr[i].rcp32 = 1.0f / (float)sample_rate;
        a.pr[i].off32 = 0.f;
        a.pr[i].enabled = fc != 0.0 ? 1 : 0;
    }
    a.taps_out = (double2*)taps_out;
    a.info_out = info_out;
    const dim3 thr(ECA_THREADS);
    bool prof;
    { std::lock_guard<std::mutex> lk(g_eca_prof_mtx); prof = g_eca_prof_on != 0; }
    hipEvent_t ev[4];
    if (prof) for (int i = 0; i < 4; ++i) PRC_HIP(hipEventCreate(&ev[i]));
    if (prof) PRC_HIP(hipEventRecord(ev[0], stream));
    ECA_FOR_NB(B, hipLaunchKernelGGL(eca_corr_kernel<NB>, dim3((unsigned)a.l.nchunk, (unsigned)B, (unsigned)nblocks), thr, 0, stream, a));
    PRC_LAUNCH_CHECK();
    hipLaunchKernelGGL(eca_reduce_kernel, dim3((unsigned)ceil_div64((int64_t)B * (B + 1) * T, ECA_THREADS), (unsigned)nblocks), thr, 0,
                       stream, a);
    PRC_LAUNCH_CHECK();
    if (prof) PRC_HIP(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(eca_levinson_kernel, dim3((unsigned)nblocks), dim3(ECA_LEV_THREADS), 0, stream, a);
    PRC_LAUNCH_CHECK();
    if (prof) PRC_HIP(hipEventRecord(ev[2], stream));
    ECA_FOR_NB(B, hipLaunchKernelGGL(eca_apply_kernel<NB>, dim3((unsigned)ceil_div64(n, ECA_SPAN), (unsigned)nblocks), thr, 0, stream, a));
    PRC_LAUNCH_CHECK();
    if (prof) {
        PRC_HIP(hipEventRecord(ev[3], stream));
        PRC_HIP(hipEventSynchronize(ev[3]));
        std::lock_guard<std::mutex> lk(g_eca_prof_mtx);
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            PRC_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            g_eca_prof_ms[i] = ms;
        }
        for (int i = 0; i < 4; ++i) PRC_HIP(hipEventDestroy(ev[i]));
    }
    return PRC_OK;
}
