// LS_Filter_SVD (clutter_removal.py:58-107): truncated-SVD block least squares without the N x T matrix.
//
// The reference builds A[:, k] = roll(ref, k - peek) (complex64, N x T, T = filterLen + peek), takes its SVD, inverts the
// singular values it keeps and forms h = V S^-1 U^H srv, out = srv - A h.  A is made of circular shifts, so
//     G = A^H A   is the Hermitian Toeplitz matrix of the circular autocorrelation  c[k] = sum_m r[m] conj(r[(m+k) mod N]),
//     A^H srv     is the conjugate of the circular cross-correlation               b[k] = sum_m r[m] conj(s[(m+k) mod N]),
// with r the peek-rolled reference (the conventions of corr_partial_kernel in ls.hip), and with G = V L V^H, sigma_i =
// sqrt(lambda_i):  h = sum_kept v_i (v_i^H A^H srv) / lambda_i.
//
// Cut rule: a singular value is dropped when  sigma < max(1e-10, rcond * sigma_max).  rcond < 0 selects the default
// 4 sqrt(T) 2^-26 (lambda below 16 T 2^-52 lambda_max: what a Gram matrix accumulated in float64 cannot tell from its own
// rounding); rcond = 0 is the reference's absolute rule alone.
//
// Kernels, per block:
//   1. svd_corr_kernel    c and b in float64: every float32 x float32 product is exact in float64 and is accumulated by
//                         fp64 FMAs; tiles of r and s staged in LDS as doubles, lags across lanes, one double2 partial per
//                         workgroup (4096 samples) and lag;
//   2. svd_reduce_kernel  adds the partials in chunk order (no floating-point atomics anywhere: results are bit-identical
//                         run to run and do not depend on the batch);
//   3. svd_gram_kernel    W = G, V = I (T x T double2, column-major);
//   4. svd_jacobi_kernel  one launch per round of a round-robin pairing, one workgroup per column pair (p, q) of W and V:
//                         alpha = |w_p|^2, beta = |w_q|^2, gamma = w_p^H w_q, rotation when |gamma|^2 > tol^2 alpha beta;
//                         pairs inside the null space (both norms below T 2^-52 |G|_F) are skipped.
//                         No workgroup touches another's columns within a launch and none waits for another.  Rotations are
//                         counted per block and sweep; every launch of a sweep after a sweep without rotations returns at once;
//   5. svd_project_kernel lambda_i = v_i^H (G v_i) = v_i^H w_i (signed) and v_i^H A^H srv;
//   6. svd_select_kernel  the cut, the kept count, sigma sorted descending, info;
//   7. svd_taps_kernel    h = sum_kept v_i coef_i (complex128);
//   8. fir_subtract_kernel of ls.hip with circular = 1, twice: out = (srv - A hi) - A lo with h = hi + lo, hi the part of h
//                         that kernel's float32 taps carry.
// The host reads the rotation counters back once per sweep (one small copy and a stream synchronisation) and stops at the
// first sweep without rotations in any block, at most SVD_SWEEP_CAP sweeps: prc_ls_svd_execute is therefore NOT capturable
// into a graph, and returns with the Jacobi sweeps complete and the last five kernels enqueued.
#include "ls_internal.h"
#include <math.h>
#include <vector>

#define SVD_THREADS 256
#define SVD_TILE 1024                       // samples staged per pass
#define SVD_CHUNK 4096                      // samples per workgroup (one partial)
#define SVD_LG 2                            // lag groups of 64 per pass: 2 sources x 2 groups = 8 independent FMA chains per lane
#define SVD_SWEEP_CAP 30
#define SVD_CTR 32                          // rotation counters per block (one per sweep)
#define SVD_MAX_T 4096

// workspace: [taps: 2 x nblocks x T double2 (float32-representable part, remainder)][first FIR pass: nblocks x n float2][counters: nblocks x SVD_CTR int32][per block: partial, cb, W, V, lam, proj, coef]
struct SvdLayout {
    size_t taps, tmp, ctr, blocks;          // byte offsets of the shared regions and of block 0
    size_t partial, cb, W, V, lam, proj, coef, per_block;   // byte offsets inside a block's region, and its size
    int nchunk;
};

static size_t svd_up(size_t x) { return (x + 255) & ~(size_t)255; }

static SvdLayout svd_layout(int64_t n, int T, int nblocks) {
    SvdLayout l;
    l.nchunk = (int)ceil_div64(n, SVD_CHUNK);
    l.taps = 0;
    l.tmp = svd_up(sizeof(double2) * (size_t)2 * nblocks * T);
    l.ctr = l.tmp + svd_up(sizeof(float2) * (size_t)nblocks * n);
    l.blocks = l.ctr + svd_up(sizeof(int32_t) * (size_t)nblocks * SVD_CTR);
    size_t o = 0;
    l.partial = o; o += svd_up(sizeof(double2) * (size_t)l.nchunk * 2 * T);
    l.cb = o;      o += svd_up(sizeof(double2) * ((size_t)2 * T + 1));       // c, b, then |G|_F^2
    l.W = o;       o += svd_up(sizeof(double2) * (size_t)T * T);
    l.V = o;       o += svd_up(sizeof(double2) * (size_t)T * T);
    l.lam = o;     o += svd_up(sizeof(double) * (size_t)T);
    l.proj = o;    o += svd_up(sizeof(double2) * (size_t)T);
    l.coef = o;    o += svd_up(sizeof(double2) * (size_t)T);
    l.per_block = o;
    return l;
}

struct SvdArgs {
    const float2* ref;
    const float2* srv;
    int64_t stride, n;
    int32_t T, peek, nchunk, nblocks;
    unsigned char* ws;
    SvdLayout l;
    double rcond, tol2;
    double2* taps_out;       // [nblocks][T] or null
    double* sv_out;          // [nblocks][T] or null
    int32_t* info_out;       // [nblocks][3] or null
};

__device__ __forceinline__ unsigned char* svd_block(const SvdArgs& a, int b) { return a.ws + a.l.blocks + (size_t)b * a.l.per_block; }
__device__ __forceinline__ int32_t* svd_ctr(const SvdArgs& a, int b) { return reinterpret_cast<int32_t*>(a.ws + a.l.ctr) + (size_t)b * SVD_CTR; }

// ---- 1. circular correlations in float64 ------------------------------------------------------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_corr_kernel(SvdArgs a) {
    __shared__ double2 P[SVD_TILE];                              // r, then the four wavefronts' sums
    __shared__ double2 S[2][SVD_TILE + 64 * SVD_LG];             // r and s, SVD_LG lag groups further
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const float2* __restrict__ ref = a.ref + (int64_t)b * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)b * a.stride;
    const int64_t n = a.n, m_begin = (int64_t)chunk * SVD_CHUNK;
    const int64_t m_end = m_begin + SVD_CHUNK < n ? m_begin + SVD_CHUNK : n;
    const int T = a.T, peek = a.peek;
    double2* part = reinterpret_cast<double2*>(svd_block(a, b) + a.l.partial) + (size_t)chunk * 2 * T;
    for (int L0 = 0; L0 < T; L0 += 64 * SVD_LG) {
        double2 acc[2][SVD_LG];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < SVD_LG; ++g) acc[s][g] = make_double2(0.0, 0.0);
        for (int64_t t0 = m_begin; t0 < m_end; t0 += SVD_TILE) {
            const int cnt = m_end - t0 < SVD_TILE ? (int)(m_end - t0) : SVD_TILE;
            for (int i = tid; i < SVD_TILE; i += SVD_THREADS) {
                double2 v = make_double2(0.0, 0.0);
                if (i < cnt) {
                    int64_t idx = t0 + i + peek;                 // r[m] = ref[(m + peek) mod n], peek < n
                    if (idx >= n) idx -= n;
                    const float2 f = ref[idx];
                    v = make_double2((double)f.x, (double)f.y);
                }
                P[i] = v;
            }
            for (int i = tid; i < SVD_TILE + 64 * SVD_LG; i += SVD_THREADS) {
                const int64_t m = (t0 + i + L0) % n;             // the lagged index wraps, more than once when n is short
                int64_t idx = m + peek;
                if (idx >= n) idx -= n;
                const float2 fr = ref[idx], fs = srv[m];
                S[0][i] = make_double2((double)fr.x, (double)fr.y);
                S[1][i] = make_double2((double)fs.x, (double)fs.y);
            }
            __syncthreads();
            const int i0 = wave * (SVD_TILE / 4);
            const int i1 = i0 + SVD_TILE / 4 < cnt ? i0 + SVD_TILE / 4 : cnt;
#pragma unroll 2
            for (int i = i0; i < i1; ++i) {
                const double2 p = P[i];
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int g = 0; g < SVD_LG; ++g) {           // acc += p conj(q)
                        const double2 q = S[s][i + lane + 64 * g];
                        acc[s][g].x = fma(p.x, q.x, acc[s][g].x);
                        acc[s][g].x = fma(p.y, q.y, acc[s][g].x);
                        acc[s][g].y = fma(p.y, q.x, acc[s][g].y);
                        acc[s][g].y = fma(-p.x, q.y, acc[s][g].y);
                    }
            }
            __syncthreads();
        }
        double2* red = P;                                        // 4 waves x 2 x SVD_LG x 64 = SVD_TILE sums
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < SVD_LG; ++g) red[((wave * 2 + s) * SVD_LG + g) * 64 + lane] = acc[s][g];
        __syncthreads();
        for (int t = tid; t < 2 * SVD_LG * 64; t += SVD_THREADS) {
            double2 v = red[t];
#pragma unroll
            for (int w = 1; w < 4; ++w) {                        // the wavefronts in a fixed order
                const double2 u = red[w * 2 * SVD_LG * 64 + t];
                v.x += u.x;
                v.y += u.y;
            }
            const int s = t / (SVD_LG * 64);
            const int lag = L0 + (t - s * SVD_LG * 64);
            if (lag < T) part[(size_t)s * T + lag] = v;
        }
        __syncthreads();
    }
}
static_assert(4 * 2 * SVD_LG * 64 <= SVD_TILE, "the wavefront sums reuse the tile of r");

// ---- 2. partials in chunk order; the rotation counters start at zero ---------------------------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_reduce_kernel(SvdArgs a) {
    const int b = blockIdx.y, t = blockIdx.x * SVD_THREADS + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < SVD_CTR) svd_ctr(a, b)[threadIdx.x] = 0;
    if (t >= 2 * a.T) return;
    const double2* part = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.partial);
    double2 v = make_double2(0.0, 0.0);
    for (int c = 0; c < a.nchunk; ++c) {
        const double2 u = part[(size_t)c * 2 * a.T + t];
        v.x += u.x;
        v.y += u.y;
    }
    reinterpret_cast<double2*>(svd_block(a, b) + a.l.cb)[t] = v;
}

// sum of K doubles per thread over the workgroup by a fixed tree; every thread gets the totals
template <int K>
__device__ __forceinline__ void svd_block_sum(double (&v)[K], double (*sm)[SVD_THREADS], int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k][tid] = v[k];
    __syncthreads();
    for (int s = SVD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sm[k][tid] += sm[k][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sm[k][0];
    __syncthreads();
}

// |G|_F^2 = T |c[0]|^2 + 2 sum_d (T - d) |c[d]|^2 = sum_i lambda_i^2 >= lambda_max^2: the scale of the null threshold
__global__ __launch_bounds__(SVD_THREADS) void svd_norm_kernel(SvdArgs a) {
    __shared__ double sm[1][SVD_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
    double2* cb = reinterpret_cast<double2*>(svd_block(a, b) + a.l.cb);
    double r[1] = {0.0};
    for (int d = tid; d < T; d += SVD_THREADS) {
        const double2 c = cb[d];
        r[0] = fma((d ? 2.0 : 1.0) * (double)(T - d), c.x * c.x + c.y * c.y, r[0]);
    }
    svd_block_sum<1>(r, sm, tid);
    if (tid == 0) cb[2 * T] = make_double2(r[0], 0.0);
}

// ---- 3. W = G (G[j][k] = c[k-j] for k >= j, Hermitian), V = I ----------------------------------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_gram_kernel(SvdArgs a) {
    const int b = blockIdx.y, T = a.T;
    const int64_t idx = (int64_t)blockIdx.x * SVD_THREADS + threadIdx.x;
    if (idx >= (int64_t)T * T) return;
    const int k = (int)(idx / T), j = (int)(idx - (int64_t)k * T);       // column k, row j
    const double2* c = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.cb);
    reinterpret_cast<double2*>(svd_block(a, b) + a.l.W)[idx] = k >= j ? c[k - j] : zconj(c[j - k]);
    reinterpret_cast<double2*>(svd_block(a, b) + a.l.V)[idx] = make_double2(j == k ? 1.0 : 0.0, 0.0);
}

// ---- 4. one round of one-sided Jacobi on the columns of W (and the same rotations on V) --------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_jacobi_kernel(SvdArgs a, int sweep, int round) {
    __shared__ double sm[4][SVD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y, T = a.T;
    int32_t* ctr = svd_ctr(a, b);
    if (sweep > 0 && ctr[sweep - 1] == 0) return;               // converged: written by earlier launches only
    // round-robin: players 0 .. np-1 (np even; player T is the bye of an odd T), player np-1 stays, the others turn
    const int np = T + (T & 1), m = np - 1, i = blockIdx.x;
    const int pa = i == 0 ? m : (round + i) % m, pb = i == 0 ? round : (round - i + m) % m;
    const int p = pa < pb ? pa : pb, q = pa < pb ? pb : pa;
    if (q >= T) return;
    double2* W = reinterpret_cast<double2*>(svd_block(a, b) + a.l.W);
    double2* V = reinterpret_cast<double2*>(svd_block(a, b) + a.l.V);
    double2* wp = W + (size_t)p * T;
    double2* wq = W + (size_t)q * T;
    double r[4] = {0.0, 0.0, 0.0, 0.0};                           // alpha, beta, gamma = w_p^H w_q
    for (int j = tid; j < T; j += SVD_THREADS) {
        const double2 x = wp[j], y = wq[j];
        r[0] = fma(x.x, x.x, fma(x.y, x.y, r[0]));
        r[1] = fma(y.x, y.x, fma(y.y, y.y, r[1]));
        r[2] = fma(x.x, y.x, fma(x.y, y.y, r[2]));
        r[3] = fma(x.x, y.y, fma(-x.y, y.x, r[3]));
    }
    svd_block_sum<4>(r, sm, tid);
    const double alpha = r[0], beta = r[1], g2 = r[2] * r[2] + r[3] * r[3];
    // columns of the null space: |w| ~ |lambda| below T 2^-52 |G|_F (lambda_max <= |G|_F <= sqrt(T) lambda_max) is what the
    // rotations with the large columns leave of their rounding, and a pair of them is left alone: measured against c[0]
    // instead, such pairs converged only linearly and a periodic reference (rank 8 of 26) was still rotating after 30
    // sweeps.  A pair whose smaller column lies below T 2^-52 of the larger is left alone as well (sigma below
    // sqrt(T) 2^-26 of the larger one's: under the default cut); without it the same input does not converge either.
    const double gf2 = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.cb)[2 * T].x;
    const double nr2 = ((double)T * 0x1p-52) * ((double)T * 0x1p-52), nt2 = nr2 * gf2;
    if (alpha < nt2 && beta < nt2) return;
    if (fmin(alpha, beta) < nr2 * fmax(alpha, beta)) return;
    if (!(g2 > a.tol2 * alpha * beta)) return;
    if (tid == 0) atomicAdd(&ctr[sweep], 1);
    const double ag = sqrt(g2), zeta = (beta - alpha) / (2.0 * ag);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
    const double2 se = make_double2(sn * r[2] / ag, sn * r[3] / ag);     // s e^{i phi}, gamma = |gamma| e^{i phi}
    double2* vp = V + (size_t)p * T;
    double2* vq = V + (size_t)q * T;
    for (int j = tid; j < T; j += SVD_THREADS) {                  // x' = c x - conj(se) y,  y' = se x + c y
        double2 x = wp[j], y = wq[j];
        wp[j] = zsub(zscale(x, cs), zmul(zconj(se), y));
        wq[j] = zadd(zmul(se, x), zscale(y, cs));
        x = vp[j];
        y = vq[j];
        vp[j] = zsub(zscale(x, cs), zmul(zconj(se), y));
        vq[j] = zadd(zmul(se, x), zscale(y, cs));
    }
}

// ---- 5. lambda_i = v_i^H w_i (w_i = G v_i), proj_i = v_i^H (A^H srv) = v_i^H conj(b) ------------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_project_kernel(SvdArgs a) {
    __shared__ double sm[3][SVD_THREADS];
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y, T = a.T;
    const double2* w = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.W) + (size_t)i * T;
    const double2* v = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.V) + (size_t)i * T;
    const double2* bb = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.cb) + T;
    double r[3] = {0.0, 0.0, 0.0};
    for (int j = tid; j < T; j += SVD_THREADS) {
        const double2 x = v[j], y = w[j], z = bb[j];
        r[0] = fma(x.x, y.x, fma(x.y, y.y, r[0]));
        r[1] = fma(x.x, z.x, fma(-x.y, z.y, r[1]));                // conj(x) conj(z)
        r[2] = fma(-x.x, z.y, fma(-x.y, z.x, r[2]));
    }
    svd_block_sum<3>(r, sm, tid);
    if (tid == 0) {
        reinterpret_cast<double*>(svd_block(a, b) + a.l.lam)[i] = r[0];
        reinterpret_cast<double2*>(svd_block(a, b) + a.l.proj)[i] = make_double2(r[1], r[2]);
    }
}

// ---- 6. the cut: coef_i = proj_i / lambda_i for the directions kept, sigma sorted, info --------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_select_kernel(SvdArgs a) {
    __shared__ double smax[SVD_THREADS];
    __shared__ int skept;
    const int tid = threadIdx.x, b = blockIdx.x, T = a.T;
    const double* lam = reinterpret_cast<const double*>(svd_block(a, b) + a.l.lam);
    const double2* proj = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.proj);
    double2* coef = reinterpret_cast<double2*>(svd_block(a, b) + a.l.coef);
    double mx = 0.0;
    for (int i = tid; i < T; i += SVD_THREADS) mx = fmax(mx, lam[i]);
    smax[tid] = mx;
    if (tid == 0) skept = 0;
    __syncthreads();
    for (int s = SVD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) smax[tid] = fmax(smax[tid], smax[tid + s]);
        __syncthreads();
    }
    const double cut = fmax(1e-10, a.rcond * sqrt(smax[0]));
    int kept = 0;
    for (int i = tid; i < T; i += SVD_THREADS) {
        const double l = lam[i], sg = sqrt(fmax(l, 0.0));
        const bool keep = !(sg < cut);
        coef[i] = keep ? make_double2(proj[i].x / l, proj[i].y / l) : make_double2(0.0, 0.0);
        kept += keep;
        if (a.sv_out) {                                          // rank by counting: descending, ties by index
            int rank = 0;
            for (int j = 0; j < T; ++j) {
                const double sj = sqrt(fmax(lam[j], 0.0));
                rank += (sj > sg) || (sj == sg && j < i);
            }
            a.sv_out[(size_t)b * T + rank] = sg;
        }
    }
    if (kept) atomicAdd(&skept, kept);
    __syncthreads();
    if (tid == 0 && a.info_out) {
        const int32_t* ctr = svd_ctr(a, b);
        int sweeps = T > 1 ? SVD_SWEEP_CAP : 0, conv = T > 1 ? 0 : 1;
        for (int s = 0; s < SVD_SWEEP_CAP && T > 1; ++s)
            if (ctr[s] == 0) { sweeps = s + 1; conv = 1; break; }
        a.info_out[(size_t)b * 3 + 0] = skept;
        a.info_out[(size_t)b * 3 + 1] = sweeps;
        a.info_out[(size_t)b * 3 + 2] = conv;
    }
}

// ---- 7. h = V coef, the directions in index order ---------------------------------------------------------------------
__global__ __launch_bounds__(SVD_THREADS) void svd_taps_kernel(SvdArgs a) {
    const int b = blockIdx.y, T = a.T, j = blockIdx.x * SVD_THREADS + threadIdx.x;
    if (j >= T) return;
    const double2* V = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.V);
    const double2* coef = reinterpret_cast<const double2*>(svd_block(a, b) + a.l.coef);
    double2 h = make_double2(0.0, 0.0);
    for (int i = 0; i < T; ++i) {
        const double2 v = V[(size_t)i * T + j], c = coef[i];
        h.x = fma(v.x, c.x, fma(-v.y, c.y, h.x));
        h.y = fma(v.x, c.y, fma(v.y, c.x, h.y));
    }
    // the FIR kernel rounds its taps to float32: it runs twice, on the float32-representable part and on the remainder
    const double2 hi = make_double2((double)(float)h.x, (double)(float)h.y);
    double2* tw = reinterpret_cast<double2*>(a.ws + a.l.taps);
    tw[(size_t)b * T + j] = hi;
    tw[((size_t)a.nblocks + b) * T + j] = zsub(h, hi);
    if (a.taps_out) a.taps_out[(size_t)b * T + j] = h;
}

static int svd_check_sizes(const char* who, int64_t n, int32_t filter_len, int32_t peek, int32_t nblocks) {
    PRC_REQUIRE(filter_len >= 0 && peek >= 0 && nblocks > 0 && n > 0, PRC_EINVAL,
                "%s: non-positive size (n %lld, filter_len %d, peek %d, nblocks %d)", who, (long long)n, filter_len, peek, nblocks);
    PRC_REQUIRE(n < ((int64_t)1 << 31), PRC_ESHAPE, "%s: n = %lld exceeds the limit of %lld samples per block", who, (long long)n,
                (long long)(((int64_t)1 << 31) - 1));
    PRC_REQUIRE(nblocks <= PRC_MAX_BATCH, PRC_ESHAPE, "%s: nblocks = %d exceeds the limit of %d blocks (PRC_MAX_BATCH)", who, nblocks,
                PRC_MAX_BATCH);
    const int64_t T = (int64_t)filter_len + peek;
    PRC_REQUIRE(T >= 1 && T < n && T <= SVD_MAX_T, PRC_EINVAL,
                "%s: filter_len + peek = %lld taps, need 1 <= taps < n (%lld) and taps <= %d", who, (long long)T, (long long)n, SVD_MAX_T);
    return PRC_OK;
}

extern "C" int prc_ls_svd_workspace_bytes(int64_t n, int32_t filter_len, int32_t peek, int32_t nblocks, size_t* bytes) {
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_ls_svd_workspace_bytes: null argument");
    { const int rc = svd_check_sizes("prc_ls_svd_workspace_bytes", n, filter_len, peek, nblocks); if (rc) return rc; }
    const SvdLayout l = svd_layout(n, filter_len + peek, nblocks);
    *bytes = l.blocks + (size_t)nblocks * l.per_block;
    return PRC_OK;
}

// optional stage timing (tools/ls_svd_bench.py): events around correlate | Gram + Jacobi | project, select, taps | FIR of one
// execute, which then also waits for the FIR
static std::mutex g_svd_prof_mtx;
static int g_svd_prof_on = 0;
static double g_svd_prof_ms[4] = {0.0, 0.0, 0.0, 0.0};
static int g_svd_prof_sweeps = 0;

extern "C" int prc_ls_svd_set_profiling(int32_t enable) {
    std::lock_guard<std::mutex> lk(g_svd_prof_mtx);
    g_svd_prof_on = enable != 0;
    return PRC_OK;
}

extern "C" int prc_ls_svd_get_profile(double* ms, int32_t* sweeps) {
    PRC_REQUIRE(ms && sweeps, PRC_EINVAL, "prc_ls_svd_get_profile: null argument");
    std::lock_guard<std::mutex> lk(g_svd_prof_mtx);
    for (int i = 0; i < 4; ++i) ms[i] = g_svd_prof_ms[i];
    *sweeps = g_svd_prof_sweeps;
    return PRC_OK;
}

extern "C" int prc_ls_svd_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t filter_len, int32_t peek,
                                  double rcond, int32_t nblocks, void* out, int64_t out_stride, void* taps_out, double* sv_out,
                                  int32_t* info_out, void* workspace, void* stream_) {
    PRC_RANGE("prc_ls_svd_execute");
    PRC_REQUIRE(ref && srv && out && workspace, PRC_EINVAL, "prc_ls_svd_execute: null argument");
    { const int rc = svd_check_sizes("prc_ls_svd_execute", n, filter_len, peek, nblocks); if (rc) return rc; }
    PRC_REQUIRE(stride >= n && out_stride >= n, PRC_EINVAL, "prc_ls_svd_execute: stride shorter than n");
    PRC_REQUIRE(!(rcond != rcond) && rcond < 1.0, PRC_EINVAL, "prc_ls_svd_execute: rcond = %g, need rcond < 1 (negative: the default)", rcond);
    PRC_REQUIRE(((uintptr_t)workspace & 15) == 0, PRC_EINVAL, "prc_ls_svd_execute: the workspace must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const int T = filter_len + peek;
    SvdArgs a;
    a.ref = (const float2*)ref;
    a.srv = (const float2*)srv;
    a.stride = stride;
    a.n = n;
    a.T = T;
    a.peek = peek;
    a.nblocks = nblocks;
    a.ws = (unsigned char*)workspace;
    a.l = svd_layout(n, T, nblocks);
    a.nchunk = a.l.nchunk;
    a.rcond = rcond < 0.0 ? 4.0 * sqrt((double)T) * 0x1p-26 : rcond;
    // rotation threshold on |gamma| / sqrt(alpha beta): the rounding of a T-term float64 inner product, as LAPACK's
    // one-sided Jacobi takes it (sqrt(T) eps), with eps = 2^-52
    const double tol = sqrt((double)T) * 0x1p-52;
    a.tol2 = tol * tol;
    a.taps_out = (double2*)taps_out;
    a.sv_out = sv_out;
    a.info_out = info_out;
    const dim3 thr(SVD_THREADS);
    bool prof;
    { std::lock_guard<std::mutex> lk(g_svd_prof_mtx); prof = g_svd_prof_on != 0; }
    hipEvent_t ev[5];
    if (prof) for (int i = 0; i < 5; ++i) PRC_HIP(hipEventCreate(&ev[i]));
    if (prof) PRC_HIP(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(svd_corr_kernel, dim3((unsigned)a.nchunk, (unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    hipLaunchKernelGGL(svd_reduce_kernel, dim3((unsigned)ceil_div64(2 * T, SVD_THREADS), (unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    if (prof) PRC_HIP(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(svd_norm_kernel, dim3((unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    hipLaunchKernelGGL(svd_gram_kernel, dim3((unsigned)ceil_div64((int64_t)T * T, SVD_THREADS), (unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    int sweeps_run = 0;
    if (T > 1) {
        const int np = T + (T & 1);
        std::vector<int32_t> ctr((size_t)nblocks * SVD_CTR);
        for (int sweep = 0; sweep < SVD_SWEEP_CAP; ++sweep) {
            for (int round = 0; round < np - 1; ++round) {
                hipLaunchKernelGGL(svd_jacobi_kernel, dim3((unsigned)(np / 2), (unsigned)nblocks), thr, 0, stream, a, sweep, round);
                PRC_LAUNCH_CHECK();
            }
            PRC_HIP(hipMemcpyAsync(ctr.data(), a.ws + a.l.ctr, sizeof(int32_t) * ctr.size(), hipMemcpyDeviceToHost, stream));
            PRC_HIP(hipStreamSynchronize(stream));
            sweeps_run = sweep + 1;
            bool busy = false;
            for (int b = 0; b < nblocks; ++b) busy = busy || ctr[(size_t)b * SVD_CTR + sweep] != 0;
            if (!busy) break;
        }
    }
    if (prof) PRC_HIP(hipEventRecord(ev[2], stream));
    hipLaunchKernelGGL(svd_project_kernel, dim3((unsigned)T, (unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    hipLaunchKernelGGL(svd_select_kernel, dim3((unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    hipLaunchKernelGGL(svd_taps_kernel, dim3((unsigned)ceil_div64(T, SVD_THREADS), (unsigned)nblocks), thr, 0, stream, a);
    PRC_LAUNCH_CHECK();
    if (prof) PRC_HIP(hipEventRecord(ev[3], stream));
    // out = (srv - A hi) - A lo: with taps of 50 (a band-limited reference at the default cut) the
    // float32 rounding of the taps alone is 1e-4 of the output
    const double2* tw = reinterpret_cast<const double2*>(a.ws + a.l.taps);
    float2* tmp = reinterpret_cast<float2*>(a.ws + a.l.tmp);
    int rc = ls_launch_fir_circular((const float2*)ref, (const float2*)srv, tmp, tw, stride, stride, n, n, T, peek, nblocks, stream);
    if (rc == PRC_OK)
        rc = ls_launch_fir_circular((const float2*)ref, tmp, (float2*)out, tw + (size_t)nblocks * T, stride, n, out_stride, n, T,
                                    peek, nblocks, stream);
    if (prof) {
        PRC_HIP(hipEventRecord(ev[4], stream));
        PRC_HIP(hipEventSynchronize(ev[4]));
        std::lock_guard<std::mutex> lk(g_svd_prof_mtx);
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            PRC_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            g_svd_prof_ms[i] = ms;
        }
        g_svd_prof_sweeps = sweeps_run;
        for (int i = 0; i < 5; ++i) PRC_HIP(hipEventDestroy(ev[i]));
    }
    return rc;
}
