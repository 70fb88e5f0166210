// Order-statistic CFAR (OS-CFAR, Rohling) beside CFAR_2D's cell average: the noise estimate of a cell is the k-th smallest
// of its training cells instead of their mean.  Same window as cfar.hip (tap (a, b) of cell (i, j) reads
// X[(i + c - a) mod H, (j + c - b) mod W], c = (fw-1)/2, taps outside the guard block [e1, e2)^2), so the two detectors
// differ only by the statistic.  DESIGN.md section 18.
//
// A rank is not separable, so every output looks at its Nt training cells in every sweep; the work is in needing few sweeps
// and few instructions per (cell, training value):
//   * float bits -> order-preserving uint32 keys once, on the tile load; everything after that is integer compares.
//   * selection = narrowing the KEY interval [lo, hm] that holds the answer, one counting sweep per step
//     (c = #{x < t}: one compare and one add-with-carry per training value).  The interval starts at the tile's own
//     [min, max] (one LDS atomic pair per thread), not at [0, 2^32): the sign and the exponent bits a tile shares cost nothing.
//     The first CO_INTERP_STEPS pivots are interpolated from the counts at the two ends (the rank says where in the
//     interval the answer should sit), later ones are midpoints, which bound the loop.
//   * the bisection stops as soon as  #{x < lo} == k-1  (the answer is the smallest value >= lo)  or  #{x <= hm} == k
//     (the largest value <= hm) -- at the latest when two values are left in the interval -- and ONE closing sweep takes
//     that minimum / maximum.  A cell of a Rayleigh map needs 5 sweeps on average and its wavefront, which waits for its
//     slowest cell, 9-10, instead of 32; maps full of ties fall through to lo == hm.
//   * a thread owns 4 adjacent columns of one row: the 4 windows share fw + 3 of their 4 fw columns, so a row of the
//     union is read once (ds_read_b128 at 16-byte aligned offsets in the compile-time form) and compared against 4 pivots.
// The loop is exact for every finite input and bounded for any bit pattern: NaNs are just keys.
#include "common.h"
#include "cfar_mean.h"
#include "order_select.h"

#define CO_TX 64          // outputs per workgroup: 16 rows x 64 columns, 256 threads x 4 adjacent columns
#define CO_TY 16
#define CO_R 4
#define CO_INTERP_STEPS 12                    // steps whose pivot is interpolated from the two counts; then midpoints
#define CO_MAX_STEPS (CO_INTERP_STEPS + 33)   // a midpoint step halves the interval's width: 32 of them reach lo == hm from any start

__host__ __device__ inline int co_pitch(int fw) { return (CO_TX + fw - 1 + (CO_R - 1) + 3) & ~3; }

// One row of the union of a thread's 4 windows: union column u (tile column 4 cx + u) is tap b = fw - 1 + o - u of output o.
// GROW: the row crosses the guard block.  f(o, x) sees every training value of output o in this row.
template <int FW, int E1C, int E2C, bool GROW, typename F>
__device__ __forceinline__ void co_row(const uint32_t* __restrict__ row, int fw, int e1, int e2, F&& f) {
    if (FW > 0) {
        constexpr int NQ = (FW + CO_R - 1 + 3) / 4;
        uint32_t x[NQ * 4];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(row)[q];
            x[4 * q] = v.x, x[4 * q + 1] = v.y, x[4 * q + 2] = v.z, x[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < FW + CO_R - 1; ++u) {
#pragma unroll
            for (int o = 0; o < CO_R; ++o) {
                const int b = FW - 1 + o - u;
                if (b >= 0 && b < FW && !(GROW && b >= E1C && b < E2C)) f(o, x[u]);
            }
        }
    } else {
        for (int u = 0; u < fw + CO_R - 1; ++u) {
            const uint32_t x = row[u];
#pragma unroll
            for (int o = 0; o < CO_R; ++o) {
                const int b = fw - 1 + o - u;
                if (b >= 0 && b < fw && !(GROW && b >= e1 && b < e2)) f(o, x);
            }
        }
    }
}

// every training value of the thread's 4 outputs, once: `base` = tile row (fw-1) + ty, column 4 cx (tap a reads row -a)
template <int FW, int E1C, int E2C, typename F>
__device__ __forceinline__ void co_sweep(const uint32_t* __restrict__ base, int pitch, int fw, int e1, int e2, F&& f) {
#pragma unroll 1
    for (int a = 0; a < e1; ++a) co_row<FW, E1C, E2C, false>(base - a * pitch, fw, e1, e2, f);
#pragma unroll 1
    for (int a = e1; a < e2; ++a) co_row<FW, E1C, E2C, true>(base - a * pitch, fw, e1, e2, f);
#pragma unroll 1
    for (int a = e2; a < fw; ++a) co_row<FW, E1C, E2C, false>(base - a * pitch, fw, e1, e2, f);
}

// FW > 0: compile-time widths (the reference's own CFAR_2D(18, 4) window), FW = 0: run-time widths.
template <typename TIn, int FW, int GW>
__global__ __launch_bounds__(256) void cfar_os_kernel(const TIn* __restrict__ X, int H, int W, int fw_rt, int e1_rt, int e2_rt,
                                                      int rank, int nt, int plain, const float* __restrict__ partial,
                                                      float thresh, int use_thresh, float* __restrict__ out,
                                                      float* __restrict__ noise) {
    constexpr int E1C = FW > 0 ? ((FW - GW) / 2 < 0 ? 0 : (FW - GW) / 2) : 0;
    constexpr int E2C = FW > 0 ? (FW - E1C + 1 > FW ? FW : FW - E1C + 1) : 0;
    const int fw = FW > 0 ? FW : fw_rt, e1 = FW > 0 ? E1C : e1_rt, e2 = FW > 0 ? E2C : e2_rt;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ uint32_t span[2];                             // the tile's smallest and largest key
    uint32_t* tile = reinterpret_cast<uint32_t*>(smem_raw);  // th x pitch keys
    const int th = CO_TY + fw - 1, tw = CO_TX + fw - 1, pitch = co_pitch(fw);
    const int f = blockIdx.z;
    const TIn* x = X + (int64_t)f * H * W;
    const int c = (fw - 1) / 2;
    const int i0 = blockIdx.y * CO_TY, j0 = blockIdx.x * CO_TX;
    if (threadIdx.x == 0) span[0] = 0xffffffffu, span[1] = 0u;
    __syncthreads();
    {
        // tile element (r, s) <-> X[(i0 + c - (fw-1) + r) mod H, (j0 + c - (fw-1) + s) mod W], as cfar_sep_kernel loads it
        const int tx = threadIdx.x & 63, tq = threadIdx.x >> 6;
        uint32_t kmin = 0xffffffffu, kmax = 0u;
        int ii = (i0 + c - (fw - 1) + tq) % H;
        if (ii < 0) ii += H;
        const int rstep = 4 % H, sstep = 64 % W;
        for (int r = tq; r < th; r += 4) {
            int jj = (j0 + c - (fw - 1) + tx) % W;
            if (jj < 0) jj += W;
            for (int s_ = tx; s_ < tw; s_ += 64) {
                const uint32_t k = prc_okey_raw(cfar_mag(x[(int64_t)ii * W + jj]));
                tile[r * pitch + s_] = k;
                kmin = min(kmin, k), kmax = max(kmax, k);
                jj += sstep;
                if (jj >= W) jj -= W;
            }
            ii += rstep;
            if (ii >= H) ii -= H;
        }
        atomicMin(&span[0], kmin);
        atomicMax(&span[1], kmax);
    }
    float mean_abs = 1.f;
    if (!plain) {
        float tot = 0.f;
        for (int k = 0; k < CFAR_MEAN_PARTIALS; ++k) tot += partial[(int64_t)f * CFAR_MEAN_PARTIALS + k];
        mean_abs = tot / (float)((int64_t)H * W);
    }
    __syncthreads();
    const int ty = threadIdx.x >> 4, cx = threadIdx.x & 15;  // a wavefront: 4 rows x 16 threads x 4 columns
    const int i = i0 + ty, jq = j0 + CO_R * cx;
    if (i >= H || jq >= W) return;                           // no barrier below
    const uint32_t* base = tile + ((fw - 1) + ty) * pitch + CO_R * cx;
    const uint32_t km1 = (uint32_t)(rank - 1), k = (uint32_t)rank;

    // invariant per output: the answer is in [lo, hm], clo = #{x < lo} <= k-1, chi = #{x <= hm} >= k
    uint32_t lo[CO_R], hm[CO_R], clo[CO_R], chi[CO_R];
    bool live[CO_R];
#pragma unroll
    for (int o = 0; o < CO_R; ++o) lo[o] = span[0], hm[o] = span[1], clo[o] = 0u, chi[o] = (uint32_t)nt, live[o] = jq + o < W;
    for (int step = 0; step < CO_MAX_STEPS; ++step) {
        bool done = true;
#pragma unroll
        for (int o = 0; o < CO_R; ++o) {
            live[o] = live[o] && lo[o] != hm[o] && clo[o] != km1 && chi[o] != k;
            done = done && !live[o];
        }
        if (__all(done)) break;
        uint32_t t[CO_R], cnt[CO_R];
#pragma unroll
        for (int o = 0; o < CO_R; ++o) {
            const uint32_t w = hm[o] - lo[o];                // >= 1 while live
            uint32_t off = w >> 1;
            if (step < CO_INTERP_STEPS) {
                // the k-th smallest sits about (k - clo - 1/2) / (chi - clo) of the way through the chi - clo values in
                // [lo, hm] (chi >= k > clo: the fraction is inside (0, 1)); float32 is plenty for a guess, and the guess is
                // a pure function of the cell's own state
                const float fr = ((float)(k - clo[o]) - 0.5f) / (float)(chi[o] - clo[o]);
                off = min((uint32_t)fminf(fr * (float)(w - 1u), 4294967040.0f), w - 1u);
            }
            t[o] = lo[o] + off + 1u, cnt[o] = 0u;            // lo < t <= hm while live
        }
        co_sweep<FW, E1C, E2C>(base, pitch, fw, e1, e2, [&](int o, uint32_t v) { cnt[o] += v < t[o] ? 1u : 0u; });
#pragma unroll
        for (int o = 0; o < CO_R; ++o) {
            if (live[o]) {
                if (cnt[o] <= km1) lo[o] = t[o], clo[o] = cnt[o];
                else hm[o] = t[o] - 1u, chi[o] = cnt[o];
            }
        }
    }
    // closing sweep: the smallest x - lo over x >= lo (values below lo wrap to huge ones), or the smallest hm - x over
    // x <= hm, written as (~x) - (~hm).  With lo == hm the answer is lo itself and is present: the minimum is 0.
    uint32_t flip[CO_R], off[CO_R], m[CO_R];
    bool open = false;
#pragma unroll
    for (int o = 0; o < CO_R; ++o) {
        const bool up = clo[o] == km1 || lo[o] == hm[o];
        flip[o] = up ? 0u : 0xffffffffu;
        off[o] = up ? lo[o] : ~hm[o];
        m[o] = lo[o] == hm[o] ? 0u : 0xffffffffu;
        open = open || (lo[o] != hm[o] && jq + o < W);
    }
    if (__any(open))
        co_sweep<FW, E1C, E2C>(base, pitch, fw, e1, e2, [&](int o, uint32_t v) { m[o] = min(m[o], (v ^ flip[o]) - off[o]); });
    const uint32_t* centre = tile + ((fw - 1) + ty - c) * pitch + (fw - 1) + CO_R * cx - c;
    const int64_t at = (int64_t)f * H * W + (int64_t)i * W + jq;
#pragma unroll
    for (int o = 0; o < CO_R; ++o) {
        if (jq + o >= W) break;
        const uint32_t ans = flip[o] ? hm[o] - m[o] : lo[o] + m[o];
        const float z = prc_key_value(ans) + 0.0f;                // -0 -> +0
        const float xv = prc_key_value(centre[o]);
        const float cr = plain ? xv / z : (xv / mean_abs) / (z + 1e-10f);
        out[at + o] = use_thresh ? (cr > thresh ? 1.f : 0.f) : cr;
        if (noise) noise[at + o] = z;
    }
}

static void co_window(int32_t fw, int32_t gw, int* e1, int* e2) {
    int a = (fw - gw) / 2;
    if (a < 0) a = 0;
    int b = fw - a + 1;
    if (b > fw) b = fw;
    *e1 = a, *e2 = b;
}

extern "C" int prc_cfar_training_cells(int32_t fw, int32_t gw, int32_t* ncells) {
    PRC_REQUIRE(ncells != nullptr, PRC_EINVAL, "prc_cfar_training_cells: null pointer");
    PRC_REQUIRE(fw > 0 && fw <= 32767 && gw >= 0, PRC_EINVAL, "prc_cfar_training_cells: fw = %d, gw = %d", fw, gw);
    int e1, e2;
    co_window(fw, gw, &e1, &e2);
    *ncells = fw * fw - (e2 - e1) * (e2 - e1);
    return PRC_OK;
}

struct CoShape { int e1, e2, nt, rank; size_t lds; };

static int co_check(prc_cfar_os_desc* d, const prc_cfar_os_desc* desc, int32_t nframes, CoShape* sh, const char* who) {
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_CFAR_OS_DESC_SIZE_MIN, who, "prc_cfar_os_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->H > 0 && d->W > 0 && d->fw > 0 && d->gw >= 0 && nframes > 0, PRC_EINVAL,
                "%s: bad size (H = %d, W = %d, fw = %d, gw = %d, nframes = %d)", who, d->H, d->W, d->fw, d->gw, nframes);
    PRC_REQUIRE(d->scale == PRC_CFAR_SCALE_REFERENCE || d->scale == PRC_CFAR_SCALE_PLAIN, PRC_EINVAL, "%s: scale = %d", who, d->scale);
    PRC_REQUIRE(d->input == 0 || d->input == 1, PRC_EINVAL, "%s: input = %d, not 0 (float32) or 1 (complex64)", who, d->input);
    sh->lds = sizeof(uint32_t) * ((size_t)CO_TY + d->fw - 1) * (size_t)co_pitch(d->fw < 4096 ? d->fw : 4096);
    PRC_REQUIRE(d->fw < 4096 && sh->lds <= 64 * 1024, PRC_EUNSUPPORTED,
                "%s: fw = %d: the 16 x 64 tile with its halo does not fit 64 KiB of LDS", who, d->fw);
    co_window(d->fw, d->gw, &sh->e1, &sh->e2);
    sh->nt = d->fw * d->fw - (sh->e2 - sh->e1) * (sh->e2 - sh->e1);
    PRC_REQUIRE(sh->nt > 0, PRC_EINVAL, "%s: the window (fw = %d, gw = %d) has no training cell", who, d->fw, d->gw);
    PRC_REQUIRE(d->rank >= 0 && d->rank <= sh->nt, PRC_EINVAL, "%s: rank = %d outside 1 .. %d training cells", who, d->rank, sh->nt);
    sh->rank = d->rank ? d->rank : (3 * sh->nt + 3) / 4;      // ceil(0.75 Nt)
    return PRC_OK;
}

extern "C" int prc_cfar_os_workspace_bytes(const prc_cfar_os_desc* desc, int32_t nframes, size_t* bytes) {
    prc_cfar_os_desc d;
    CoShape sh;
    const int rc = co_check(&d, desc, nframes, &sh, "prc_cfar_os_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(bytes != nullptr, PRC_EINVAL, "prc_cfar_os_workspace_bytes: null pointer");
    *bytes = d.scale == PRC_CFAR_SCALE_PLAIN ? 0 : sizeof(float) * (size_t)CFAR_MEAN_PARTIALS * (size_t)nframes;
    return PRC_OK;
}

template <typename TIn>
static void co_launch(const prc_cfar_os_desc& d, const CoShape& sh, const TIn* X, float* out, float* noise, int32_t nframes,
                      float* partial, hipStream_t stream) {
    const int plain = d.scale == PRC_CFAR_SCALE_PLAIN;
    const int64_t hw = (int64_t)d.H * d.W;
    for (int32_t f0 = 0; f0 < nframes; f0 += 65535) {         // gridDim.z
        const int32_t nf = nframes - f0 < 65535 ? nframes - f0 : 65535;
        const TIn* x = X + f0 * hw;
        float* o = out + f0 * hw;
        float* z = noise ? noise + f0 * hw : nullptr;
        float* p = partial ? partial + (size_t)f0 * CFAR_MEAN_PARTIALS : nullptr;
        if (!plain)
            hipLaunchKernelGGL(cfar_abs_partial_kernel<TIn>, dim3(CFAR_MEAN_PARTIALS, nf), dim3(256), 0, stream, x, hw, p);
        dim3 grid((d.W + CO_TX - 1) / CO_TX, (d.H + CO_TY - 1) / CO_TY, nf);
        if (d.fw == 18 && d.gw == 4)
            hipLaunchKernelGGL((cfar_os_kernel<TIn, 18, 4>), grid, dim3(256), sh.lds, stream, x, d.H, d.W, d.fw, sh.e1, sh.e2, sh.rank,
                               sh.nt, plain, p, d.thresh, d.use_thresh, o, z);
        else
            hipLaunchKernelGGL((cfar_os_kernel<TIn, 0, 0>), grid, dim3(256), sh.lds, stream, x, d.H, d.W, d.fw, sh.e1, sh.e2, sh.rank,
                               sh.nt, plain, p, d.thresh, d.use_thresh, o, z);
    }
}

extern "C" int prc_cfar_os(const prc_cfar_os_desc* desc, const void* X, float* out, float* noise, int32_t nframes,
                           void* workspace, void* stream) {
    PRC_RANGE("prc_cfar_os");
    prc_cfar_os_desc d;
    CoShape sh;
    const int rc = co_check(&d, desc, nframes, &sh, "prc_cfar_os");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(X && out, PRC_EINVAL, "prc_cfar_os: null pointer");
    PRC_REQUIRE(workspace || d.scale == PRC_CFAR_SCALE_PLAIN, PRC_EINVAL,
                "prc_cfar_os: the reference scale needs a workspace (prc_cfar_os_workspace_bytes)");
    if (d.input == 1) co_launch<float2>(d, sh, (const float2*)X, out, noise, nframes, (float*)workspace, (hipStream_t)stream);
    else co_launch<float>(d, sh, (const float*)X, out, noise, nframes, (float*)workspace, (hipStream_t)stream);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) { prc_set_error("prc_cfar_os: launch failed: %s", hipGetErrorString(le)); return PRC_EHIP; }
    return PRC_OK;
}
