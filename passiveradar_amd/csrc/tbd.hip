// Track-before-detect: Viterbi integration of a stack of statistic frames along every admissible path (include/prcore.h
// states the definition).  I_k[h, w] = z'_k[h, w] + alpha max over the predecessors of I_{k-1}, with a
// back pointer per cell and frame; the recursion is sequential in k and parallel in the cells.
//
// tbd_block_kernel, the time-blocked form: a 1024-thread workgroup owns a band of B rows at full width and advances nk <= K
// frames in one launch.  Two score buffers of R = B + 2 G rows (G = nk qd halo rows either side) of Wp = W + 2 qr floats sit in
// LDS.  Row h' is STAGED WITH ITS SHIFT APPLIED: column u of a staged row holds I[h'][u - s[h']] (-Inf where that is outside the
// frame, and in rows outside the frame), so the predecessor (h + dh, w - s[h + dh] + dw) of cell (h, w) is staged element
// (h + dh, w + dw) whatever the shifts are: the max loop walks (2 qd + 1) rows of (2 qr + 1) consecutive floats and does no
// index arithmetic and no bounds test (-Inf is never chosen).  Step j reads rows [j qd, R - j qd) of one buffer and writes
// rows [(j+1) qd, R - (j+1) qd) of the other: the halo shrinks by qd a step and after nk steps exactly the band is left.
// Every step writes the band's rows of score / back to memory.  Full-width rows: no column halo.
//   LDS: 2 R Wp 4 bytes <= PRC_TBD_LDS_BYTES (156 KiB of the 160 KiB a CDNA4 workgroup addresses; above 64 KiB by opt-in, as
//   plots.hip).  The flagship frame (1024 x 177, reach (1, 1), K = 8): Wp = 179, G = 8, B = 4 (tbd_plan), R = 20: 28 640 bytes.
//   Banks: a wavefront works on 64 consecutive columns of one row, so a ds_read_b32 / ds_write_b32 touches 64 consecutive
//   dwords: each 32-lane half covers the 32 banks once, conflict-free at every row stride -- rows need no padding beyond the
//   2 qr columns the predecessors reach into.
// tbd_frame_kernel, one frame per launch: one thread per cell, predecessors read from the previous score frame in global memory
// with the bounds tests of the definition (64-bit column arithmetic: any int32 shift).  For frames too wide for the blocked form.
// Both forms share tbd_input (z'), the ascending-code strict-greater choice and tbd_sum (one rounded product, one rounded sum):
// the same bytes.  tbd_trace_kernel: one thread per end, depth dependent byte loads.
#include "common.h"

#include <math.h>
#include <algorithm>

namespace {

constexpr int TT = 1024;                  // threads per workgroup, blocked form
constexpr int TWAVES = TT / PRC_WAVE;
constexpr int TU = 4;                     // items of a wavefront whose statistic is loaded together
constexpr int FT = 256;                   // threads per workgroup, one frame per launch and trace
constexpr int TBD_NONE = 255;
constexpr int TBD_CUS = 256;              // compute units of an MI355X

struct TbdArgs {
    const float* stat;        // first frame of this launch
    const float* prev;        // the score of the frame before it, or NULL: the recursion starts here (I = z', back = 255)
    float* score;             // first frame of this launch
    uint8_t* back;            // the same, or NULL
    const int32_t* shift;     // [H] or NULL
    int H, W, qd, qr;
    int wlo, whi, c0, c1;     // the excluded zones: w < wlo, w >= whi, Doppler column H-1-h in [c0, c1)
    int nk;                   // frames this launch advances (blocked form)
    int B;                    // rows of a band (blocked form)
    float alpha, clip;
};

__device__ __forceinline__ float tbd_input(const TbdArgs& a, int h, int w, float z) {
    const int c = a.H - 1 - h;
    if (w < a.wlo || w >= a.whi || (c >= a.c0 && c < a.c1)) return 0.0f;
    return z > a.clip ? a.clip : z;                 // a NaN stays
}

__device__ __forceinline__ float tbd_sum(float zp, float alpha, float best, int code) {
    const float m = code == TBD_NONE ? 0.0f : best;
    return __fadd_rn(zp, __fmul_rn(alpha, m));      // two roundings: never one fused operation
}

// A barrier that orders LDS traffic only.  A workgroup shares nothing through global memory inside a launch, and
// __syncthreads() would also wait for every global store and load in flight: one memory round trip per step.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// QD, QR >= 0: the reaches at compile time (the max loop unrolls); -1: from the arguments
template <int QD, int QR>
__global__ __launch_bounds__(TT) void tbd_block_kernel(TbdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tbd_lds[];
    const int qd = QD >= 0 ? QD : a.qd, qr = QR >= 0 ? QR : a.qr;
    const int H = a.H, W = a.W, Wp = W + 2 * qr;
    const int G = a.nk * qd, R = a.B + 2 * G;
    const int r0 = (int)blockIdx.x * a.B - G;       // the frame row of staged row 0
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int nch = (W + 63) >> 6;                  // 64-column pieces of a row
    const size_t HW = (size_t)H * (size_t)W;
    float* src = tbd_lds;
    float* dst = tbd_lds + R * Wp;

    // beyond +-(W + qr) a shift leaves no predecessor in bounds: clamped there, w + s cannot overflow
    auto shift_of = [&](int h) -> int {
        if (!a.shift) return 0;
        const int s = a.shift[h], lim = W + qr;
        return s > lim ? lim : (s < -lim ? -lim : s);
    };

    // Work of a step: items (row, 64-column piece) of its rows, item wave + TWAVES n to this wavefront as its n-th.  The
    // statistic of TU items is loaded before any of them is worked on, and the first TU items of step j + 1 are loaded before
    // step j's work: one memory latency per step is exposed, not one per item (plain loads stay in flight across the barrier).
    auto item = [&](int lo, int rows, int n, int& i, int& w, int& h) -> bool {
        const int it = wave + TWAVES * n;
        if (it >= rows * nch) return false;
        const int ir = it / nch;
        i = lo + ir;
        w = (it - ir * nch) * 64 + lane;
        h = r0 + i;
        return h >= 0 && h < H && w < W;
    };
    auto fetch = [&](int j, int n0, float (&z)[TU]) {
        const int lo = (j + 1) * qd, rows = R - 2 * lo;
        const float* x = a.stat + (size_t)j * HW;
#pragma unroll
        for (int u = 0; u < TU; ++u) {
            int i, w, h;
            z[u] = item(lo, rows, n0 + u, i, w, h) ? x[(size_t)h * W + w] : 0.0f;
        }
    };
    float zn[TU];
    fetch(0, 0, zn);

    for (int i = (int)threadIdx.x; i < 2 * R * Wp; i += TT) tbd_lds[i] = -INFINITY;
    lds_barrier();
    if (a.prev) {
        for (int it = wave; it < R * nch; it += TWAVES) {
            const int i = it / nch, w = (it - i * nch) * 64 + lane, h = r0 + i;
            if (h < 0 || h >= H || w >= W) continue;
            const int u = w + shift_of(h);
            if (u >= -qr && u < W + qr) src[i * Wp + u + qr] = a.prev[(size_t)h * W + w];
        }
        lds_barrier();
    }

    for (int j = 0; j < a.nk; ++j) {
        const int lo = (j + 1) * qd, rows = R - 2 * lo;      // staged rows [lo, lo + rows) are computed in this step
        const bool plain = j == 0 && !a.prev;
        for (int n0 = 0; wave + TWAVES * n0 < rows * nch; n0 += TU) {
            float z[TU];
            if (n0 == 0) {
#pragma unroll
                for (int u = 0; u < TU; ++u) z[u] = zn[u];
                if (j + 1 < a.nk) fetch(j + 1, 0, zn);       // in flight across this step's work and its barrier
            } else {
                fetch(j, n0, z);
            }
#pragma unroll
            for (int u = 0; u < TU; ++u) {
                int i, w, h;
                if (!item(lo, rows, n0 + u, i, w, h)) continue;
                const size_t cell = (size_t)h * W + w;
                const float zp = tbd_input(a, h, w, z[u]);
                float best = -INFINITY;
                int code = TBD_NONE;
                if (!plain) {
                    const float* p = src + (i - qd) * Wp + w;    // staged column w + dw + qr, from dw = -qr
                    int c = 0;
                    for (int dh = 0; dh <= 2 * qd; ++dh, p += Wp) {
                        for (int dw = 0; dw <= 2 * qr; ++dw, ++c) {
                            const float v = p[dw];
                            if (v > best) { best = v; code = c; }
                        }
                    }
                }
                const float I = tbd_sum(zp, a.alpha, best, code);
                const int us = w + shift_of(h);
                if (us >= -qr && us < W + qr) dst[i * Wp + us + qr] = I;
                if (i >= G && i < G + a.B) {
                    a.score[(size_t)j * HW + cell] = I;
                    if (a.back) a.back[(size_t)j * HW + cell] = (uint8_t)code;
                }
            }
        }
        lds_barrier();
        float* t = src; src = dst; dst = t;
    }
}

template <int QD, int QR>
__global__ __launch_bounds__(FT) void tbd_frame_kernel(TbdArgs a) {
    const int qd = QD >= 0 ? QD : a.qd, qr = QR >= 0 ? QR : a.qr;
    const int64_t W = a.W, H = a.H;
    const int64_t idx = (int64_t)blockIdx.x * FT + threadIdx.x;
    if (idx >= H * W) return;
    const int64_t h = idx / W, w = idx - h * W;
    const float zp = tbd_input(a, (int)h, (int)w, a.stat[idx]);
    float best = -INFINITY;
    int code = TBD_NONE;
    if (a.prev) {
        int c = 0;
        for (int dh = -qd; dh <= qd; ++dh) {
            const int64_t hp = h + dh;
            if (hp < 0 || hp >= H) { c += 2 * qr + 1; continue; }
            const int64_t base = w - (a.shift ? (int64_t)a.shift[hp] : 0);
            for (int dw = -qr; dw <= qr; ++dw, ++c) {
                const int64_t wp = base + dw;
                if (wp < 0 || wp >= W) continue;
                const float v = a.prev[hp * W + wp];
                if (v > best) { best = v; code = c; }
            }
        }
    }
    a.score[idx] = tbd_sum(zp, a.alpha, best, code);
    if (a.back) a.back[idx] = (uint8_t)code;
}

struct TraceArgs {
    const uint8_t* back;
    const int32_t* shift;     // or NULL
    const int32_t* ends;
    int32_t* paths;
    int H, W, qd, qr, nframes, nends, depth;
};

__global__ __launch_bounds__(FT) void tbd_trace_kernel(TraceArgs a) {
    const int e = (int)(blockIdx.x * FT + threadIdx.x);
    if (e >= a.nends) return;
    const int64_t W = a.W, H = a.H, HW = H * W;
    const int nr = 2 * a.qr + 1, ncodes = (2 * a.qd + 1) * nr;
    int32_t* out = a.paths + (size_t)e * (size_t)a.depth;
    const int64_t f = a.ends[2 * (size_t)e];
    int64_t cell = a.ends[2 * (size_t)e + 1];
    int j = 0;
    if (f >= 0 && f < a.nframes && cell >= 0 && cell < HW) {
        out[0] = (int32_t)cell;
        for (j = 1; j < a.depth && f - j >= 0; ++j) {
            const int code = a.back[(size_t)(f - j + 1) * (size_t)HW + (size_t)cell];
            if (code >= ncodes) break;                       // 255 and codes prc_tbd never writes
            const int64_t h = cell / W, w = cell - h * W;
            const int64_t hp = h + (code / nr - a.qd);
            if (hp < 0 || hp >= H) break;
            const int64_t wp = w - (a.shift ? (int64_t)a.shift[hp] : 0) + (code % nr - a.qr);
            if (wp < 0 || wp >= W) break;
            cell = hp * W + wp;
            out[j] = (int32_t)cell;
        }
    }
    for (; j < a.depth; ++j) out[j] = -1;
}

int tbd_check(prc_tbd_desc* d, const prc_tbd_desc* desc, const char* who) {
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_TBD_DESC_SIZE_MIN, who, "prc_tbd_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->H >= 1 && d->W >= 1, PRC_ESHAPE, "%s: H = %d, W = %d: a frame has at least one cell", who, d->H, d->W);
    PRC_REQUIRE((int64_t)d->H * d->W <= (int64_t)0x7fffffff, PRC_ESHAPE, "%s: H * W too large", who);
    PRC_REQUIRE(d->doppler_reach >= 0 && d->range_reach >= 0, PRC_EINVAL, "%s: doppler_reach = %d, range_reach = %d: not >= 0", who,
                d->doppler_reach, d->range_reach);
    PRC_REQUIRE((2 * (int64_t)d->doppler_reach + 1) * (2 * (int64_t)d->range_reach + 1) <= 255, PRC_EINVAL,
                "%s: reaches (%d, %d) give more than 255 predecessor codes", who, d->doppler_reach, d->range_reach);
    PRC_REQUIRE(d->range_guard >= 0 && d->doppler_guard >= 0, PRC_EINVAL, "%s: range_guard = %d, doppler_guard = %d: not >= 0", who,
                d->range_guard, d->doppler_guard);
    PRC_REQUIRE(d->alpha > 0.0f && d->alpha <= 1.0f, PRC_EINVAL, "%s: alpha = %g, not in (0, 1]", who, (double)d->alpha);
    PRC_REQUIRE(!isnan(d->clip), PRC_EINVAL, "%s: clip is NaN", who);
    return PRC_OK;
}

// frames per launch and rows per band of the blocked form; K = 1: one frame per launch
struct TbdPlan { int K, B; size_t lds; };

TbdPlan tbd_plan(const prc_tbd_desc& d) {
    TbdPlan p = {1, 0, 0};
    const int64_t optK = prc_opt(PRC_OPT_TBD_FRAMES), optB = prc_opt(PRC_OPT_TBD_ROWS);
    int64_t K = optK == 0 ? PRC_TBD_FRAMES : optK;
    const int64_t qd = d.doppler_reach;
    const int64_t row_bytes = 8 * ((int64_t)d.W + 2 * d.range_reach);      // one row of both buffers
    const int64_t Rmax = PRC_TBD_LDS_BYTES / row_bytes;
    if (d.H > (1 << 30)) return p;                                         // row arithmetic of the blocked form is 32-bit
    while (K >= 2 && Rmax < 1 + 2 * K * qd) --K;
    if (K < 2) return p;
    // one workgroup per compute unit of the MI355X where the frame has the rows for it: measured the fastest band height at
    // 1024 rows (taller bands leave compute units idle, shorter ones run the workgroups in two rounds)
    int64_t B = optB > 0 ? optB : (d.H + TBD_CUS - 1) / TBD_CUS;
    B = std::min<int64_t>(B, Rmax - 2 * K * qd);
    B = std::max<int64_t>(std::min<int64_t>(B, d.H), 1);
    p.K = (int)K;
    p.B = (int)B;
    p.lds = (size_t)((B + 2 * K * qd) * row_bytes);
    return p;
}

template <int QD, int QR>
int tbd_launch(const prc_tbd_desc& d, TbdArgs a, const float* stat, const float* prev, int32_t nframes, float* score, uint8_t* back,
               hipStream_t stream) {
    const TbdPlan p = tbd_plan(d);
    const size_t HW = (size_t)d.H * (size_t)d.W;
    if (p.K >= 2) {
        const int rc = prc_lds_optin(reinterpret_cast<const void*>(&tbd_block_kernel<QD, QR>), PRC_TBD_LDS_BYTES);
        if (rc) return rc;
    }
    for (int32_t k0 = 0; k0 < nframes; k0 += p.K) {
        a.stat = stat + (size_t)k0 * HW;
        a.prev = k0 ? score + (size_t)(k0 - 1) * HW : prev;
        a.score = score + (size_t)k0 * HW;
        a.back = back ? back + (size_t)k0 * HW : nullptr;
        a.nk = std::min<int32_t>(p.K, nframes - k0);
        a.B = p.B;
        if (p.K >= 2)
            hipLaunchKernelGGL((tbd_block_kernel<QD, QR>), dim3((unsigned)((d.H + p.B - 1) / p.B)), dim3(TT), p.lds, stream, a);
        else
            hipLaunchKernelGGL((tbd_frame_kernel<QD, QR>), dim3((unsigned)((HW + FT - 1) / FT)), dim3(FT), 0, stream, a);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

}  // namespace

extern "C" int prc_tbd(const prc_tbd_desc* desc, const float* stat, const int32_t* row_shift, const float* prev, int32_t nframes,
                       float* score, uint8_t* back, void* stream) {
    PRC_RANGE("prc_tbd");
    prc_tbd_desc d;
    const int rc = tbd_check(&d, desc, "prc_tbd");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_tbd: nframes = %d", nframes);
    if (nframes == 0) return PRC_OK;
    PRC_REQUIRE(stat && score, PRC_EINVAL, "prc_tbd: null pointer");
    TbdArgs a;
    memset(&a, 0, sizeof(a));
    a.shift = row_shift;
    a.H = d.H; a.W = d.W; a.qd = d.doppler_reach; a.qr = d.range_reach;
    a.wlo = d.range_guard;
    a.whi = d.W - std::min(d.range_guard, d.W);
    a.c0 = d.H / 2 - d.doppler_guard;
    a.c1 = (int)std::min<int64_t>((int64_t)d.H / 2 + d.doppler_guard, 0x7fffffff);
    a.alpha = d.alpha; a.clip = d.clip;
    if (d.doppler_reach == 1 && d.range_reach == 1)
        return tbd_launch<1, 1>(d, a, stat, prev, nframes, score, back, (hipStream_t)stream);
    return tbd_launch<-1, -1>(d, a, stat, prev, nframes, score, back, (hipStream_t)stream);
}

extern "C" int prc_tbd_trace(const prc_tbd_desc* desc, const uint8_t* back, const int32_t* row_shift, int32_t nframes,
                             const int32_t* ends, int32_t nends, int32_t depth, int32_t* paths, void* stream) {
    PRC_RANGE("prc_tbd_trace");
    prc_tbd_desc d;
    const int rc = tbd_check(&d, desc, "prc_tbd_trace");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nframes >= 0 && nends >= 0, PRC_EINVAL, "prc_tbd_trace: nframes = %d, nends = %d", nframes, nends);
    PRC_REQUIRE(depth >= 1, PRC_EINVAL, "prc_tbd_trace: depth = %d, not >= 1", depth);
    if (nends == 0) return PRC_OK;
    PRC_REQUIRE(ends && paths && (back || nframes == 0), PRC_EINVAL, "prc_tbd_trace: null pointer");
    TraceArgs a;
    a.back = back; a.shift = row_shift; a.ends = ends; a.paths = paths;
    a.H = d.H; a.W = d.W; a.qd = d.doppler_reach; a.qr = d.range_reach;
    a.nframes = nframes; a.nends = nends; a.depth = depth;
    hipLaunchKernelGGL(tbd_trace_kernel, dim3((unsigned)((nends + FT - 1) / FT)), dim3(FT), 0, (hipStream_t)stream, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
