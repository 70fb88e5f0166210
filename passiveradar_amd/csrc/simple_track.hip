// Single-target tracker on device: simple_target_tracker (target_detection.py:530-681).
//
// Per frame the reference normalises v / mean|v| (fp64, whole frame), takes s = fliplr(frame.T) (s[r, c] =
// frame[H-1-c, r]: range row r = storage column w, Doppler column c = H-1-h), zeroes s[:8], s[-8:] and s[:, 250:260],
// multiplies by the lock state's gate and takes np.argmax.  What that argmax can be depends only on the frame's class:
//   NaN in the frame, or all zeros  every cell is NaN (v/NaN, 0/0), so the first unmasked cell wins: (8, 0), or (0, 0)
//                                   when W <= 16 masks every row;
//   an Inf in the frame (mean Inf)  the unmasked +-Inf cells become Inf/Inf = NaN and stay NaN under any gate (NaN * 0),
//                                   every other cell is +-0: the first of those cells, else (0, 0);
//   positive finite mean            no NaN; cells outside the gate are v*0 = +-0 and masked cells +0, so the result is
//                                   the first maximum inside the gate if that maximum is > 0, else s[0, 0] (row 0 is
//                                   always masked, so flat index 0 always holds a zero).
// Division by a positive finite mean keeps the order of float32 values widened to fp64, so every comparison runs on the
// raw values and the mean's exact bits never matter (for float64 frames the reference's division may merge two values
// within about one ulp; those frames are the documented exception).
//
// strack_scan_kernel: P workgroups per frame, each over a band of storage rows, write one partial (sum |v|, NaN seen,
//   first unmasked Inf cell, the ungated maximum and its first s-flat index) to the workspace.  The frame is read once.
// strack_walk_kernel: ONE workgroup walks the frames in order.  It combines a frame's P partials, and for a gated frame
//   of positive finite mean reads only the gate window (at most 48 range x 96 Doppler cells: contiguous range segments
//   of storage rows), masks inside it and reduces.  The lock state and the adaptive Kalman update run in fp64 on every
//   thread (uniform, no broadcast); thread 0 writes the record with ordinary stores.
#include "common.h"

#include <math.h>

namespace {

constexpr int ST = 256;            // threads per scan / walk workgroup
constexpr int SW = ST / PRC_WAVE;  // wavefronts per workgroup
constexpr int MAX_PARTS = 16;      // scan workgroups per frame
constexpr int32_t NONE = 0x7fffffff;

struct Part {
    double sum;      // sum |v| over the band (fp64)
    double vmax;     // largest unmasked finite value (-inf: none)
    int32_t imax;    // its first s-flat index (NONE: none)
    int32_t iinf;    // first s-flat index of an unmasked +-Inf cell (NONE: none)
    int32_t nan;     // 1: a NaN in the band (masked or not: the mean sees the whole frame)
    int32_t pad;
};
static_assert(sizeof(Part) == 32, "Part layout");

__host__ __device__ inline int parts_for(int H, int W) {
    const int64_t n = (int64_t)H * W;
    int64_t p = (n + 16383) / 16384;
    if (p > MAX_PARTS) p = MAX_PARTS;
    if (p > H) p = H;
    return p < 1 ? 1 : (int)p;
}

__device__ __forceinline__ bool masked(int r, int c, int W) {
    // s[:8, :] = 0, s[-8:, :] = 0 (W < 8: the whole axis), s[:, 250:260] = 0 (empty for H <= 250)
    return r < 8 || r >= W - 8 || (c >= 250 && c < 260);
}

// (value, index) order of the argmax: larger value first, then smaller s-flat index
__device__ __forceinline__ void best_of(double& v, int32_t& i, double ov, int32_t oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void wave_best(double& v, int32_t& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, PRC_WAVE);
        const int32_t oi = __shfl_xor(i, o, PRC_WAVE);
        best_of(v, i, ov, oi);
    }
}

template <typename T>
__global__ __launch_bounds__(ST) void strack_scan_kernel(const T* __restrict__ frames, int H, int W, int rows_per,
                                                         Part* __restrict__ parts) {
    __shared__ Part red[SW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int P = parts_for(H, W);
    const int f = blockIdx.x / P, p = blockIdx.x - f * P;
    const int h0 = p * rows_per;
    const int h1 = min(H, h0 + rows_per);
    const T* x = frames + (size_t)f * (size_t)H * (size_t)W;
    double sum = 0.0, vmax = -INFINITY;
    int32_t imax = NONE, iinf = NONE, nan = 0;
    if (h0 < h1) {
        const int64_t end = (int64_t)h1 * W;
        // element i = h*W + w, walked with stride ST; (h, w) advanced without a division per element
        const int dh = ST / W, dw = ST % W;
        int h = h0 + tid / W, w = tid % W;
        for (int64_t i = (int64_t)h0 * W + tid; i < end; i += ST) {
            const double v = (double)x[i];
            sum += fabs(v);
            const int c = H - 1 - h;
            const int32_t si = w * H + c;
            if (isnan(v)) {
                nan = 1;
            } else if (!masked(w, c, W)) {
                if (isinf(v)) iinf = min(iinf, si);
                else best_of(vmax, imax, v, si);
            }
            w += dw;
            h += dh;
            if (w >= W) { w -= W; h += 1; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, PRC_WAVE);
        iinf = min(iinf, __shfl_xor(iinf, o, PRC_WAVE));
        nan |= __shfl_xor(nan, o, PRC_WAVE);
    }
    wave_best(vmax, imax);
    if (lane == 0) {
        red[wv].sum = sum; red[wv].vmax = vmax; red[wv].imax = imax; red[wv].iinf = iinf; red[wv].nan = nan;
    }
    __syncthreads();
    if (tid == 0) {
        Part o = red[0];
        for (int q = 1; q < SW; ++q) {
            o.sum += red[q].sum;
            o.iinf = min(o.iinf, red[q].iinf);
            o.nan |= red[q].nan;
            best_of(o.vmax, o.imax, red[q].vmax, red[q].imax);
        }
        o.pad = 0;
        parts[(size_t)f * P + p] = o;
    }
}

// simple_target_tracker's constants (:640-647) -- not multitarget_tracker's
__constant__ double kF1[16] = {1, 0, -0.003, 0, 0, 0, -0.003, -0.03, 0, 0, 1, 1, 0, 0, 0, 1};
__constant__ double kF2[16] = {1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1};
__constant__ double kQ[4] = {2.0, 0.02, 0.2, 0.05};
__constant__ double kP0[4] = {5.0, 0.0225, 0.04, 0.1};
constexpr double kR = 5.0;   // R = diag(5, 5)

struct State {
    double lock[4], m[2], e[2], x[4], P[16], S[4];
    int64_t idx[2];
};

__device__ void initial_state(State& s) {
    // :648-656.  The tuple is built as (lockMode, estimate, measurement, measIdx, ...) but the dtype's field order is
    // (lock_mode, measurement, measurement_idx, estimate, ...): measurement = H x0 = [30, -20], measurement_idx =
    // [35, -30], estimate = [50, 50] (intentional, as the reference)
    for (int i = 0; i < 4; ++i) s.lock[i] = i == 0 ? 1.0 : 0.0;
    s.m[0] = 30.0; s.m[1] = -20.0;
    s.idx[0] = 35; s.idx[1] = -30;
    s.e[0] = 50.0; s.e[1] = 50.0;
    s.x[0] = 30.0; s.x[1] = 2.0; s.x[2] = -20.0; s.x[3] = -1.0;
    for (int i = 0; i < 16; ++i) s.P[i] = (i % 5 == 0) ? kP0[i / 5] : 0.0;
    s.S[0] = 1.0; s.S[1] = 0.0; s.S[2] = 0.0; s.S[3] = 1.0;
}

__device__ void load_state(State& s, const prc_strack_record* r) {
    for (int i = 0; i < 4; ++i) s.lock[i] = r->lock_mode[i];
    for (int i = 0; i < 2; ++i) { s.m[i] = r->measurement[i]; s.idx[i] = r->measurement_idx[i]; s.e[i] = r->estimate[i]; }
    for (int i = 0; i < 4; ++i) s.x[i] = r->x[i];
    for (int i = 0; i < 16; ++i) s.P[i] = r->P[i];
    for (int i = 0; i < 4; ++i) s.S[i] = r->S[i];
}

__device__ void store_state(prc_strack_record* r, const State& s) {
    for (int i = 0; i < 4; ++i) r->lock_mode[i] = s.lock[i];
    for (int i = 0; i < 2; ++i) { r->measurement[i] = s.m[i]; r->measurement_idx[i] = s.idx[i]; r->estimate[i] = s.e[i]; }
    for (int i = 0; i < 4; ++i) r->x[i] = s.x[i];
    for (int i = 0; i < 16; ++i) r->P[i] = s.P[i];
    for (int i = 0; i < 4; ++i) r->S[i] = s.S[i];
}

// Python slice normalisation of [a, b) on an axis of length n (step 1)
__device__ __forceinline__ int64_t slice_end(int64_t a, int64_t n) {
    if (a < 0) {
        a += n;
        if (a < 0) a = 0;
    } else if (a > n) {
        a = n;
    }
    return a;
}

// simple_track_update (:539-624) after the argmax: measurement, lock state, adaptive_kalman_update (:63-114)
__device__ void step(State& s, int64_t i0, int64_t i1, int H, int W, double rext, double dext) {
    // range_meas = rangeExtent*(1 - i0/W), doppler_meas = dopplerExtent*(2*i1/H - 1): this operation order, bitwise
    const double z0 = __dmul_rn(rext, __dsub_rn(1.0, (double)i0 / (double)W));
    const double z1 = __dmul_rn(dext, __dsub_rn((double)(2 * i1) / (double)H, 1.0));
    const double d0 = __dsub_rn(z0, s.e[0]), d1 = __dsub_rn(z1, s.e[1]);
    const double h1 = __dmul_rn(0.5, d1);
    const bool found = sqrt(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(h1, h1))) < 12.0;
    // track_update_matrix @ lockMode: found 0->1, 1->2, 2->2, 3->2; not found 0->0, 1->0, 2->3, 3->0
    const double l0 = s.lock[0], l1 = s.lock[1], l2 = s.lock[2], l3 = s.lock[3];
    if (found) {
        s.lock[0] = 0.0; s.lock[1] = l0; s.lock[2] = l1 + l2 + l3; s.lock[3] = 0.0;
    } else {
        s.lock[0] = l0 + l1 + l3; s.lock[1] = 0.0; s.lock[2] = 0.0; s.lock[3] = l2;
    }
    // adaptive R: the squared distance to the PREVIOUS measurement
    const double r0 = z0 - s.m[0], r1 = z1 - s.m[1];
    const double scale = r0 * r0 + r1 * r1;
    double x[4], FP[16], P[16];
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 4; ++j) acc += kF1[4 * i + j] * s.x[j];
        x[i] = acc;
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += kF2[4 * i + q] * s.P[4 * q + j];
            FP[4 * i + j] = acc;
        }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += FP[4 * i + q] * kF2[4 * j + q];
            P[4 * i + j] = acc + (i == j ? kQ[i] : 0.0);
        }
    // S = H P H^T + R * scale; H picks state components 0 and 2; closed-form 2 x 2 inverse
    const double S[4] = {P[0] + kR * scale, P[2], P[8], P[10] + kR * scale};
    const double det = S[0] * S[3] - S[1] * S[2];
    const double Si[4] = {S[3] / det, -S[1] / det, -S[2] / det, S[0] / det};
    double K[8];
    for (int i = 0; i < 4; ++i) {           // K = P H^T S^-1
        K[2 * i] = P[4 * i] * Si[0] + P[4 * i + 2] * Si[2];
        K[2 * i + 1] = P[4 * i] * Si[1] + P[4 * i + 2] * Si[3];
    }
    const double y0 = z0 - x[0], y1 = z1 - x[2];
    for (int i = 0; i < 4; ++i) x[i] += K[2 * i] * y0 + K[2 * i + 1] * y1;
    for (int i = 0; i < 4; ++i)             // (I - K H) P
        for (int j = 0; j < 4; ++j)
            s.P[4 * i + j] = P[4 * i + j] - (K[2 * i] * P[j] + K[2 * i + 1] * P[8 + j]);
    for (int i = 0; i < 4; ++i) s.x[i] = x[i];
    for (int i = 0; i < 4; ++i) s.S[i] = S[i];
    s.m[0] = z0; s.m[1] = z1;
    s.idx[0] = i0; s.idx[1] = i1;
    s.e[0] = x[0]; s.e[1] = x[2];
}

template <typename T>
__global__ __launch_bounds__(ST) void strack_walk_kernel(const T* __restrict__ frames, int H, int W, int nframes,
                                                         int P, double rext, double dext, const Part* __restrict__ parts,
                                                         const prc_strack_record* state_in,
                                                         prc_strack_record* __restrict__ records) {
    __shared__ double red_v[2][SW];
    __shared__ int32_t red_i[2][SW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = (int64_t)H * W;
    State s;
    if (state_in) load_state(s, state_in);
    else initial_state(s);
    int nsync = 0;     // gated frames so far: their LDS slots alternate, so gated frame j+2 writes only after j+1's barrier
    for (int f = 0; f < nframes; ++f) {
        // the frame's class and its gate-independent answers, from the scan's partials (every thread, uniform)
        const Part* pp = parts + (size_t)f * P;
        double sum = 0.0, vmax = -INFINITY;
        int32_t imax = NONE, iinf = NONE, nan = 0;
        for (int q = 0; q < P; ++q) {
            const Part o = pp[q];
            sum += o.sum;
            iinf = min(iinf, o.iinf);
            nan |= o.nan;
            best_of(vmax, imax, o.vmax, o.imax);
        }
        const double mean = sum / (double)n;
        int32_t idx;
        if (nan || mean == 0.0) {
            idx = W > 16 ? 8 * H : 0;                        // every cell NaN: the first unmasked one, s[8, 0]
        } else if (isinf(mean)) {
            idx = iinf != NONE ? iinf : 0;                   // the first Inf/Inf = NaN cell, else all +-0
        } else {
            // gate (:566-584): lock state 1 or 3 -> s[ly-24:ly+24, lx-48:lx+48], 2 -> s[ly-16:ly+16, lx-32:lx+32]
            int dy = 0, dx = 0;
            if (s.lock[1] == 1.0) { dy = 24; dx = 48; }
            else if (s.lock[2] == 1.0) { dy = 16; dx = 32; }
            else if (s.lock[3] == 1.0) { dy = 24; dx = 48; }
            if (dy == 0) {
                idx = (imax != NONE && vmax > 0.0) ? imax : 0;
            } else {
                const int64_t ly = s.idx[0], lx = s.idx[1];
                const int ra = (int)slice_end(ly - dy, W), rb = (int)slice_end(ly + dy, W);
                const int ca = (int)slice_end(lx - dx, H), cb = (int)slice_end(lx + dx, H);
                const int nr = rb - ra, nc = cb - ca;
                double bv = -INFINITY;
                int32_t bi = NONE;
                if (nr > 0 && nc > 0) {
                    const T* x = frames + (size_t)f * (size_t)n;
                    // window cell q: Doppler column c = ca + q / nr, range row r = ra + q % nr; storage (H-1-c, r), so
                    // consecutive threads read consecutive range cells of one storage row
                    for (int q = tid; q < nr * nc; q += ST) {
                        const int c = ca + q / nr, r = ra + q % nr;
                        if (masked(r, c, W)) continue;
                        best_of(bv, bi, (double)x[(int64_t)(H - 1 - c) * W + r], r * H + c);
                    }
                }
                wave_best(bv, bi);
                const int buf = nsync++ & 1;
                if (lane == 0) { red_v[buf][wv] = bv; red_i[buf][wv] = bi; }
                __syncthreads();
                bv = red_v[buf][0];
                bi = red_i[buf][0];
                for (int q = 1; q < SW; ++q) best_of(bv, bi, red_v[buf][q], red_i[buf][q]);
                idx = (bi != NONE && bv > 0.0) ? bi : 0;
            }
        }
        step(s, idx / H, idx % H, H, W, rext, dext);
        if (tid == 0) store_state(records + f, s);
    }
}

}  // namespace

static int strack_check(prc_strack_desc* d, const prc_strack_desc* desc, const char* who) {
    PRC_REQUIRE(desc, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_STRACK_DESC_SIZE_630, who, "prc_strack_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->H >= 1 && d->W >= 1 && (int64_t)d->H * d->W <= (int64_t)0x7fffffff, PRC_EINVAL,
                "%s: H = %d, W = %d: need H, W >= 1 and H * W < 2^31", who, d->H, d->W);
    PRC_REQUIRE(d->dtype == PRC_REAL_F32 || d->dtype == PRC_REAL_F64, PRC_EINVAL,
                "%s: dtype = %d, not PRC_REAL_F32 (0) or PRC_REAL_F64 (1)", who, d->dtype);
    return PRC_OK;
}

extern "C" int prc_strack_workspace_bytes(const prc_strack_desc* desc, int32_t nframes, size_t* bytes) {
    prc_strack_desc d;
    const int rc = strack_check(&d, desc, "prc_strack_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_strack_workspace_bytes: null argument");
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_strack_workspace_bytes: nframes = %d", nframes);
    *bytes = (size_t)nframes * (size_t)parts_for(d.H, d.W) * sizeof(Part);
    return PRC_OK;
}

extern "C" int prc_strack_run(const prc_strack_desc* desc, const void* frames, int32_t nframes,
                              const prc_strack_record* state_in, prc_strack_record* records, void* workspace,
                              void* stream) {
    PRC_RANGE("prc_strack_run");
    prc_strack_desc d;
    const int rc = strack_check(&d, desc, "prc_strack_run");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_strack_run: nframes = %d", nframes);
    if (nframes == 0) return PRC_OK;
    PRC_REQUIRE(frames && records && workspace, PRC_EINVAL, "prc_strack_run: null argument");
    const int P = parts_for(d.H, d.W);
    const int rows_per = (d.H + P - 1) / P;
    Part* parts = (Part*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (d.dtype == PRC_REAL_F32) {
        hipLaunchKernelGGL(strack_scan_kernel<float>, dim3((uint32_t)P * (uint32_t)nframes), dim3(ST), 0, st, (const float*)frames, d.H,
                           d.W, rows_per, parts);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(strack_walk_kernel<float>, dim3(1), dim3(ST), 0, st, (const float*)frames, d.H, d.W, nframes,
                           P, d.range_extent, d.doppler_extent, parts, state_in, records);
    } else {
        hipLaunchKernelGGL(strack_scan_kernel<double>, dim3((uint32_t)P * (uint32_t)nframes), dim3(ST), 0, st, (const double*)frames, d.H,
                           d.W, rows_per, parts);
        PRC_LAUNCH_CHECK();
        hipLaunchKernelGGL(strack_walk_kernel<double>, dim3(1), dim3(ST), 0, st, (const double*)frames, d.H, d.W,
                           nframes, P, d.range_extent, d.doppler_extent, parts, state_in, records);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
