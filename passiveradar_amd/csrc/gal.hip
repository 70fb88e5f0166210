// Gradient adaptive lattice joint-process estimator (GAL_JPE, clutter_removal.py:251-365), one wavefront per stream.
//
// Per sample n (x = ref[n + peek], bo = the previous step's b, lattice length L <= delay length D):
//   f[m] = x - sum_{j=1..m} conj(k[j]) bo[j-1]                      (an inclusive prefix sum over the lattice taps)
//   b[0] = x;  b[m] = bo[m-1] - k[m] f[m-1]  (1 <= m < L);  b[m] = bo[m-1]  (L <= m < D: the delay line)
//   P[m-1] = 0.9 P[m-1] + 0.19 (|f[m-1]|^2 + |bo[m-1]|^2);  k[m] += mu1 (conj(f[m-1]) b[m] + bo[m-1] conj(f[m])) / (P[m-1] + 1e-10)
//   e = srv[n] - h^H b;  h += mu2 conj(e) b / (b^H b + 1e-10);  out[n] = e
//   mu1 = min(0.999 mu1 + 1e-8 e^2, 5e-3)   -- e^2, not |e|^2: mu1 is complex, and min() is NumPy's lexicographic order
// Element m needs only bo[m-1] (a shift by one element) and its own f[m]: every update is local once the prefix sum is
// known.  Only the L lattice elements need the lattice arithmetic; a delay-line element (m >= L) needs its shift, its share
// of h^H b and b^H b, and its h update.
//
// Two one-wavefront forms (D <= 2048), each templated on TPL = elements per lane:
// * gal_row_kernel, L <= 64 (short lattices: the HipBackend mode's 8, the reference's ballpark): element m = 64 t + lane,
//   row t.  Row 0 is the whole lattice (k, P, one DPP wave scan for f); rows 1.. are the delay line and hold b and h only
//   (4 VGPRs per element).  The delay line shifts in registers: one DPP wave_shr per row with the row below's lane 63 (two
//   v_readlane) entering lane 0.  That is the history window of b[L-1] the delay line is, kept where its reader is: an LDS
//   window would read each element's b back per step instead (a ds_read per row).
// * gal_lattice_kernel, L > 64: lane l holds elements m = l TPL + t (consecutive), so the prefix sum is a serial chain in the
//   lane plus ONE wave scan, and the elements walk downwards from the lane's inclusive prefix (f[m-1] = f[m] + conj(k) bo).
//   Every element runs the lattice code (selects for m >= L).  A row form with L / 64 lattice rows needs one wave scan per
//   row: at L = D = 1034 it stepped in 4.09 us against 2.04 for this form (MI355X, tools/gal_bench.py).
// Both then do ONE reduction of h^H b and b^H b (v_permlane32_swap folds, interleaved DPP row sums) and the h update.
// ref / srv come in 64 samples at a time, one per lane (the next block is loaded while this one runs), and a step reads its
// sample with v_readlane; the errors collect in one register (lane j keeps step j's) and leave as one coalesced store: no LDS,
// no barrier anywhere.  Placement is the NLMS lesson (nlms.hip header): workgroups of 4 / 8 / 12 independent wavefronts
// that ask for more than half of the CU's LDS, so each CU gets exactly one workgroup and each SIMD 1 / 2 / 3 wavefronts.
//
// VALU instructions per step (the step loop of the -save-temps listing, classified as tools/isa_stats.py does; no scratch in
// any instantiation):
//   row form:     ~23 per delay-line row + ~128 for the lattice row, the reduction and the scalar tail -- TPL 1: 151, 4: 220,
//                 8: 314, 17: 519, 32: 866; up to TPL 24 three wavefronts fit a SIMD.
//   lattice form: ~64 per element + ~87 -- TPL 4: 343, 8: 592, 17: 1161, 32: 2503; from TPL 17 one wavefront per SIMD.
// A lone wavefront issues one wave64 FP32 instruction per 4 cycles (1.67 ns at 2.4 GHz), so the step time of one stream is
// the instruction count; the per-element work is scalar FP32 (the compiler forms no packed FMAs here).  Measured times:
// DESIGN.md, profiles/gal_bench.json.
//
// Above D = 2048 (32 elements per lane) gal_generic_kernel runs: one workgroup of 256 threads per stream, thread t owning a
// contiguous run of elements, its state in a caller-provided device workspace (prc_gal_workspace_bytes), two workgroup
// barriers per step (block scan, block reduction).  A fallback that takes any D, not a fast path.
#include "common.h"
#include "wave.h"

struct GalArgs {
    const float2* ref;
    const float2* srv;
    float2* out;
    float2* k_out;          // [nstreams][D] or nullptr
    float2* h_out;          // [nstreams][D] or nullptr
    int64_t n, stride, out_stride;
    int32_t L, D, peek, nstreams;
    float mu1, mu2;
};

// inclusive scan over the 64 lanes: Hillis-Steele inside each 16-lane row (row_shr 1, 2, 4, 8; lanes without a source add
// 0), then row_bcast:15 adds row 0's total into row 1 and row 2's into row 3, row_bcast:31 adds rows 0-1 into rows 2-3
__device__ __forceinline__ void gal_wave_scan2(float& a, float& b) {
    a += dpp_add_src<0x111, 0xF>(a); b += dpp_add_src<0x111, 0xF>(b);
    a += dpp_add_src<0x112, 0xF>(a); b += dpp_add_src<0x112, 0xF>(b);
    a += dpp_add_src<0x114, 0xF>(a); b += dpp_add_src<0x114, 0xF>(b);
    a += dpp_add_src<0x118, 0xF>(a); b += dpp_add_src<0x118, 0xF>(b);
    a += dpp_add_src<0x142, 0xA>(a); b += dpp_add_src<0x142, 0xA>(b);
    a += dpp_add_src<0x143, 0xC>(a); b += dpp_add_src<0x143, 0xC>(b);
}

// mu1 <- min(0.999 mu1 + 1e-8 e^2, 5e-3), complex64 arithmetic; NumPy orders complex numbers lexicographically, so the cap
// applies when Re > 5e-3, or Re == 5e-3 and Im > 0 (clutter_removal.py:359)
__device__ __forceinline__ void gal_mu1_update(float& mr, float& mi, float er, float ei) {
    const float e2r = er * er - ei * ei, e2i = er * ei + ei * er;
    const float nr = 0.999f * mr + 1e-8f * e2r, ni = 0.999f * mi + 1e-8f * e2i;
    const bool cap = nr > 5e-3f || (nr == 5e-3f && ni > 0.f);
    mr = cap ? 5e-3f : nr;
    mi = cap ? 0.f : ni;
}

// one element m: bp = bo[m-1], fm = f[m] on entry and f[m-1] on return; writes the new b, P and k.  lat: 1 <= m < L (k and P
// change only there: the step size is 0 elsewhere), first: m == 0 (b = x), valid: m < D (padding keeps b = 0)
__device__ __forceinline__ void gal_element(v2f& b, v2f& k, float& P, v2f bp, v2f& fm, float x_r, float x_i, bool lat,
                                            bool first, bool valid, float mr, float mi) {
    // c = conj(k) bp
    const v2f c = {k.x * bp.x + k.y * bp.y, k.x * bp.y - k.y * bp.x};
    const v2f f1 = fm + c;                                               // f[m-1]
    // lattice: b = bp - k f[m-1]
    const v2f bl = {bp.x - (k.x * f1.x - k.y * f1.y), bp.y - (k.x * f1.y + k.y * f1.x)};
    v2f nb = lat ? bl : bp;
    nb = first ? v2f{x_r, x_i} : nb;
    nb = valid ? nb : v2f{0.f, 0.f};
    // P[m-1] = 0.9 P + 0.19 (|f[m-1]|^2 + |bo[m-1]|^2)
    const float E = f1.x * f1.x + f1.y * f1.y + (bp.x * bp.x + bp.y * bp.y);
    P = 0.9f * P + 0.19f * E;
    // grad = conj(f[m-1]) b[m] + bo[m-1] conj(f[m]);  k += mu1 grad / (P + 1e-10)
    const v2f g = {f1.x * nb.x + f1.y * nb.y + (bp.x * fm.x + bp.y * fm.y),
                   f1.x * nb.y - f1.y * nb.x + (bp.y * fm.x - bp.x * fm.y)};
    const float rr = __builtin_amdgcn_rcpf(P + 1e-10f);                  // P >= 1e-8 > 0: always finite, no branch
    const float r = lat ? rr : 0.f;
    const v2f gs = g * r;
    k.x += mr * gs.x - mi * gs.y;
    k.y += mr * gs.y + mi * gs.x;
    b = nb;
    fm = f1;
}

// the row's elements moved up by one: element (t, l) <- (t, l-1), (t, 0) <- (t-1, 63); row 0's lane 0 gets 0
// (t is a constant of the unrolled row loops, so every index below is one)
template <int N>
__device__ __forceinline__ v2f gal_shift_row(const v2f (&b)[N], const int t) {
    float o_r = 0.f, o_i = 0.f;
    if (t > 0) {
        o_r = wave_readlane(b[t > 0 ? t - 1 : 0].x, 63);
        o_i = wave_readlane(b[t > 0 ? t - 1 : 0].y, 63);
    }
    return v2f{wave_shr1(o_r, b[t].x), wave_shr1(o_i, b[t].y)};
}

// The row form, L <= 64: element m = 64 t + lane lives in row t of lane `lane`.  Row 0 holds the whole lattice (k, P); the
// rows above it are delay line and hold only b and h.
template <int TPL, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void gal_row_kernel(GalArgs a) {
    constexpr int LR = 1;                               // lattice rows
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (s >= a.nstreams) return;                        // no barriers: idle wavefronts just leave
    const float2* __restrict__ ref = a.ref + (int64_t)s * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)s * a.stride;
    float2* __restrict__ out = a.out + (int64_t)s * a.out_stride;
    const int L = a.L, D = a.D;
    const int64_t nsteps = a.n - a.peek - 1 > 0 ? a.n - a.peek - 1 : 0;
    for (int64_t i = nsteps + lane; i < a.n; i += 64) out[i] = make_float2(0.f, 0.f);     // :320, outside the loop's range

    v2f b[TPL], h[TPL], k[LR];
    float P[LR];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        b[t] = v2f{0.f, 0.f};
        h[t] = v2f{0.f, 0.f};
    }
#pragma unroll
    for (int t = 0; t < LR; ++t) {
        k[t] = v2f{0.f, 0.f};
        P[t] = 1e-8f;
    }
    float mr = a.mu1, mi = 0.f;
    const float mu2 = a.mu2;

    // the 64 steps of a block: lane j holds x = ref[n0 + j + peek] and d = srv[n0 + j]
    auto load_block = [&](int64_t n0, float2& xv, float2& dv) {
        const bool in = n0 + lane < nsteps;
        xv = in ? ref[n0 + lane + a.peek] : make_float2(0.f, 0.f);
        dv = in ? srv[n0 + lane] : make_float2(0.f, 0.f);
    };
    float2 xv, dv, xn, dn;
    load_block(0, xv, dv);
    for (int64_t n0 = 0; n0 < nsteps; n0 += 64) {
        load_block(n0 + 64, xn, dn);                    // in flight while this block runs
        const int cnt = nsteps - n0 < 64 ? (int)(nsteps - n0) : 64;
        float eor = 0.f, eoi = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float x_r = wave_readlane(xv.x, j), x_i = wave_readlane(xv.y, j);
            const float d_r = wave_readlane(dv.x, j), d_i = wave_readlane(dv.y, j);
            // 1. lattice rows, upwards: bo[m-1], c = conj(k) bo[m-1], the row's inclusive scan plus the rows below -> f[m]
            v2f bpl[LR], fl[LR];
            float car_r = 0.f, car_i = 0.f;
#pragma unroll
            for (int t = 0; t < LR; ++t) {
                {
                    const v2f bp = gal_shift_row(b, t);
                    float cr = k[t].x * bp.x + k[t].y * bp.y, ci = k[t].x * bp.y - k[t].y * bp.x;
                    gal_wave_scan2(cr, ci);
                    fl[t] = v2f{x_r - (car_r + cr), x_i - (car_i + ci)};
                    car_r += wave_readlane(cr, 63);
                    car_i += wave_readlane(ci, 63);
                    bpl[t] = bp;
                }
            }
            // 2. all rows, downwards (a delay row reads the row below before that row is rewritten); the partial sums
            float yr = 0.f, yi = 0.f, bb = 0.f;
#pragma unroll
            for (int t = TPL - 1; t >= 0; --t) {
                const int m = 64 * t + lane;
                if (t < LR) {
                    v2f fm = fl[t < LR ? t : 0];
                    gal_element(b[t], k[t < LR ? t : 0], P[t < LR ? t : 0], bpl[t < LR ? t : 0], fm, x_r, x_i,
                                m >= 1 && m < L, m == 0, m < D, mr, mi);
                } else {
                    // the delay line (m >= L): b[m] = bo[m-1], nothing else
                    const v2f bp = gal_shift_row(b, t);
                    b[t] = m < D ? bp : v2f{0.f, 0.f};
                }
                yr += h[t].x * b[t].x + h[t].y * b[t].y;                  // conj(h) b
                yi += h[t].x * b[t].y - h[t].y * b[t].x;
                bb += b[t].x * b[t].x + b[t].y * b[t].y;
            }
            // 3. one reduction for h^H b and b^H b
            wave_allsum3(yr, yi, bb);
            const float er = d_r - yr, ei = d_i - yi;
            // 4. h += mu2 conj(e) b / (b^H b + 1e-10)
            const float sc = mu2 / (bb + 1e-10f);
            const v2f cs = {er * sc, -ei * sc};
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                h[t].x += cs.x * b[t].x - cs.y * b[t].y;
                h[t].y += cs.x * b[t].y + cs.y * b[t].x;
            }
            eor = lane == j ? er : eor;
            eoi = lane == j ? ei : eoi;
            gal_mu1_update(mr, mi, er, ei);
        }
        if (lane < cnt) out[n0 + lane] = make_float2(eor, eoi);
        xv = xn;
        dv = dn;
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const int m = 64 * t + lane;
        if (m < D) {
            const v2f kv = t < LR ? k[t < LR ? t : 0] : v2f{0.f, 0.f};
            if (a.k_out) a.k_out[(int64_t)s * D + m] = make_float2(kv.x, kv.y);
            if (a.h_out) a.h_out[(int64_t)s * D + m] = make_float2(h[t].x, h[t].y);
        }
    }
}

// ---- long lattices (L > 64): consecutive elements per lane ----------------------------------------------------------
// Lane l holds elements m = l TPL + t.  The shift is a register rename inside the lane plus one DPP move across lanes, and
// the prefix sum is a serial chain in the lane plus ONE wave scan of the lane totals, then the elements walk downwards from
// the lane's inclusive prefix (f[m-1] = f[m] + conj(k[m]) bo[m-1]).  Every element runs the lattice arithmetic; for the
// elements at m >= L the step size is 0 and the new b is a select.  At L = D = 1034 this form steps in 2.04 us where the
// row form above, with 17 lattice rows and so 17 row scans, took 4.09 us (MI355X, tools/gal_bench.py).
template <int TPL, int MAXW>
__global__ __launch_bounds__(64 * MAXW) void gal_lattice_kernel(GalArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (s >= a.nstreams) return;                        // no barriers: idle wavefronts just leave
    const float2* __restrict__ ref = a.ref + (int64_t)s * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)s * a.stride;
    float2* __restrict__ out = a.out + (int64_t)s * a.out_stride;
    const int L = a.L, D = a.D;
    const int64_t nsteps = a.n - a.peek - 1 > 0 ? a.n - a.peek - 1 : 0;
    for (int64_t i = nsteps + lane; i < a.n; i += 64) out[i] = make_float2(0.f, 0.f);     // :320, outside the loop's range

    const int m0 = lane * TPL;
    v2f b[TPL], k[TPL], h[TPL];
    float P[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        b[t] = v2f{0.f, 0.f};
        k[t] = v2f{0.f, 0.f};
        h[t] = v2f{0.f, 0.f};
        P[t] = 1e-8f;
    }
    float mr = a.mu1, mi = 0.f;
    const float mu2 = a.mu2;

    // the 64 steps of a block: lane j holds x = ref[n0 + j + peek] and d = srv[n0 + j]
    auto load_block = [&](int64_t n0, float2& xv, float2& dv) {
        const bool in = n0 + lane < nsteps;
        xv = in ? ref[n0 + lane + a.peek] : make_float2(0.f, 0.f);
        dv = in ? srv[n0 + lane] : make_float2(0.f, 0.f);
    };
    float2 xv, dv, xn, dn;
    load_block(0, xv, dv);
    for (int64_t n0 = 0; n0 < nsteps; n0 += 64) {
        load_block(n0 + 64, xn, dn);                    // in flight while this block runs
        const int cnt = nsteps - n0 < 64 ? (int)(nsteps - n0) : 64;
        float eor = 0.f, eoi = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float x_r = wave_readlane(xv.x, j), x_i = wave_readlane(xv.y, j);
            const float d_r = wave_readlane(dv.x, j), d_i = wave_readlane(dv.y, j);
            // 1. the lane's total of c_t = conj(k_t) bo[m-1]
            const v2f bp0 = {wave_shr1(0.f, b[TPL - 1].x), wave_shr1(0.f, b[TPL - 1].y)};    // bo of the previous lane's last element
            float cr = 0.f, ci = 0.f;
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                const v2f bp = t ? b[t - 1] : bp0;
                cr += k[t].x * bp.x + k[t].y * bp.y;
                ci += k[t].x * bp.y - k[t].y * bp.x;
            }
            // 2. inclusive prefix over the wavefront: f at the lane's last element
            gal_wave_scan2(cr, ci);
            v2f fm = {x_r - cr, x_i - ci};
            // 3. the elements from the top down (b[t-1] is still the old value when element t reads it)
            float yr = 0.f, yi = 0.f, bb = 0.f;
#pragma unroll
            for (int t = TPL - 1; t >= 0; --t) {
                const int m = m0 + t;
                const v2f bp = t ? b[t - 1] : bp0;
                gal_element(b[t], k[t], P[t], bp, fm, x_r, x_i, m >= 1 && m < L, m == 0, m < D, mr, mi);
                yr += h[t].x * b[t].x + h[t].y * b[t].y;                  // conj(h) b
                yi += h[t].x * b[t].y - h[t].y * b[t].x;
                bb += b[t].x * b[t].x + b[t].y * b[t].y;
            }
            // 4. one reduction for h^H b and b^H b
            wave_allsum3(yr, yi, bb);
            const float er = d_r - yr, ei = d_i - yi;
            // 5. h += mu2 conj(e) b / (b^H b + 1e-10)
            const float sc = mu2 / (bb + 1e-10f);
            const v2f cs = {er * sc, -ei * sc};
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                h[t].x += cs.x * b[t].x - cs.y * b[t].y;
                h[t].y += cs.x * b[t].y + cs.y * b[t].x;
            }
            eor = lane == j ? er : eor;
            eoi = lane == j ? ei : eoi;
            gal_mu1_update(mr, mi, er, ei);
        }
        if (lane < cnt) out[n0 + lane] = make_float2(eor, eoi);
        xv = xn;
        dv = dn;
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const int m = m0 + t;
        if (m < D) {
            if (a.k_out) a.k_out[(int64_t)s * D + m] = make_float2(k[t].x, k[t].y);
            if (a.h_out) a.h_out[(int64_t)s * D + m] = make_float2(h[t].x, h[t].y);
        }
    }
}

// ---- any delay length: state in the caller's workspace -----------------------------------------------------------------
// Per stream: b (two buffers: this step's bo and the new b), k, h (complex64) and P (float32), D each.  Thread t owns the
// contiguous elements [t per, (t+1) per), per = ceil(D / 256).  The scan slot is written before the first barrier of a step
// and read between the two; the reduction slot before the second and read before the next step's first: one slot of each
// suffices.  The new b goes to the other buffer, read (element m-1 by the neighbour) only after the step's second barrier.
#define GALG_THREADS 256
#define GALG_WAVES (GALG_THREADS / 64)
// per stream, rounded to 16 bytes so that every stream's arrays stay aligned
__host__ __device__ __forceinline__ size_t gal_ws_stream_bytes(int D) {
    return ((size_t)D * (4 * sizeof(float2) + sizeof(float)) + 15) / 16 * 16;
}

__global__ __launch_bounds__(GALG_THREADS) void gal_generic_kernel(GalArgs a, unsigned char* __restrict__ ws) {
    __shared__ float2 scan_slot[GALG_WAVES];
    __shared__ float red_slot[3][GALG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const float2* __restrict__ ref = a.ref + (int64_t)s * a.stride;
    const float2* __restrict__ srv = a.srv + (int64_t)s * a.stride;
    float2* __restrict__ out = a.out + (int64_t)s * a.out_stride;
    const int L = a.L, D = a.D;
    float2* bbuf0 = reinterpret_cast<float2*>(ws + (size_t)s * gal_ws_stream_bytes(D));
    float2* bbuf1 = bbuf0 + D;
    float2* kk = bbuf1 + D;
    float2* hh = kk + D;
    float* PP = reinterpret_cast<float*>(hh + D);
    const int per = (D + GALG_THREADS - 1) / GALG_THREADS;
    const int lo = tid * per < D ? tid * per : D, hi = (tid + 1) * per < D ? (tid + 1) * per : D;
    const int64_t nsteps = a.n - a.peek - 1 > 0 ? a.n - a.peek - 1 : 0;
    for (int64_t i = nsteps + tid; i < a.n; i += GALG_THREADS) out[i] = make_float2(0.f, 0.f);
    for (int m = lo; m < hi; ++m) {
        bbuf0[m] = make_float2(0.f, 0.f);
        kk[m] = make_float2(0.f, 0.f);
        hh[m] = make_float2(0.f, 0.f);
        PP[m] = 1e-8f;
    }
    __syncthreads();
    float mr = a.mu1, mi = 0.f;
    for (int64_t n = 0; n < nsteps; ++n) {
        const float2* bo = (n & 1) ? bbuf1 : bbuf0;
        float2* bn = (n & 1) ? bbuf0 : bbuf1;
        const float2 x = ref[n + a.peek], d = srv[n];
        float cr = 0.f, ci = 0.f;
        for (int m = lo; m < hi; ++m) {
            const float2 bp = m ? bo[m - 1] : make_float2(0.f, 0.f), kv = kk[m];
            cr += kv.x * bp.x + kv.y * bp.y;
            ci += kv.x * bp.y - kv.y * bp.x;
        }
        // block-wide inclusive scan of the threads' totals
        float wr = cr, wi = ci;
        gal_wave_scan2(wr, wi);
        if (lane == 63) scan_slot[wave] = make_float2(wr, wi);
        __syncthreads();
        for (int q = 0; q < wave; ++q) { wr += scan_slot[q].x; wi += scan_slot[q].y; }
        v2f fm = {x.x - wr, x.y - wi};
        float yr = 0.f, yi = 0.f, bb = 0.f;
        for (int m = hi - 1; m >= lo; --m) {
            const float2 bpf = m ? bo[m - 1] : make_float2(0.f, 0.f), kf = kk[m];
            v2f b = {0.f, 0.f}, k = {kf.x, kf.y};
            float P = PP[m];
            gal_element(b, k, P, v2f{bpf.x, bpf.y}, fm, x.x, x.y, m >= 1 && m < L, m == 0, true, mr, mi);
            bn[m] = make_float2(b.x, b.y);
            kk[m] = make_float2(k.x, k.y);
            PP[m] = P;
            const float2 hv = hh[m];
            yr += hv.x * b.x + hv.y * b.y;
            yi += hv.x * b.y - hv.y * b.x;
            bb += b.x * b.x + b.y * b.y;
        }
        wave_allsum3(yr, yi, bb);
        if (lane == 0) {
            red_slot[0][wave] = yr;
            red_slot[1][wave] = yi;
            red_slot[2][wave] = bb;
        }
        __syncthreads();
        float sr = 0.f, si = 0.f, sb = 0.f;
#pragma unroll
        for (int q = 0; q < GALG_WAVES; ++q) {          // the same order in every thread: one error sample for all
            sr += red_slot[0][q];
            si += red_slot[1][q];
            sb += red_slot[2][q];
        }
        const float er = d.x - sr, ei = d.y - si;
        const float sc = a.mu2 / (sb + 1e-10f);
        const float csr = er * sc, csi = -ei * sc;
        for (int m = lo; m < hi; ++m) {
            const float2 b = bn[m];
            float2 hv = hh[m];
            hv.x += csr * b.x - csi * b.y;
            hv.y += csr * b.y + csi * b.x;
            hh[m] = hv;
        }
        if (tid == 0) out[n] = make_float2(er, ei);
        gal_mu1_update(mr, mi, er, ei);
    }
    for (int m = lo; m < hi; ++m) {
        if (a.k_out) a.k_out[(int64_t)s * D + m] = kk[m];
        if (a.h_out) a.h_out[(int64_t)s * D + m] = hh[m];
    }
}

#define GAL_FAST_MAX 2048

// wavefronts per workgroup the register footprint allows (3 / 2 / 1 per SIMD: <= 168 / 256 / 512 registers), from the
// -Rpass-analysis=kernel-resource-usage figures of each instantiation
__host__ __device__ constexpr int gal_row_max_waves(int tpl) { return tpl <= 24 ? 12 : 8; }
__host__ __device__ constexpr int gal_lattice_max_waves(int tpl) { return tpl <= 10 ? 12 : (tpl <= 14 ? 8 : 4); }

extern "C" int prc_gal_workspace_bytes(int32_t delay_len, int32_t nstreams, size_t* bytes) {
    PRC_REQUIRE(bytes, PRC_EINVAL, "prc_gal_workspace_bytes: null argument");
    PRC_REQUIRE(delay_len > 0 && nstreams > 0, PRC_EINVAL, "prc_gal_workspace_bytes: non-positive size");
    *bytes = delay_len <= GAL_FAST_MAX ? 0 : (size_t)nstreams * gal_ws_stream_bytes(delay_len);
    return PRC_OK;
}

extern "C" int prc_gal_execute(const void* ref, const void* srv, int64_t n, int64_t stride, int32_t lattice_len,
                               int32_t delay_len, int32_t peek, float mu1, float mu2, void* out, int64_t out_stride,
                               void* k_out, void* h_out, int32_t nstreams, void* workspace, void* stream) {
    PRC_RANGE("prc_gal_execute");
    PRC_REQUIRE(ref && srv && out, PRC_EINVAL, "prc_gal_execute: null argument");
    PRC_REQUIRE(n > 0 && delay_len > 0 && lattice_len > 0 && peek >= 0 && nstreams > 0, PRC_EINVAL,
                "prc_gal_execute: non-positive size (n %lld, lattice %d, delay %d, peek %d, streams %d)", (long long)n,
                lattice_len, delay_len, peek, nstreams);
    PRC_REQUIRE(lattice_len <= delay_len, PRC_ESHAPE, "prc_gal_execute: lattice length %d exceeds delay-line length %d",
                lattice_len, delay_len);
    PRC_REQUIRE(stride >= n && out_stride >= n, PRC_ESHAPE, "prc_gal_execute: stride shorter than n");
    GalArgs a;
    a.ref = (const float2*)ref;
    a.srv = (const float2*)srv;
    a.out = (float2*)out;
    a.k_out = (float2*)k_out;
    a.h_out = (float2*)h_out;
    a.n = n;
    a.stride = stride;
    a.out_stride = out_stride;
    a.L = lattice_len;
    a.D = delay_len;
    a.peek = peek;
    a.nstreams = nstreams;
    a.mu1 = mu1;
    a.mu2 = mu2;
    if (delay_len > GAL_FAST_MAX) {
        PRC_REQUIRE(workspace, PRC_EINVAL, "prc_gal_execute: delay length %d needs a workspace of prc_gal_workspace_bytes",
                    delay_len);
        hipLaunchKernelGGL(gal_generic_kernel, dim3(nstreams), dim3(GALG_THREADS), 0, (hipStream_t)stream, a,
                           (unsigned char*)workspace);
        PRC_LAUNCH_CHECK();
        return PRC_OK;
    }
    // rows (elements per lane), rounded up to an instantiated count: every element beyond D is masked
    const int need = (delay_len + 63) / 64;
    static const int tpls[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 28, 32};
    int tpl = 32;
    for (const int t : tpls) if (t >= need) { tpl = t; break; }
    const bool rows = lattice_len <= 64;                // the row form: one lattice row, delay-line rows with b and h only
    const int maxw = rows ? gal_row_max_waves(tpl) : gal_lattice_max_waves(tpl);
    // wavefronts per workgroup = per CU: the NLMS cost model (1 / 2 / 3 wavefronts per SIMD step at 1.0 / 1.68 / 2.44)
    int nw = 4;
    double best = 1e30;
    for (int w = 4; w <= maxw; w += 4) {
        const double rounds = (double)ceil_div64(ceil_div64(nstreams, w), 256);
        const double cost = rounds * (w == 4 ? 1.0 : (w == 8 ? 1.68 : 2.44));
        if (cost < best) { best = cost; nw = w; }
    }
    const size_t lds = 84 * 1024;                      // unused; more than half a CU's LDS: one workgroup per CU
    const int grid = (int)ceil_div64(nstreams, nw);
#define PRC_GAL_LAUNCH(KERNEL)                                                                  \
    {                                                                                           \
        { int rc_ = prc_lds_optin(reinterpret_cast<const void*>(&KERNEL), (int)lds); if (rc_) return rc_; } \
        hipLaunchKernelGGL((KERNEL), dim3(grid), dim3(64 * nw), lds, (hipStream_t)stream, a);   \
        PRC_LAUNCH_CHECK();                                                                     \
        return PRC_OK;                                                                          \
    }
#define PRC_GAL_CASE(G)                                                                         \
    case G:                                                                                     \
        if (rows) PRC_GAL_LAUNCH((gal_row_kernel<G, gal_row_max_waves(G)>))                 \
        else PRC_GAL_LAUNCH((gal_lattice_kernel<G, gal_lattice_max_waves(G)>))
    switch (tpl) {
        PRC_GAL_CASE(1) PRC_GAL_CASE(2) PRC_GAL_CASE(3) PRC_GAL_CASE(4) PRC_GAL_CASE(5) PRC_GAL_CASE(6)
        PRC_GAL_CASE(7) PRC_GAL_CASE(8) PRC_GAL_CASE(10) PRC_GAL_CASE(12) PRC_GAL_CASE(14) PRC_GAL_CASE(17)
        PRC_GAL_CASE(20) PRC_GAL_CASE(24) PRC_GAL_CASE(28) PRC_GAL_CASE(32)
        default: break;
    }
#undef PRC_GAL_LAUNCH
#undef PRC_GAL_LAUNCH
#undef PRC_GAL_CASE
    return PRC_EUNSUPPORTED;
}
