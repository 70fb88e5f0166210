// Pieces shared by the FFT-domain kernels of the block least-squares canceller (ls_fft.hip on the one-wavefront 1024-point
// transform, ls_fft_team*.hip on the four-wavefront 4096-point transform).  Where the transform matters the helpers are
// templated on W, the threads per transform (64 or 256): thread t, register r holds slot W r + t, a register is 8 W bytes
// of a stream further on and a transform holds 16 W slots.  Loads are raw buffer loads (common.h): the range check of a
// descriptor supplies the zeros, and a slot offset below zero wraps to a huge unsigned one, out of range.
#pragma once
#include "ls_internal.h"
#include <math.h>

// exp(j x): 7th-order Taylor for |x| <= 0.3 (error < 2e-9, the usual case: Doppler bins of a few Hz), sincosf
// beyond (bins of kHz at a few hundred kHz of sample rate; only ever reached in the rarely taken wrap branches)
__device__ __forceinline__ float2 ls_small_rot(float x) {
    if (fabsf(x) > 0.3f) {
        float s, c;
        sincosf(x, &s, &c);
        return make_float2(c, s);
    }
    const float x2 = x * x;
    const float c = 1.f + x2 * (-0.5f + x2 * (1.f / 24.f + x2 * (-1.f / 720.f)));
    const float s = x * (1.f + x2 * (-1.f / 6.f + x2 * (1.f / 120.f + x2 * (-1.f / 5040.f))));
    return make_float2(c, s);
}

struct LsSlot {        // one register slot of the rotated reference, before the data arrived
    bool ok;           // slot carries a sample (else zero)
    bool wr;           // source index wrapped around the block end
    int off;           // clamped source offset into ref
};

// logical r[m] = ref[(m+peek) mod n] * exp(j phi((m+peek) mod n)),  m may lie outside [0, n)
__device__ __forceinline__ LsSlot ls_slot(int m, int n, int peek, bool circular, bool want) {
    LsSlot s;
    s.wr = false;
    bool ok = want;
    if (m >= n) { if (circular) { m -= n; s.wr = true; } else ok = false; }
    if (m < 0) { if (circular) { m += n; s.wr = true; } else ok = false; }
    int off = m + peek;
    if (off >= n) { off -= n; s.wr = true; }
    s.ok = ok;
    s.off = ok ? off : 0;
    return s;
}

__device__ __forceinline__ float2 ls_slot_finish(float2 raw, const LsSlot& s, int rot, float theta32, float2 base,
                                                 float2 step) {
    float2 v = raw;
    if (rot) {
        const float2 cont = cmul(base, step);
        const float2 wrapped = ls_small_rot(theta32 * (float)(s.wr ? s.off : 0));
        v = cmul(v, s.wr ? wrapped : cont);
    }
    return s.ok ? v : make_float2(0.f, 0.f);
}

// Wrapped tail of the peek-rotated reference: the slots from `wstart` on, at most `peek` of them and none from slot `lim`
// on (the transform length, or less where the caller wants nothing beyond the block), take ref[0], ref[1], ... -- the
// source index restarted at the block end (np.roll at clutter_removal.py:139).  Added onto x, whose unwrapped load left
// zeros there; a wave-uniform, rarely taken branch.  PHASE: the samples carry the Doppler rotation, and the restarted
// ramp has its own phase theta32 * index (the unrotated rho of the cached-spectrum chain has none).
template <int W, bool PHASE>
__device__ __forceinline__ void ls_add_wrapped_tail(float2 (&x)[16], const float2* ref, unsigned vo8, int wstart, int peek,
                                                    int lim, int t = 0, int rot = 0, float theta32 = 0.f) {
    if (peek > 0 && wstart < lim) {
        int cw = lim - wstart;
        if (cw > peek) cw = peek;
        const __amdgpu_buffer_rsrc_t rw = prc_rsrc(ref, prc_clampu(cw) * 8u);
        const unsigned voff = vo8 - (unsigned)wstart * 8u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float2 w = prc_buf_load_c64(rw, voff + 8u * W * r, 0u);
            if (PHASE && rot) {
                // index inside [0, peek]: lanes outside the wrapped run carry zeros, keep their phase argument small
                const int k = W * r + t - wstart;
                w = cmul(w, ls_small_rot(theta32 * (float)(k < 0 ? 0 : (k > peek ? peek : k))));
            }
            x[r].x += w.x;
            x[r].y += w.y;
        }
    }
}

// rho piece of the cached-spectrum chain in slots [ext, ext+cnt) (vslot: the lane offset that carries -ext): samples
// n0 .. n0+cnt-1 of rho = roll(ref, -peek), masked by the range check, then the wrapped ones among them.
template <int W>
__device__ __forceinline__ void ls_load_rho_piece(float2 (&up)[16], const float2* ref, int n, int peek, int n0, int cnt,
                                                  unsigned vslot) {
    int cu = cnt;
    if (n - peek - n0 < cu) cu = n - peek - n0;
    const __amdgpu_buffer_rsrc_t ru = prc_rsrc(ref + peek + n0, prc_clampu(cu) * 8u);
#pragma unroll
    for (int r = 0; r < 16; ++r) up[r] = prc_buf_load_c64(ru, vslot + 8u * W * r, 0u);
    const int wst = n - peek - n0;                // first wrapped sample of the piece
    if (peek > 0 && wst < cnt) {
        // a last piece shorter than peek starts inside the wrapped run (wst < 0): the source then
        // starts at ref[-wst], not at ref[0] -- otherwise the slots below `ext` would pick up the
        // wrapped samples that belong to the previous piece and count them twice
        const int w0 = wst > 0 ? wst : 0;
        const __amdgpu_buffer_rsrc_t rw = prc_rsrc(ref + (w0 - wst), prc_clampu(cnt - w0) * 8u);
        const unsigned voff = vslot - (unsigned)w0 * 8u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float2 w = prc_buf_load_c64(rw, voff + 8u * W * r, 0u);
            up[r].x += w.x;
            up[r].y += w.y;
        }
    }
}

// Fused kernels, last `peek` outputs of the block: rho samples whose ramp restarted carry gamma instead of 1 (g1 = gamma - 1);
// y holds the FIR output of the piece at n0 in slots [ext, ext+cnt).
template <int W>
__device__ __forceinline__ void ls_gamma_edge(float2 (&y)[16], const double2* taps, const float2* ref, float2 g1, int n,
                                              int n0, int cnt, int ext, int peek, int T, int t) {
    if (peek > 0 && n0 + cnt > n - peek) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int nn = n0 + W * r + t - ext;
            const int over = nn - (n - peek);            // 0..peek-1 for affected outputs
            if (over >= 0 && nn < n) {
                float2 acc = make_float2(0.f, 0.f);
                for (int k = 0; k <= over && k < T; ++k) {
                    const double2 wk = taps[k];
                    cmac(acc, make_float2((float)wk.x, (float)wk.y), ref[over - k]);   // rho[nn-k] = ref[nn-k+peek-n]
                }
                const float2 c = cmul(g1, acc);
                y[r].x += c.x;
                y[r].y += c.y;
            }
        }
    }
}

// Fused kernels, one rotation on the way out: from this bin's frame to the frame of whoever reads the stream next.
// idx: the stream index + peek of this thread's slot 0.  Returns whether the output is rotated at all.
template <bool ROT_IN>
__device__ __forceinline__ bool ls_out_rotation(const LsFftArgs& a, int64_t idx, float2& obase, float2& ibase) {
    const bool rot_out = a.rot || a.rot2;
    obase = make_float2(1.f, 0.f);
    ibase = make_float2(1.f, 0.f);
    if (rot_out) {
        const float2 p1 = a.rot ? phase_rot(a.pr, idx) : make_float2(1.f, 0.f);
        float2 p2 = a.rot2 ? phase_rot(a.pr2, idx) : make_float2(1.f, 0.f);
        p2.y = -p2.y;
        obase = cmul(p1, p2);
        if (ROT_IN) ibase = make_float2(p1.x, -p1.y);
    }
    return rot_out;
}

// taps (complex128) to float2 registers in slots [0, T), zero padded: the input of the tap transform
template <int W>
__device__ __forceinline__ void ls_load_taps(float2 (&h)[16], const double2* __restrict__ taps, int T, int t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int idx = W * r + t;
        const double2 tp = taps[idx < T ? idx : 0];
        h[r] = idx < T ? make_float2((float)tp.x, (float)tp.y) : make_float2(0.f, 0.f);
    }
}

// part[0/1][lag] of one wave / team holds conj(g) * sc, lags 0 .. T-1 of the inverse transforms wrr (autocorrelation, AUTO
// only) and wrs (cross-correlation): the Levinson / prepare / solve prologues conjugate back
template <int W, bool AUTO>
__device__ __forceinline__ void ls_store_partial(float2* __restrict__ part, const float2 (&wrr)[16], const float2 (&wrs)[16],
                                                 int T, int t, float sc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lag = W * r + t;
        if (lag < T) {
            if (AUTO) part[lag] = make_float2(wrr[r].x * sc, -wrr[r].y * sc);
            part[T + lag] = make_float2(wrs[r].x * sc, -wrs[r].y * sc);
        }
    }
}
