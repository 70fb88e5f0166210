// Shared by the 4096-point CAF segment kernels (caf_fft_team.hip, caf_fft_team8.hip, caf_fft_team_multi.hip): the argument
// block, the workgroup -> work mapping and the pieces of a segment pass that do not depend on the team.  The device pieces
// are templated on NR, the registers per thread of a 4096-point array (16 for the four-wavefront team of fft_team.h, 8 for
// the eight-wavefront team of fft_team8.h): thread t, register r holds sample / lag (FT_P / NR) r + t.
#pragma once
#include "caf_internal.h"
#include "fft_team.h"
#include <type_traits>

struct CafTeamArgs {
    CafSegArgs s;
    const float2* gtab;
    int32_t piece;      // B = 4097 - lagblk samples of ref per transform
    int32_t lagblk;     // lags per block (<= 3073)
    int32_t nlagblk;    // lag blocks covering 0..range_bins
    int32_t segs;       // consecutive slow-time samples per workgroup
    // several reference channels in ONE launch (nothing shared between them but the L2 -- "turns" without the tail of four
    // small launches): channel z reads refs[z] and writes its surfaces y_ref_stride elements further on
    const float2* refs[PRC_CAF_MAX_REFS];
    int64_t y_ref_stride;
    int32_t nref, chunks_x, nchunks;   // channels; workgroup chunks per frame; chunks_x * nframes
    int32_t xcd_contig;                // 1: an XCD takes a contiguous run of chunks; 0: chunks go round the XCDs in launch order
    int32_t pair_half;                 // > 0: frames overlap by half (= this many chunks): the two frames that cover the same
                                       // samples run in consecutive slots of one XCD (PRC_OPT_CAF_PAIR_FRAMES)
    int32_t nframes;
};

// the same segment kernel on the eight-wavefront transform of fft_team8.h (caf_fft_team8.hip); `a` as prepared by
// caf_launch_fft_team_refs
int caf_launch_fft_team8(const CafTeamArgs& a, dim3 grid, bool has_window, hipStream_t stream);

#define CAFT_TAIL_MAX 16      // a last piece of at most this many samples is added directly after the inverse transform

// pieces (transforms of the reference) per segment of q1 samples when a lag block is lb lags wide: pieces of 4097 - lb
// samples, a remainder of at most CAFT_TAIL_MAX goes the direct way
static inline int64_t caft_pieces(int64_t q1, int lb) {
    const int64_t Bp = FT_P + 1 - lb;
    const int64_t pieces = q1 / Bp;
    return q1 % Bp > CAFT_TAIL_MAX || pieces == 0 ? pieces + 1 : pieces;
}

template <int N> using caft_int = std::integral_constant<int, N>;

// Workgroup -> (channel ch, frame b, chunk of segments bx); false: this workgroup has no work (uniform, before any barrier).
// Workgroups reach the eight XCDs round-robin in launch order and every XCD has its own L2: workgroup
// L (XCD L & 7, slot L >> 3 there) takes channel (L >> 3) % nref of chunk 8 ((L >> 3) / nref) + (L & 7).  The channels of
// a multi-illuminator frame read the SAME surveillance windows and sit in consecutive slots of ONE XCD: one of them
// fetches a window from HBM, the others find it in that XCD's L2 (config 5, four channels: 219 -> 96 MB fetched per
// surface, 301 -> 281 us per frame).  Chunks themselves keep going round the XCDs: giving every XCD a contiguous run of
// segments instead (PRC_OPT_CAF_XCD_CONTIG = 1; neighbouring segments share half a window) measured 3-6 % SLOWER at
// one channel and at four, configs 3 and 5 alike (profiles/r04_ab_log.md, call 12) -- eight distant streams instead of
// one; it is the option's off position that ships.
__device__ __forceinline__ bool caft_work(const CafTeamArgs& a, int* ch, int* b, int* bx) {
    const int per_xcd = (a.nchunks + 7) >> 3;
    const int slot = (int)(blockIdx.x >> 3);
    const int ci = slot / a.nref;
    *ch = slot % a.nref;
    if (a.pair_half > 0) {
        // 50 %-overlapped frames: position A of the stream (in chunks of half a frame) is covered by frame A / half (its
        // first half) and by the frame before (its second half) -- the two take consecutive slots, like the channels, and
        // share the reference and surveillance samples through the L2 (config 5, 16 frames: 285 -> 276 us per four-
        // illuminator frame, 74 -> 72.4 us per surface at one channel; config 3: no difference)
        const int k = ci & 1, A = (ci >> 1) * 8 + (int)(blockIdx.x & 7u);
        if (A >= (a.nframes + 1) * a.pair_half) return false;
        *b = A / a.pair_half - k;
        *bx = A % a.pair_half + k * a.pair_half;
        return *b >= 0 && *b < a.nframes && *bx < a.chunks_x;
    }
    const int chunk = a.xcd_contig ? (int)(blockIdx.x & 7u) * per_xcd + ci : ci * 8 + (int)(blockIdx.x & 7u);
    if (ci >= per_xcd || chunk >= a.nchunks) return false;
    *b = chunk / a.chunks_x;
    *bx = chunk - *b * a.chunks_x;
    return true;
}

// Samples [lo, hi_f] of slow-time sample j's segment go through the transforms in pieces of B; a short remainder after the
// last full piece, `tail` samples from hi_f + 1, goes the direct way (caft_tail).  Frame-relative 32-bit results (n < 2^31).
struct CaftSeg {
    int lo, hi_f, tail;
};
__device__ __forceinline__ CaftSeg caft_segment(const CafSegArgs& s, int64_t j, int N, int B) {
    const int64_t n_hi64 = j * s.q + s.half;
    const int64_t n_lo64 = n_hi64 - (s.ntaps - 1);
    const int lo = n_lo64 < 0 ? 0 : (int)n_lo64;
    const int hi = n_hi64 > N - 1 ? N - 1 : (int)n_hi64;
    const int len = hi - lo + 1;
    int tail = len % B;
    if (tail > CAFT_TAIL_MAX || len < B) tail = 0;
    return {lo, hi - tail, tail};
}

// Surveillance slots [0, want) of a piece and lag block into the time layout: frame offsets start .. with circular wrap
// (range_doppler_processing.py:82).  Raw buffer loads as in caf_fft.hip: the descriptor's num_records encodes "samples that
// exist" (end of the frame, n_valid < n), slots beyond them read as zero.  vo8 = 8 t.
template <int NR>
__device__ __forceinline__ void caft_load_srv(float2 (&v)[NR], const float2* __restrict__ srv, int start, int want, int N,
                                              int NV, unsigned vo8) {
    constexpr unsigned STEP = 8u * (FT_P / NR);                 // bytes between a thread's registers
    if (start >= N) start -= N;
    int c1 = want;
    if (N - start < c1) c1 = N - start;
    if (NV - start < c1) c1 = NV - start;
    const __amdgpu_buffer_rsrc_t rv = prc_rsrc(srv + start, prc_clampu(c1) * 8u);
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = prc_buf_load_c64(rv, vo8, STEP * r);
    const int over = start + want - N;                          // slots that wrapped (uniform, rare)
    if (over > 0) {
        const __amdgpu_buffer_rsrc_t rw2 = prc_rsrc(srv, prc_clampu(over < NV ? over : NV) * 8u);
        const unsigned voff = vo8 - (unsigned)(N - start) * 8u; // threads before the wrap: out of range
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float2 w2 = prc_buf_load_c64(rw2, voff + STEP * r, 0u);
            v[r].x += w2.x;
            v[r].y += w2.y;
        }
    }
}

// Direct lag products of the `tail` samples after the last full piece (acc is the unnormalised inverse transform,
// x 4096).  Raw buffer loads over the frame's surveillance samples: an index >= n_valid, a lag outside this block
// or beyond range_bins reads as zero from the hardware range check -- no 64-bit addresses, no selects.
template <bool HAS_WIN, int NR>
__device__ __forceinline__ void caft_tail(float2 (&acc)[NR], const float2* __restrict__ ref,
                                          const float2* __restrict__ srv, const float* __restrict__ win, int hi_f,
                                          int tail, int L0, int LB, int R, int N, int NV, int t) {
    const __amdgpu_buffer_rsrc_t rs = prc_rsrc(srv, (unsigned)NV * 8u);
    for (int i = 0; i < tail; ++i) {
        const int n1 = hi_f + 1 + i;
        float2 uu = make_float2(0.f, 0.f);
        if (n1 < NV) {
            uu = ref[n1];
            if (HAS_WIN) { const float w = win[n1]; uu.x *= w; uu.y *= w; }
        }
        uu.x *= (float)FT_P;
        uu.y *= (float)FT_P;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int within = (FT_P / NR) * r + t;
            const int lag = L0 + within;
            int idx = n1 + lag;
            if (idx >= N) idx -= N;
            const bool ok = within < LB && lag <= R;
            const float2 sv = prc_buf_load_c64(rs, ok ? (unsigned)idx * 8u : 0xFFFFFFF0u, 0u);
            cmac_conj_a(acc[r], uu, sv);
        }
    }
}

// Epilogue of a lag block: lag L0 + within of segment j, frame b goes to column R - lag of the surfaces at y, conjugated
// and normalised (acc is the unnormalised inverse transform of conj(U) V)
template <int NR>
__device__ __forceinline__ void caft_store(const float2 (&acc)[NR], const CafSegArgs& s, float2* __restrict__ y, int b,
                                           int64_t j, int L0, int LB, int R, int t) {
    const float sc = 1.0f / (float)FT_P;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int within = (FT_P / NR) * r + t;
        const int lag = L0 + within;
        if (within < LB && lag <= R) y[caf_y_off(s, b, j, R - lag)] = make_float2(acc[r].x * sc, -acc[r].y * sc);
    }
}
