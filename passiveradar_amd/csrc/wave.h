// Wavefront primitives shared by the units that reduce, scan or shift across the 64 lanes of one wavefront: the xor-butterfly
// reductions (LDS crossbar), the DPP moves, and the fused all-lane sums built from them.  Every function is called by whole
// wavefronts.  The addition order of each sum is part of the results the units are tested to, bit for bit
// (tests/test_gpu_order_select.py holds each one to the emulation of its own tree).
#pragma once
#include "common.h"

typedef float v2f __attribute__((ext_vector_type(2)));   // a complex64 in an even VGPR pair: one operand of v_pk_*_f32

// ---- xor butterflies, 32 down to 1: every lane ends with the result ----
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, PRC_WAVE);
    return v;
}
// the sum over the lanes that agree modulo `m` (a power of two below 64): the butterflies 32 down to m
__device__ __forceinline__ double wave_sum_mod(double v, int m) {
    for (int o = 32; o >= m; o >>= 1) v += __shfl_xor(v, o, PRC_WAVE);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, PRC_WAVE));
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, PRC_WAVE);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, PRC_WAVE);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w < v ? w : v;
    }
    return v;
}

// ---- DPP moves (no LDS crossbar).  CTRL: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror,
// 0x140 row_mirror, 0x111 + n row_shr:n, 0x138 wave_shr:1, 0x142 row_bcast:15, 0x143 row_bcast:31 ----
// x moved by CTRL; lanes without a source, or in a row outside ROW_MASK, get 0 (the neutral element of the add that follows)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_src(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, true));
}
// lane l <- lane l-1 of src across the whole wavefront; lane 0 <- `lane0`
__device__ __forceinline__ float wave_shr1(float lane0, float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(src), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_readlane(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// ---- fused all-lane sums ----
// A chain sums two values at once: v_permlane32_swap puts the `lo` partials of the upper half next to the `hi` partials of
// the lower half, one add folds the halves (lanes 0-31: lo(l) + lo(l+32); lanes 32-63: hi), four DPP adds reduce the 16-lane
// rows (xor-1 / xor-2 inside quads, half-row mirror, row mirror: every lane of a row then holds the row sum), and row_bcast:15
// adds row 0 into row 1 and row 2 into row 3 (rows 0 and 2 add zero): lane 31 holds the sum of lo, lane 63 the sum of hi.
// N independent chains go step by step, side by side.
template <int N>
__device__ __forceinline__ void wave_fold_chains(float (&v)[N], const float (&lo)[N], const float (&hi)[N]) {
    decltype(__builtin_amdgcn_permlane32_swap(0, 0, false, false)) sw[N];
#pragma unroll
    for (int c = 0; c < N; ++c) sw[c] = __builtin_amdgcn_permlane32_swap(__float_as_int(lo[c]), __float_as_int(hi[c]), false, false);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = __int_as_float(sw[c][0]) + __int_as_float(sw[c][1]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += dpp_mov<0xB1>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += dpp_mov<0x4E>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += dpp_mov<0x141>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += dpp_mov<0x140>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += dpp_add_src<0x142, 0xA>(v[c]);
}
// both sums of a complex dot product (re, im) in ONE reduction: 9 instructions where two separate all-lane sums took 22
__device__ __forceinline__ void wave_allsum2(float& yr, float& yi) {
    float v[1];
    wave_fold_chains<1>(v, {yr}, {yi});
    yr = wave_readlane(v[0], 31);
    yi = wave_readlane(v[0], 63);
}
// the same with a third, real sum (bb) beside it: a second chain of the same steps with bb in both halves
__device__ __forceinline__ void wave_allsum3(float& yr, float& yi, float& bb) {
    float v[2];
    wave_fold_chains<2>(v, {yr, bb}, {yi, bb});
    yr = wave_readlane(v[0], 31);
    yi = wave_readlane(v[0], 63);
    bb = wave_readlane(v[1], 31);
}
