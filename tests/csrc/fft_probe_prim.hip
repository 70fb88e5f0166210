// TEST ONLY: the packed-f32 primitives of passiveradar_amd/csrc/fft_pk.h next to the scalar forms they stand for, on the
// same registers: the test compares the two outputs bit for bit.  Built WITHOUT -DFT_PK, so that cmac_conj_a, cscale and
// ltc_cmac_bconj are the scalar forms; the packed ones are called by their pk_ names.
#include "../../passiveradar_amd/csrc/ls_team_cached.h"
#include "../../passiveradar_amd/csrc/fft_pk.h"
#ifdef FT_PK
#error "the primitive probe compares scalar with packed forms: build it without FT_PK"
#endif

enum {
    P_DFT16_F16 = 0, P_DFT16_F12, P_DFT16_F8, P_DFT16_I16, P_DFT16_I12, P_DFT16_I8,   // dft16<+-1, NZ> / pk_dft16
    P_MULTW_F_V, P_MULTW_I_V,     // mul_tw<+-1> / pk_mul_tw, twiddle in a VGPR pair (one per register, from tw[])
    P_MULTW_F_S, P_MULTW_I_S,     // the same with the twiddle in an SGPR pair (the kernel argument w)
    P_TWIDDLE_F, P_TWIDDLE_I,     // mul_tw over registers 1..15 / pk_twiddle<+-1, 1> (multiply halves first, four at a time)
    P_CMAC_CONJ_A,                // cmac_conj_a / pk_cmac_conj_a, accumulated over the 16 registers
    P_CMULC_V, P_CMULC_S,         // cmul (common.h) / pk_cmulc, pk_cmulc_s
    P_CMAC_BCONJ,                 // ltc_cmac_bconj / pk_cmac_bconj
    P_CSCALE,                     // cscale / pk_scale (scale: w.x)
    P_COUNT
};

template <int DIR, int NZ>
__device__ __forceinline__ void both_dft16(float2 (&x)[16], v2f (&p)[16]) {
#pragma unroll
    for (int r = NZ; r < 16; ++r) { x[r] = make_float2(0.f, 0.f); p[r] = v2f{0.f, 0.f}; }
    dft16<DIR, NZ>(x);
    pk_dft16<DIR, NZ>(p);
}

// in, tw: nthreads x 16 float2 (thread-major); out_s / out_p: the scalar and the packed result, same shape
template <int WHICH>
__global__ __launch_bounds__(256) void prim_kernel(const float2* in, const float2* tw, float2* out_s, float2* out_p, float2 w,
                                                   int nthreads) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nthreads) return;
    float2 x[16], c[16];
    v2f p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { x[r] = in[16 * t + r]; c[r] = tw[16 * t + r]; p[r] = pk_from(x[r]); }
    if (WHICH == P_DFT16_F16) both_dft16<1, 16>(x, p);
    else if (WHICH == P_DFT16_F12) both_dft16<1, 12>(x, p);
    else if (WHICH == P_DFT16_F8) both_dft16<1, 8>(x, p);
    else if (WHICH == P_DFT16_I16) both_dft16<-1, 16>(x, p);
    else if (WHICH == P_DFT16_I12) both_dft16<-1, 12>(x, p);
    else if (WHICH == P_DFT16_I8) both_dft16<-1, 8>(x, p);
    else if (WHICH == P_MULTW_F_V || WHICH == P_MULTW_I_V) {
        constexpr int DIR = WHICH == P_MULTW_F_V ? 1 : -1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { x[r] = mul_tw<DIR>(x[r], c[r]); p[r] = pk_mul_tw<DIR>(p[r], pk_from(c[r])); }
    } else if (WHICH == P_MULTW_F_S || WHICH == P_MULTW_I_S) {
        constexpr int DIR = WHICH == P_MULTW_F_S ? 1 : -1;
        const v2f ws = pk_from(w);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            x[r] = mul_tw<DIR>(x[r], w);
            p[r] = pk_cmul_q_s<(DIR < 0)>(p[r], ws, pk_cmul_p_s(p[r], ws));
        }
    } else if (WHICH == P_TWIDDLE_F || WHICH == P_TWIDDLE_I) {
        constexpr int DIR = WHICH == P_TWIDDLE_F ? 1 : -1;
#pragma unroll
        for (int r = 1; r < 16; ++r) x[r] = mul_tw<DIR>(x[r], c[r]);
        pk_twiddle<DIR, 1>(p, [&](int k) { return pk_from(c[k]); });
    } else if (WHICH == P_CMAC_CONJ_A) {
        float2 a = x[0];
        v2f b = p[0];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cmac_conj_a(a, x[r], c[r]);
            pk_cmac_conj_a(b, p[r], pk_from(c[r]));
            x[r] = a;
            p[r] = b;
        }
    } else if (WHICH == P_CMULC_V) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = pk_cmulc(p[r], pk_from(c[r])); x[r] = cmul(x[r], c[r]); }
    } else if (WHICH == P_CMULC_S) {
        const v2f ws = pk_from(w);
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = pk_cmulc_s(p[r], ws); x[r] = cmul(x[r], w); }
    } else if (WHICH == P_CMAC_BCONJ) {
        float2 a = x[0];
        v2f b = p[0];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            ltc_cmac_bconj(a, x[r], c[r]);
            pk_cmac_bconj(b, p[r], pk_from(c[r]));
            x[r] = a;
            p[r] = b;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { x[r] = cscale(x[r], w.x); p[r] = pk_scale(p[r], w.x); }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { out_s[16 * t + r] = x[r]; out_p[16 * t + r] = pk_to(p[r]); }
}

template <int WHICH>
static int launch(const float2* din, const float2* dtw, float2* ds, float2* dp, float2 w, int nthreads) {
    hipLaunchKernelGGL(prim_kernel<WHICH>, dim3((nthreads + 255) / 256), dim3(256), 0, 0, din, dtw, ds, dp, w, nthreads);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// in, tw, out_scalar, out_packed: nthreads x 16 complex64 on the host; (wx, wy): the uniform operand
extern "C" int fft_probe_prim(const void* in_host, const void* tw_host, void* out_scalar, void* out_packed, int nthreads,
                              float wx, float wy, int which) {
    if (nthreads <= 0 || which < 0 || which >= P_COUNT) return -5;
    float2* d[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes = sizeof(float2) * 16 * (size_t)nthreads;
    int rc = 0;
    for (int i = 0; i < 4; ++i)
        if (hipMalloc(&d[i], bytes) != hipSuccess) rc = -1;
    if (rc == 0 && (hipMemcpy(d[0], in_host, bytes, hipMemcpyHostToDevice) || hipMemcpy(d[1], tw_host, bytes, hipMemcpyHostToDevice)))
        rc = -1;
    const float2 w = make_float2(wx, wy);
    if (rc == 0) {
        switch (which) {
#define PROBE_CASE(M) case M: rc = launch<M>(d[0], d[1], d[2], d[3], w, nthreads); break;
            PROBE_CASE(0) PROBE_CASE(1) PROBE_CASE(2) PROBE_CASE(3) PROBE_CASE(4) PROBE_CASE(5) PROBE_CASE(6) PROBE_CASE(7)
            PROBE_CASE(8) PROBE_CASE(9) PROBE_CASE(10) PROBE_CASE(11) PROBE_CASE(12) PROBE_CASE(13) PROBE_CASE(14)
            PROBE_CASE(15) PROBE_CASE(16)
#undef PROBE_CASE
        }
    }
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = -3;
    if (rc == 0 && (hipMemcpy(out_scalar, d[2], bytes, hipMemcpyDeviceToHost) || hipMemcpy(out_packed, d[3], bytes, hipMemcpyDeviceToHost)))
        rc = -3;
    for (int i = 0; i < 4; ++i) hipFree(d[i]);
    return rc;
}
