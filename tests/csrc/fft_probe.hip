// TEST ONLY: exposes the 4096-point team transform of passiveradar_amd/csrc/fft_team.h on its own, so that the
// GPU tests can check it against numpy.fft directly (layouts of tools/fft4096_model.py).  Not part of libprcore, but
// linked against it: the twiddle table is the device copy the library itself uploads (ft_device_tables).
// Built once per shipped set of FT_* defines (Makefile); every build exposes the same entry point and the same modes.
#include "../../passiveradar_amd/csrc/fft_team.h"

// time layout     : thread t, register r <-> element 256 r + t of the block
// frequency layout: thread t, register r <-> element 16 t + r of the block (bin (t >> 4) + 16 (t & 15) + 256 r)
enum {
    M_FWD0 = 0,        // ft4096_fwd<0>: time in, frequency layout out
    M_ROUNDTRIP = 1,   // ft4096_fwd<0>, ft4096_inv<1>: time in, time out (x 4096)
    M_SCHED_ALT = 2,   // (fwd<0>, fwd<1>, cmac_conj_a) x 3, inv<1> -- twice, strictly alternating buffers, no extra barrier
    M_FWD1 = 3,        // ft4096_fwd<1>
    M_FWD0_NZ12 = 4,   // ft4096_fwd<0, 12>: registers 12..15 are zero (as in the kernels: not even read)
    M_FWD0_NZ8 = 5,
    M_FWD1_NZ12 = 6,
    M_FWD1_NZ8 = 7,
    M_INV0 = 8,        // ft4096_inv<0>: frequency layout in, time out (x 4096)
    M_INV1 = 9,
    M_SCHED_CAF = 10,  // caf_fft_team: (fwd<0>, fwd<1>, cmac_conj_a) x 3, inv<0>, ft_team_sync() -- twice
    M_SCHED_LS = 11,   // ls_fft_team_cached: fwd<1> | (fwd<1>, product, inv<0>) x 3 -- twice; fwd<1>, inv<0> alternate
    M_COUNT = 12
};

template <int CUR, int NZ>
__device__ __forceinline__ void fwd_freq_out(float2 (&u)[16], const FtLane& f, float2* ob) {
#pragma unroll
    for (int r = NZ; r < 16; ++r) u[r] = make_float2(0.f, 0.f);
    ft4096_fwd<CUR, NZ>(u, f);
#pragma unroll
    for (int r = 0; r < 16; ++r) ob[16 * f.t + r] = u[r];
}

template <int MODE>
__global__ __launch_bounds__(FT_THREADS, 2) void probe_kernel(const float2* x, const float2* y, float2* out,
                                                              const float2* gtab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* lds = reinterpret_cast<float2*>(smem_raw);
    const FtLane f = ft_setup(lds, gtab);
    const int t = f.t;
    const float2* xb = x + (size_t)blockIdx.x * FT_P;
    const float2* yb = y + (size_t)blockIdx.x * FT_P;
    float2* ob = out + (size_t)blockIdx.x * FT_P;
    float2 u[16], v[16];
    if (MODE == M_INV0 || MODE == M_INV1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) u[r] = xb[16 * t + r];
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { u[r] = xb[256 * r + t]; v[r] = yb[256 * r + t]; }
    }
    if (MODE == M_FWD0) fwd_freq_out<0, 16>(u, f, ob);
    else if (MODE == M_FWD1) fwd_freq_out<1, 16>(u, f, ob);
    else if (MODE == M_FWD0_NZ12) fwd_freq_out<0, 12>(u, f, ob);
    else if (MODE == M_FWD0_NZ8) fwd_freq_out<0, 8>(u, f, ob);
    else if (MODE == M_FWD1_NZ12) fwd_freq_out<1, 12>(u, f, ob);
    else if (MODE == M_FWD1_NZ8) fwd_freq_out<1, 8>(u, f, ob);
    else if (MODE == M_ROUNDTRIP) {
        ft4096_fwd<0>(u, f);
        ft4096_inv<1>(u, f);
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[256 * r + t] = u[r];
    } else if (MODE == M_INV0 || MODE == M_INV1) {
        if (MODE == M_INV0) ft4096_inv<0>(u, f);
        else ft4096_inv<1>(u, f);
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[256 * r + t] = u[r];
    } else if (MODE == M_SCHED_ALT || MODE == M_SCHED_CAF) {
        float2 acc[16];
        for (int rep = 0; rep < 2; ++rep) {
#pragma unroll
            for (int m = 0; m < 16; ++m) acc[m] = make_float2(0.f, 0.f);
            for (int piece = 0; piece < 3; ++piece) {
                float2 a[16], b[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { a[r] = u[r]; b[r] = v[r]; }
                ft4096_fwd<0>(a, f);
                ft4096_fwd<1>(b, f);
#pragma unroll
                for (int m = 0; m < 16; ++m) cmac_conj_a(acc[m], a[m], b[m]);
            }
            if (MODE == M_SCHED_ALT) ft4096_inv<1>(acc, f);
            else {
                ft4096_inv<0>(acc, f);
                ft_team_sync();           // fft_team.h: restarting at buffer 0 after an inverse that used buffer 0
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[256 * r + t] = acc[r];
    } else {
        // the fused LS pass keeps one spectrum and alternates fwd<1>, inv<0>: here conj(U) V goes through the inverse once
        // per piece and the three time-domain results are added (2 w is exact, 3 w is one rounding)
        float2 sum[16];
        for (int rep = 0; rep < 2; ++rep) {
            float2 a[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { a[r] = u[r]; sum[r] = make_float2(0.f, 0.f); }
            ft4096_fwd<1>(a, f);
            if (FT_NBUF == 2) ft_team_sync();     // two forward transforms on the same buffer (one-buffer builds: no hazard)
            for (int piece = 0; piece < 3; ++piece) {
                float2 b[16], w[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { b[r] = v[r]; w[r] = make_float2(0.f, 0.f); }
                ft4096_fwd<1>(b, f);
#pragma unroll
                for (int m = 0; m < 16; ++m) cmac_conj_a(w[m], a[m], b[m]);
                ft4096_inv<0>(w, f);
#pragma unroll
                for (int r = 0; r < 16; ++r) { sum[r].x += w[r].x; sum[r].y += w[r].y; }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[256 * r + t] = sum[r];
    }
}

template <int MODE>
static int launch(const float2* dx, const float2* dy, float2* dout, const float2* dtab, int nblocks) {
    const size_t lds = sizeof(float2) * FT_LDS_ELEMS;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&probe_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) return -2;
    hipLaunchKernelGGL(probe_kernel<MODE>, dim3(nblocks), dim3(FT_THREADS), lds, 0, dx, dy, dout, dtab);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// x, y, out: nblocks x 4096 complex64 on the host.  Returns 0, or a negative code (no kernel runs for an unknown mode).
extern "C" int fft_probe(const void* x_host, const void* y_host, void* out_host, int nblocks, int mode) {
    if (nblocks <= 0 || mode < 0 || mode >= M_COUNT) return -5;
    const float2* dtab = nullptr;
    if (ft_device_tables(&dtab) != 0) return -6;
    float2 *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = sizeof(float2) * FT_P * (size_t)nblocks;
    int rc = 0;
    if (hipMalloc(&dx, bytes) || hipMalloc(&dy, bytes) || hipMalloc(&dout, bytes)) rc = -1;
    if (rc == 0 && (hipMemcpy(dx, x_host, bytes, hipMemcpyHostToDevice) || hipMemcpy(dy, y_host, bytes, hipMemcpyHostToDevice)))
        rc = -1;
    if (rc == 0) {
        switch (mode) {
#define PROBE_CASE(M) case M: rc = launch<M>(dx, dy, dout, dtab, nblocks); break;
            PROBE_CASE(0) PROBE_CASE(1) PROBE_CASE(2) PROBE_CASE(3) PROBE_CASE(4) PROBE_CASE(5)
            PROBE_CASE(6) PROBE_CASE(7) PROBE_CASE(8) PROBE_CASE(9) PROBE_CASE(10) PROBE_CASE(11)
#undef PROBE_CASE
        }
    }
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = -3;
    if (rc == 0 && hipMemcpy(out_host, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
    hipFree(dx); hipFree(dy); hipFree(dout);
    return rc;
}

// the FT_* defines this library was built with, for the tests' own bookkeeping: NBUF | PK << 4 | FACTORED << 5 | TW2_REGS << 8
extern "C" int fft_probe_flags(void) {
    int v = FT_NBUF | (FT_TW2_REGS << 8);
#ifdef FT_PK
    v |= 1 << 4;
#endif
#ifdef FT_TW2_FACTORED
    v |= 1 << 5;
#endif
    return v;
}
