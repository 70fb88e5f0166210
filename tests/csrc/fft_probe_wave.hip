// TEST ONLY: exposes the one-wavefront 1024-point transform of passiveradar_amd/csrc/fft_wave.h (and, built with -DFT_PK,
// its packed-f32 twin fft_wave_pk.h) on its own.  Not part of libprcore, but linked against it: the twiddle table is the
// device copy the library itself uploads (fftw_device_tables).
// Four wavefronts per workgroup, one transform each, every wave in its own LDS tile and on its own data; after the
// barrier that closes the table load (fft_load_tables prescribes it) no workgroup barrier follows, as in the kernels.
#include "../../passiveradar_amd/csrc/fft_wave.h"

int fftw_device_tables(const float2** out);   // caf_fft.hip

#define PW_WAVES 4

// time layout     : lane l, register r <-> element 64 r + l of the transform
// frequency layout: lane l, register r <-> element 16 l + r of the transform (bin (l >> 2) + 16 r + 256 bitrev2(l & 3))
enum {
    W_FWD16 = 0,       // fft1024_fwd<16>: time in, frequency layout out
    W_FWD12 = 1,       // fft1024_fwd<12>: registers 12..15 are zero (as in the kernels: not even read)
    W_FWD8 = 2,
    W_INV = 3,         // fft1024_inv<false>: frequency layout in, time out (x 1024)
    W_INV_PRE = 4,     // fft1024_inv<true> on the spectrum times the lane's quad sign f.sg (the caller's part, done here)
    W_ROUNDTRIP = 5,   // fft1024_fwd, fft1024_inv: time in, time out (x 1024)
    W_SCHED = 6,       // (fwd, fwd, cmac_conj_a) x 3, inv -- twice, back to back on the one tile
    W_COUNT = 7
};

template <int NZ>
__device__ __forceinline__ void fwd_freq_out(float2 (&u)[16], float2* tile, const float2* tab, const FftLane& f, float2* ob) {
#pragma unroll
    for (int r = NZ; r < 16; ++r) u[r] = make_float2(0.f, 0.f);
    fft1024_fwd<NZ>(u, tile, tab, f);
#pragma unroll
    for (int r = 0; r < 16; ++r) ob[16 * f.lane + r] = u[r];
}

template <int MODE>
__global__ __launch_bounds__(64 * PW_WAVES) void probe_wave_kernel(const float2* x, const float2* y, float2* out,
                                                                   const float2* gtab, int n) {
    __shared__ __attribute__((aligned(16))) float2 smem[FFTW_TABLE + PW_WAVES * FFTW_TILE];
    float2* tab = smem;
    float2* tile = tab + FFTW_TABLE + (threadIdx.x >> 6) * FFTW_TILE;
    fft_load_tables(tab, gtab);
    __syncthreads();
    const FftLane f = fft_lane_setup();
    const int lane = f.lane;
    const int idx = blockIdx.x * PW_WAVES + (int)(threadIdx.x >> 6);
    if (idx >= n) return;                                    // whole waves; no barrier follows
    const float2* xb = x + (size_t)idx * FFTW_P;
    const float2* yb = y + (size_t)idx * FFTW_P;
    float2* ob = out + (size_t)idx * FFTW_P;
    float2 u[16], v[16];
    if (MODE == W_INV || MODE == W_INV_PRE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) u[r] = xb[16 * lane + r];
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) { u[r] = xb[64 * r + lane]; v[r] = yb[64 * r + lane]; }
    }
    if (MODE == W_FWD16) fwd_freq_out<16>(u, tile, tab, f, ob);
    else if (MODE == W_FWD12) fwd_freq_out<12>(u, tile, tab, f, ob);
    else if (MODE == W_FWD8) fwd_freq_out<8>(u, tile, tab, f, ob);
    else if (MODE == W_INV || MODE == W_INV_PRE || MODE == W_ROUNDTRIP) {
        if (MODE == W_ROUNDTRIP) fft1024_fwd(u, tile, tab, f);
        if (MODE == W_INV_PRE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { u[r].x *= f.sg; u[r].y *= f.sg; }
            fft1024_inv<true>(u, tile, tab, f);
        } else {
            fft1024_inv<false>(u, tile, tab, f);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[64 * r + lane] = u[r];
    } else {
        float2 acc[16];
        for (int rep = 0; rep < 2; ++rep) {
#pragma unroll
            for (int m = 0; m < 16; ++m) acc[m] = make_float2(0.f, 0.f);
            for (int piece = 0; piece < 3; ++piece) {
                float2 a[16], b[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { a[r] = u[r]; b[r] = v[r]; }
                fft1024_fwd(a, tile, tab, f);
                fft1024_fwd(b, tile, tab, f);
#pragma unroll
                for (int m = 0; m < 16; ++m) cmac_conj_a(acc[m], a[m], b[m]);
            }
            fft1024_inv(acc, tile, tab, f);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[64 * r + lane] = acc[r];
    }
}

template <int MODE>
static int launch(const float2* dx, const float2* dy, float2* dout, const float2* dtab, int n) {
    hipLaunchKernelGGL(probe_wave_kernel<MODE>, dim3((n + PW_WAVES - 1) / PW_WAVES), dim3(64 * PW_WAVES), 0, 0, dx, dy, dout, dtab, n);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// x, y, out: n x 1024 complex64 on the host.  Returns 0, or a negative code (no kernel runs for an unknown mode).
extern "C" int fft_probe_wave(const void* x_host, const void* y_host, void* out_host, int n, int mode) {
    if (n <= 0 || mode < 0 || mode >= W_COUNT) return -5;
    const float2* dtab = nullptr;
    if (fftw_device_tables(&dtab) != 0) return -6;
    float2 *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = sizeof(float2) * FFTW_P * (size_t)n;
    int rc = 0;
    if (hipMalloc(&dx, bytes) || hipMalloc(&dy, bytes) || hipMalloc(&dout, bytes)) rc = -1;
    if (rc == 0 && (hipMemcpy(dx, x_host, bytes, hipMemcpyHostToDevice) || hipMemcpy(dy, y_host, bytes, hipMemcpyHostToDevice)))
        rc = -1;
    if (rc == 0) {
        switch (mode) {
#define PROBE_CASE(M) case M: rc = launch<M>(dx, dy, dout, dtab, n); break;
            PROBE_CASE(0) PROBE_CASE(1) PROBE_CASE(2) PROBE_CASE(3) PROBE_CASE(4) PROBE_CASE(5) PROBE_CASE(6)
#undef PROBE_CASE
        }
    }
    if (rc == 0 && hipDeviceSynchronize() != hipSuccess) rc = -3;
    if (rc == 0 && hipMemcpy(out_host, dout, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
    hipFree(dx); hipFree(dy); hipFree(dout);
    return rc;
}

extern "C" int fft_probe_wave_packed(void) {
#ifdef FT_PK
    return 1;
#else
    return 0;
#endif
}
