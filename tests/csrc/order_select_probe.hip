// TEST ONLY: runs the shared device primitives of passiveradar_amd/csrc/order_select.h and wave.h on their own
// (tests/test_gpu_order_select.py).  Not part of libprcore.  Every entry point takes host pointers, launches ONE workgroup and
// returns 0, -1 (allocation / copy), -3 (the device failed), -4 (the launch failed) or -5 (arguments outside the probe).
#include "../../passiveradar_amd/csrc/order_select.h"
#include "../../passiveradar_amd/csrc/wave.h"

#define OSP_THREADS 1024                 // prc_resolve_digit is written for this workgroup
#define OSP_LDS_KEYS 2048                // the largest sort the probe holds in LDS
#define OSP_GLOBAL_KEYS (1u << 16)       // ... and in global memory
#define OSP_MAX_RANKS 4096

typedef unsigned long long u64;

// ---- prc_resolve_digit: one histogram in LDS, one call per rank; sel starts as ~0 so that a call that selects nothing shows ----
__global__ __launch_bounds__(OSP_THREADS) void osp_resolve_kernel(const uint32_t* hist, int nb, const uint32_t* ranks, int nr,
                                                                  uint32_t* out) {
    __shared__ uint32_t h[PRC_RADIX_BINS];
    __shared__ uint32_t wave_tot[OSP_THREADS / PRC_WAVE];
    __shared__ uint32_t sel[3];
    const int tid = threadIdx.x;
    for (int b = tid; b < PRC_RADIX_BINS; b += OSP_THREADS) h[b] = b < nb ? hist[b] : 0xdeadu;   // bins past nb must not count
    for (int i = 0; i < nr; ++i) {
        if (tid < 3) sel[tid] = 0xffffffffu;
        __syncthreads();
        prc_resolve_digit(h, nb, ranks[i], wave_tot, sel);
        if (tid < 3) out[3 * i + tid] = sel[tid];
        __syncthreads();
    }
}

// ---- prc_bitonic: LDS form (copy in, sort, copy out) and global form (in place) ----
template <bool Global, bool Desc>
__global__ __launch_bounds__(OSP_THREADS) void osp_bitonic_kernel(u64* K, uint32_t* V, uint32_t P) {
    if (Global) {
        prc_bitonic<OSP_THREADS, true, Desc>(K, V, P);
        return;
    }
    __shared__ u64 k[OSP_LDS_KEYS];
    __shared__ uint32_t v[OSP_LDS_KEYS];
    for (uint32_t i = threadIdx.x; i < P; i += OSP_THREADS) { k[i] = K[i]; if (V) v[i] = V[i]; }
    __syncthreads();
    prc_bitonic<OSP_THREADS, false, Desc>(k, V ? v : nullptr, P);
    for (uint32_t i = threadIdx.x; i < P; i += OSP_THREADS) { K[i] = k[i]; if (V) V[i] = v[i]; }
}

// ---- wave.h: one wavefront, every lane stores what it holds after the call ----
struct OspWaveIn {
    double d[64];
    u64 q[64];
    uint32_t u[64];
    float yr[64], yi[64], bb[64];
};
struct OspWaveOut {
    double sum[64];
    u64 minq[64];
    uint32_t minu[64];
    float a2r[64], a2i[64], a3r[64], a3i[64], a3b[64];
};
__global__ __launch_bounds__(64) void osp_wave_kernel(const OspWaveIn* in, OspWaveOut* out) {
    const int l = threadIdx.x;
    out->sum[l] = wave_sum(in->d[l]);
    out->minq[l] = wave_min(in->q[l]);
    out->minu[l] = wave_min(in->u[l]);
    float yr = in->yr[l], yi = in->yi[l];
    wave_allsum2(yr, yi);
    out->a2r[l] = yr;
    out->a2i[l] = yi;
    float zr = in->yr[l], zi = in->yi[l], bb = in->bb[l];
    wave_allsum3(zr, zi, bb);
    out->a3r[l] = zr;
    out->a3i[l] = zi;
    out->a3b[l] = bb;
}

namespace {

// device copies of the host arrays of one call; freed when the call returns
struct Dev {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    void* up(const void* host, size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
        p[n++] = d;
        if (host && hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    ~Dev() { for (int i = 0; i < n; ++i) hipFree(p[i]); }
};

int finish(void* host, const void* dev, size_t bytes) {
    if (hipGetLastError() != hipSuccess) return -4;
    if (hipDeviceSynchronize() != hipSuccess) return -3;
    return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

}  // namespace

// out[i] = (bin, count below it, count in it) of ranks[i] in hist[0..nb)
extern "C" int osp_resolve(const uint32_t* hist, int nb, const uint32_t* ranks, int nr, uint32_t* out) {
    if (nb < 1 || nb > PRC_RADIX_BINS || nr < 1 || nr > OSP_MAX_RANKS) return -5;
    Dev d;
    uint32_t* dh = (uint32_t*)d.up(hist, sizeof(uint32_t) * nb);
    uint32_t* dr = (uint32_t*)d.up(ranks, sizeof(uint32_t) * nr);
    uint32_t* dout = (uint32_t*)d.up(nullptr, sizeof(uint32_t) * 3 * nr);
    if (!dh || !dr || !dout) return -1;
    hipLaunchKernelGGL(osp_resolve_kernel, dim3(1), dim3(OSP_THREADS), 0, 0, dh, nb, dr, nr, dout);
    return finish(out, dout, sizeof(uint32_t) * 3 * nr);
}

// sorts keys[0..P) in place, vals (or NULL) carried along; global = 0: in LDS (P <= 2048), 1: in global memory
extern "C" int osp_bitonic(u64* keys, uint32_t* vals, uint32_t P, int desc, int global) {
    if (P < 2 || (P & (P - 1)) || P > (global ? OSP_GLOBAL_KEYS : (uint32_t)OSP_LDS_KEYS)) return -5;
    Dev d;
    u64* dk = (u64*)d.up(keys, sizeof(u64) * P);
    uint32_t* dv = vals ? (uint32_t*)d.up(vals, sizeof(uint32_t) * P) : nullptr;
    if (!dk || (vals && !dv)) return -1;
    const dim3 g(1), b(OSP_THREADS);
    if (global && desc) hipLaunchKernelGGL((osp_bitonic_kernel<true, true>), g, b, 0, 0, dk, dv, P);
    else if (global) hipLaunchKernelGGL((osp_bitonic_kernel<true, false>), g, b, 0, 0, dk, dv, P);
    else if (desc) hipLaunchKernelGGL((osp_bitonic_kernel<false, true>), g, b, 0, 0, dk, dv, P);
    else hipLaunchKernelGGL((osp_bitonic_kernel<false, false>), g, b, 0, 0, dk, dv, P);
    int rc = finish(keys, dk, sizeof(u64) * P);
    if (rc == 0 && vals && hipMemcpy(vals, dv, sizeof(uint32_t) * P, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
    return rc;
}

extern "C" int osp_wave(const OspWaveIn* in, OspWaveOut* out) {
    Dev d;
    OspWaveIn* di = (OspWaveIn*)d.up(in, sizeof(OspWaveIn));
    OspWaveOut* dout = (OspWaveOut*)d.up(nullptr, sizeof(OspWaveOut));
    if (!di || !dout) return -1;
    hipLaunchKernelGGL(osp_wave_kernel, dim3(1), dim3(64), 0, 0, di, dout);
    return finish(out, dout, sizeof(OspWaveOut));
}

// the test's view of the two structs must be this one
extern "C" int osp_wave_in_bytes(void) { return (int)sizeof(OspWaveIn); }
extern "C" int osp_wave_out_bytes(void) { return (int)sizeof(OspWaveOut); }
