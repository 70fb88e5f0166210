// Packed-f32 radix-16 butterflies (fft_pk.h) against the scalar dft16 of fft_wave.h: VALU time of dft16 + 15 twiddle
// multiplies in registers at 1..5 wavefronts per SIMD, both forms.  hipcc -O3 --offload-arch=gfx950 -fno-slp-vectorize
// (That the two forms give the same bits is checked in the suite: tests/csrc/fft_probe_prim.hip, tests/test_gpu_fft_forms.py.)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../passiveradar_amd/csrc/fft_pk.h"
void prc_set_error(const char*, ...) {}

template <bool PK>
__global__ __launch_bounds__(256) void time_k(float2* out, int iters, float2 w) {
    extern __shared__ float2 lds[];
    float2 s = make_float2(0.f, 0.f);
    if (!PK) {
        float2 x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = make_float2((float)(threadIdx.x + r), (float)r * 0.5f);
        for (int i = 0; i < iters; ++i) {
            dft16<1>(x);
#pragma unroll
            for (int r = 1; r < 16; ++r) x[r] = mul_tw<1>(x[r], w);
#pragma unroll
            for (int r = 0; r < 16; ++r) { x[r].x *= 0.25f; x[r].y *= 0.25f; }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { s.x += x[r].x; s.y += x[r].y; }
    } else {
        v2f x[16];
        const v2f wv = pk_from(w);
#pragma unroll
        for (int r = 0; r < 16; ++r) x[r] = v2f{(float)(threadIdx.x + r), (float)r * 0.5f};
        for (int i = 0; i < iters; ++i) {
            pk_dft16<1>(x);
            pk_twiddle<1, 1>(x, [&](int) { return wv; });
#pragma unroll
            for (int r = 0; r < 16; ++r) x[r] = pk_scale(x[r], 0.25f);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { s.x += x[r].x; s.y += x[r].y; }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (iters < 0) lds[threadIdx.x] = s;
}

int main() {
    float2* d; hipMalloc(&d, 1 << 26);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipFuncSetAttribute((const void*)time_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)time_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const int iters = 4000;
    for (int pk = 0; pk < 2; ++pk)
        for (int wps = 1; wps <= 5; ++wps) {
            const size_t lds = (160 * 1024) / wps - 512;
            float ms = 0;
            for (int rep = 0; rep < 3; ++rep) {
                hipEventRecord(e0);
                if (pk) time_k<true><<<256 * wps, 256, lds>>>(d, iters, make_float2(0.6f, 0.8f));
                else time_k<false><<<256 * wps, 256, lds>>>(d, iters, make_float2(0.6f, 0.8f));
                hipEventRecord(e1); hipEventSynchronize(e1);
                hipEventElapsedTime(&ms, e0, e1);
            }
            printf("%s waves/SIMD %d: %.3f ms -> %.1f cycles@2.4GHz per iteration per SIMD\n", pk ? "packed" : "scalar", wps, ms,
                   ms * 1e-3 * 2.4e9 / ((double)iters * wps));
        }
    return 0;
}
