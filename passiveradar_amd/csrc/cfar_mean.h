// The pieces the two CFAR units share (cfar.hip: cell average, cfar_os.hip: order statistic): how a map element becomes a
// magnitude on the tile load, and the block partial sums of mean|X| (CFAR_MEAN_PARTIALS blocks of 256 threads per frame; the
// CFAR kernels add a frame's partials in index order, so both units normalise by the same float32 mean).
#pragma once
#include "common.h"

#define CFAR_MEAN_PARTIALS 64

// The map comes in as magnitudes (float: CFAR_2D's own argument) or as the complex range-Doppler map itself (float2:
// range_doppler_plot.py:56-57 calls CFAR_2D(np.abs(xambg), ...) -- |X| is then taken on the tile load, one read of the
// complex map instead of an abs kernel's read + write and two reads of its result; np.abs of complex64 is hypotf).
__device__ __forceinline__ float cfar_mag(float v) { return v; }
__device__ __forceinline__ float cfar_mag(float2 v) { return hypotf(v.x, v.y); }

template <typename TIn>
__global__ void cfar_abs_partial_kernel(const TIn* __restrict__ X, int64_t n, float* __restrict__ partial) {
    __shared__ float red[256];
    const int f = blockIdx.y;
    const TIn* x = X + (int64_t)f * n;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += fabsf(cfar_mag(x[i]));
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)f * gridDim.x + blockIdx.x] = red[0];
}
