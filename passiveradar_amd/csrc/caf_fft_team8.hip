// Cross-ambiguity segment sums for wide range spans on the EIGHT-wavefront 4096-point transform (fft_team8.h).
//
// Same algorithm, same argument block and same workgroup -> work mapping as caf_fft_team.hip
// (range_doppler_processing.py:81-86 for the boxcar decimator, :72): per slow-time sample j the (q+1)-sample segment is
// cut into pieces, U = FFT(w ref piece), V = FFT(srv piece extended by the lag span), acc += conj(U) V, one inverse per
// segment and lag block.  What differs is the team: 512 threads hold 8 points each, so u, v and the accumulator are 48
// VGPRs instead of 96 and a CU's three teams are six wavefronts per SIMD instead of three (round 6: VERDICT r5 item 3 asked
// for this kernel to be BUILT and measured against the four-wavefront one; selected by PRC_OPT_CAF_TEAM8).
#include "caf_internal.h"
#include "fft_team8.h"
#include "caf_team.h"

#ifndef CAF8_WAVES_PER_SIMD
#define CAF8_WAVES_PER_SIMD 6            // three 512-thread teams per CU
#endif

template <bool HAS_WIN>
__global__ __launch_bounds__(F8_THREADS, CAF8_WAVES_PER_SIMD) void caf_fft_team8_kernel(CafTeamArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* lds = reinterpret_cast<float2*>(smem_raw);
    int ch, b, bx;
    if (!caft_work(a, &ch, &b, &bx)) return;
    const float2* __restrict__ ref = a.refs[ch] + (int64_t)b * a.s.frame_stride;
    const float2* __restrict__ srv = a.s.srv + (int64_t)b * a.s.frame_stride;
    const float* __restrict__ win = a.s.window;
    float2* __restrict__ ych = a.s.y + (int64_t)ch * a.y_ref_stride;               // this channel's surfaces
    const F8Lane f = f8_setup(lds, a.gtab + FT_TW1);                               // the W_4096^m part of the shared table
    const int t = f.t;
    // frame-relative 32-bit arithmetic (n < 2^31); everything but t is workgroup-uniform
    const int N = (int)a.s.n, NV = (int)a.s.n_valid;
    const int R = a.s.range_bins;
    const int B = a.piece, LB = a.lagblk;
    const unsigned vo8 = (unsigned)t * 8u, vo4 = (unsigned)t * 4u;

    for (int sg = 0; sg < a.segs; ++sg) {
        const int64_t j = (int64_t)bx * a.segs + sg;
        if (j >= a.s.freq_bins) break;                         // uniform
        const CaftSeg seg = caft_segment(a.s, j, N, B);
        const int lo = seg.lo, hi_f = seg.hi_f, tail = seg.tail;

        for (int lb = 0; lb < a.nlagblk; ++lb) {
            float2 acc[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[m] = make_float2(0.f, 0.f);
            for (int n0 = lo; n0 <= hi_f; n0 += B) {
                const int rem = hi_f - n0 + 1;
                const int cnt = rem < B ? rem : B;
                float2 u[8], v[8];
                // reference piece of cnt samples, zero-padded: the descriptor's num_records stands for "samples of this piece
                // that exist"; registers r >= nz (512 r >= cnt) are zero in every thread and are not even loaded
                const int nz = cnt <= 2048 ? 4 : (cnt <= 3072 ? 6 : 8);
                {
                    int c = cnt;
                    if (NV - n0 < c) c = NV - n0;
                    const __amdgpu_buffer_rsrc_t ru = prc_rsrc(ref + n0, prc_clampu(c) * 8u);
                    const __amdgpu_buffer_rsrc_t rw = prc_rsrc(win + (HAS_WIN ? n0 : 0), HAS_WIN ? prc_clampu(c) * 4u : 0u);
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        if (r < 4 || (r < 6 && nz > 4) || nz > 6) {
                            u[r] = prc_buf_load_c64(ru, vo8, 4096u * r);
                            if (HAS_WIN) {
                                const float wv = prc_buf_load_f32(rw, vo4, 2048u * r);
                                u[r].x *= wv;
                                u[r].y *= wv;
                            }
                        } else {
                            u[r] = make_float2(0.f, 0.f);
                        }
                    }
                }
                // surveillance slots [0, cnt + LB - 1) of this lag block, issued before the reference transform so that they
                // fly under it
                caft_load_srv(v, srv, n0 + lb * LB, cnt + LB - 1, N, NV, vo8);
                __builtin_amdgcn_sched_barrier(0);
                if (nz == 4) f8_fwd<4>(u, f);
                else if (nz == 6) f8_fwd<6>(u, f);
                else f8_fwd<8>(u, f);
                __builtin_amdgcn_sched_barrier(0);
                f8_fwd<8>(v, f);
#pragma unroll
                for (int m = 0; m < 8; ++m) cmac_conj_a(acc[m], u[m], v[m]);
            }
            f8_inv(acc, f);
            const int L0 = lb * LB;
            __builtin_amdgcn_sched_barrier(0);
            if (tail > 0) caft_tail<HAS_WIN>(acc, ref, srv, win, hi_f, tail, L0, LB, R, N, NV, t);
            caft_store(acc, a.s, ych, b, j, L0, LB, R, t);
        }
    }
}

int caf_launch_fft_team8(const CafTeamArgs& a, dim3 grid, bool has_window, hipStream_t stream) {
    const size_t lds = sizeof(float2) * F8_LDS_ELEMS;
    {
        int rc = prc_lds_optin(reinterpret_cast<const void*>(has_window ? &caf_fft_team8_kernel<true> : &caf_fft_team8_kernel<false>), (int)lds);
        if (rc) return rc;
    }
    if (has_window)
        hipLaunchKernelGGL((caf_fft_team8_kernel<true>), grid, dim3(F8_THREADS), lds, stream, a);
    else
        hipLaunchKernelGGL((caf_fft_team8_kernel<false>), grid, dim3(F8_THREADS), lds, stream, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
