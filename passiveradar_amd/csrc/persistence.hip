// persistence on device: plotting_tools.py persistence(X, k, hold, decay), the digital-phosphor sum of
// simple_kalman_tracker.py:113 and range_doppler_plot.py:72, for one frame or a whole stack of them.
//
//   frame = zeros; for i < min(k+1, hold): frame = frame + X[:, :, k-i] * decay**i
//
// Bitwise: the sum starts at +0.0 and adds the terms in order, each product and each sum rounded on its own (this file
// turns contraction off and spells the roundings with __dmul_rn / __dadd_rn); decay**i is Python's float power, the
// host libm pow(decay, i), computed here on the host and carried in the kernel arguments (no allocation, no copy, no
// synchronisation); a term whose power underflows to 0 is kept (Inf * 0 is NaN).  A float32 X multiplies in float32
// as NumPy >= 2 does with a Python float (NEP 50): fl32(x * fl32(decay**i)), then widens and adds in float64.
//
// Each thread owns one element of a frame and PERS_KB consecutive output frames: the inputs those outputs share are
// read again from L1 / L2, not HBM.  More than PERS_TERMS terms chain launches that continue the float64 sums in `out`.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int PT = 256;        // threads per workgroup
constexpr int PERS_TERMS = PRC_PERSISTENCE_TERMS_PER_LAUNCH;
constexpr int PERS_KB = 8;     // output frames per thread

struct PersArgs {
    int64_t elems;             // elements per frame
    int32_t k_first, k_count, hold;
    int32_t t0, nt;            // the terms i in [t0, t0 + nt) this launch adds
    double pw[PERS_TERMS];     // pw[i - t0] = pow(decay, i)
};

template <typename Tin, typename Tout>
__global__ __launch_bounds__(PT) void persistence_kernel(const Tin* __restrict__ frames, Tout* __restrict__ out,
                                                         PersArgs a) {
    const int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x;
    if (e >= a.elems) return;
    const int j0 = blockIdx.y * PERS_KB;
    const int j1 = min(a.k_count, j0 + PERS_KB);
    for (int j = j0; j < j1; ++j) {
        const int k = a.k_first + j;
        const int n = (k < 0 || a.hold <= 0) ? 0 : min(k + 1, a.hold);
        const int i1 = min(n, a.t0 + a.nt);
        Tout* o = out + (int64_t)j * a.elems + e;
        if (a.t0 > 0 && i1 <= a.t0) continue;        // a chained launch: this sum is complete already
        double acc = a.t0 == 0 ? 0.0 : (double)*o;
        for (int i = a.t0; i < i1; ++i) {
            const Tin x = frames[(int64_t)(k - i) * a.elems + e];
            double term;
            if constexpr (sizeof(Tin) == 4) term = (double)__fmul_rn(x, (float)a.pw[i - a.t0]);
            else term = __dmul_rn(x, a.pw[i - a.t0]);
            acc = __dadd_rn(acc, term);
        }
        *o = (Tout)acc;
    }
}

template <typename Tin, typename Tout>
int launch(const void* frames, void* out, PersArgs& a, double decay, int nterms, hipStream_t st) {
    const dim3 grid((uint32_t)((a.elems + PT - 1) / PT), (uint32_t)((a.k_count + PERS_KB - 1) / PERS_KB));
    a.t0 = 0;
    do {        // one launch when nterms <= PERS_TERMS (also for nterms == 0: it writes the zeros)
        a.nt = min(PERS_TERMS, nterms - a.t0);
        for (int i = 0; i < a.nt; ++i) a.pw[i] = pow(decay, (double)(a.t0 + i));
        hipLaunchKernelGGL((persistence_kernel<Tin, Tout>), grid, dim3(PT), 0, st, (const Tin*)frames, (Tout*)out, a);
        PRC_LAUNCH_CHECK();
        a.t0 += PERS_TERMS;
    } while (a.t0 < nterms);
    return PRC_OK;
}

}  // namespace

extern "C" int prc_persistence(const void* frames, int32_t in_dtype, int64_t frame_elems, int32_t nframes,
                               int32_t k_first, int32_t k_count, int32_t hold, double decay, void* out,
                               int32_t out_dtype, void* stream) {
    PRC_RANGE("prc_persistence");
    PRC_REQUIRE((in_dtype == PRC_REAL_F32 || in_dtype == PRC_REAL_F64) &&
                (out_dtype == PRC_REAL_F32 || out_dtype == PRC_REAL_F64), PRC_EINVAL,
                "prc_persistence: in_dtype = %d, out_dtype = %d: not PRC_REAL_F32 (0) or PRC_REAL_F64 (1)", in_dtype,
                out_dtype);
    PRC_REQUIRE(frame_elems >= 0 && nframes >= 0 && k_count >= 0, PRC_EINVAL,
                "prc_persistence: frame_elems = %lld, nframes = %d, k_count = %d", (long long)frame_elems, nframes,
                k_count);
    if (frame_elems == 0 || k_count == 0) return PRC_OK;
    PRC_REQUIRE((frame_elems + PT - 1) / PT <= 0x7fffffff, PRC_EINVAL, "prc_persistence: frame_elems = %lld exceeds the limit of %lld",
                (long long)frame_elems, (long long)PT * 0x7fffffff);
    PRC_REQUIRE((k_count + PERS_KB - 1) / PERS_KB <= PRC_MAX_BATCH, PRC_EINVAL, "prc_persistence: k_count = %d exceeds the limit of %d frames",
                k_count, PERS_KB * PRC_MAX_BATCH);
    PRC_REQUIRE(out, PRC_EINVAL, "prc_persistence: null out");
    PRC_REQUIRE((int64_t)k_first + k_count - 1 <= 0x7fffffff, PRC_EINVAL, "prc_persistence: k_first + k_count too large");
    const int64_t k_last = (int64_t)k_first + k_count - 1;
    // the frames read: k - i for i < min(k + 1, hold); the reference's first read is X[:, :, k]
    const int64_t nterms = (hold <= 0 || k_last < 0) ? 0 : (k_last + 1 < hold ? k_last + 1 : hold);
    if (nterms > 0) {
        PRC_REQUIRE(frames, PRC_EINVAL, "prc_persistence: null frames");
        PRC_REQUIRE(k_last < nframes, PRC_EINVAL, "prc_persistence: frame %lld read, the stack has %d frames",
                    (long long)k_last, nframes);
    }
    PRC_REQUIRE(out_dtype == PRC_REAL_F64 || nterms <= PERS_TERMS, PRC_EINVAL,
                "prc_persistence: %lld terms with a float32 out: at most %d (the launches chain through a float64 out)",
                (long long)nterms, PERS_TERMS);
    PersArgs a;
    a.elems = frame_elems;
    a.k_first = k_first;
    a.k_count = k_count;
    a.hold = hold;
    hipStream_t st = (hipStream_t)stream;
    const int nt = (int)nterms;
    if (in_dtype == PRC_REAL_F32)
        return out_dtype == PRC_REAL_F64 ? launch<float, double>(frames, out, a, decay, nt, st)
                                         : launch<float, float>(frames, out, a, decay, nt, st);
    return out_dtype == PRC_REAL_F64 ? launch<double, double>(frames, out, a, decay, nt, st)
                                     : launch<double, float>(frames, out, a, decay, nt, st);
}
