// Plot extraction: the cells of a CFAR statistic above a threshold, grouped into connected components ("plots"), one
// prc_track_cand per plot (include/prcore.h states the definition).
//
// plots_kernel: one 1024-thread workgroup per frame, as track_measure_kernel.  Three lists of C = 2^ceil(log2 max_cells)
// entries -- A (64-bit), B (64-bit), U (32-bit), 20 C bytes -- sit in LDS up to PRC_PLOTS_LDS_CELLS cells and in the
// frame's slice of the caller's workspace above (the same code; the global form puts __threadfence before every barrier,
// as the sort does (prc_bitonic, order_select.h), and reads what an atomic of the same phase may have changed with atomic loads).
//   1  stream the frame once (16-byte loads from the first aligned element, scalar head and tail), append the storage
//      index of every detecting cell to A through an LDS counter;
//   2  bitonic-sort A ascending: from here on nothing depends on the order of the appends;
//   3  union-find on positions in A (U = parent): the W neighbour is the previous entry or absent, the row above is one
//      binary search (NW, N, NE are adjacent entries); unite with atomicMin, so a root is its component's smallest
//      position = smallest storage index, and every retry of a unite strictly lowers the larger of its two positions;
//   4  B = (root's storage index << 32 | storage index), bitonic-sorted ascending: a plot's members are contiguous and in
//      ascending storage order;
//   5  peak per plot: atomicMax of (key(stat) << 32 | ~index) on A[head position] (an integer maximum: order-free);
//      heads turn it into the output key (key(strength) << 32 | flat index), everything else is 0; U = position;
//   6  bitonic-sort (A, U) descending: the first nplots entries are the plots in output order, U their head positions;
//   7  one thread per stored plot walks its members once, in ascending storage order, for the float64 sums and the box.
// Every loop is bounded by the list length or by a strictly decreasing position; no workgroup waits for another.
#include "common.h"
#include "order_select.h"

#include <math.h>

namespace {

constexpr int PT = 1024;                       // threads per workgroup
typedef unsigned long long u64;

struct PlotArgs {
    const float* stat;
    const void* weight;        // NULL: stat
    int weight_cplx;
    int H, W, conn8, range_guard, doppler_guard;
    uint32_t n, max_cells, C;
    int capacity;
    float thresh;
    double rstep, rstart, dstep, dstart;
    int32_t* counts;
    int32_t* ncells;
    prc_track_cand* cands;
    prc_plot_info* info;       // or NULL
    unsigned char* workspace;  // the global form: 20 C bytes per frame
};

// hypotf of a complex64 weight through float64: the squares are exact, one rounding in the sum, the root and the final
// conversion each -- the correctly rounded |z| except where the last two roundings compound (np.abs of complex64 likewise)
__device__ __forceinline__ float mag(float re, float im) {
    return (float)__dsqrt_rn(__dadd_rn(__dmul_rn((double)re, (double)re), __dmul_rn((double)im, (double)im)));
}

template <bool Global>
__device__ __forceinline__ void phase_sync() {
    if (Global) __threadfence();
    __syncthreads();
}

// a load of what an atomic of the running phase may have changed
template <bool Global, class T>
__device__ __forceinline__ T fresh(const T* p) {
    return Global ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// first position in K[0..n) whose entry is >= key
__device__ __forceinline__ uint32_t lower_bound(const u64* K, uint32_t n, u64 key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (K[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool Global>
__device__ __forceinline__ uint32_t find_root(const uint32_t* par, uint32_t x) {
    for (;;) {                                   // par[x] <= x everywhere: x only decreases
        const uint32_t q = fresh<Global>(par + x);
        if (q == x) return x;
        x = q;
    }
}

template <bool Global>
__device__ void unite(uint32_t* par, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root<Global>(par, a);
        b = find_root<Global>(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(par + a, b);      // a > b
        if (old == a) return;                            // a was a root and now hangs below b
        a = old;                                         // a had the parent old < a: that one and b still have to meet
    }
}

template <bool Global>
__global__ __launch_bounds__(PT) void plots_kernel(PlotArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plots_lds[];
    __shared__ uint32_t cnt, nplots;
    const uint32_t tid = threadIdx.x;
    const uint32_t f = blockIdx.x;
    unsigned char* base = Global ? a.workspace + (size_t)f * 20u * (size_t)a.C : plots_lds;
    u64* A = reinterpret_cast<u64*>(base);
    u64* B = A + a.C;
    uint32_t* U = reinterpret_cast<uint32_t*>(B + a.C);
    const uint32_t n = a.n, W = (uint32_t)a.W, H = (uint32_t)a.H;
    const float* x = a.stat + (size_t)f * (size_t)n;
    if (tid == 0) { cnt = 0u; nplots = 0u; }
    __syncthreads();

    // ---- 1: detections ----
    const uint32_t wlo = (uint32_t)a.range_guard, whi = W - (uint32_t)min(a.range_guard, a.W);
    const int c0 = a.H / 2 - a.doppler_guard, c1 = a.H / 2 + a.doppler_guard;
    auto consider = [&](uint32_t i, float v) {
        if (!(v > a.thresh)) return;                     // NaN never detects
        const uint32_t h = i / W, w = i - h * W;
        const int c = (int)(H - 1u - h);
        if (w < wlo || w >= whi || (c >= c0 && c < c1)) return;
        const uint32_t pos = atomicAdd(&cnt, 1u);
        if (pos < a.max_cells) A[pos] = (u64)i;
    };
    {
        uint32_t head = (uint32_t)((16u - ((uintptr_t)x & 15u)) & 15u) >> 2;      // elements before the first 16-byte line
        if (head > n) head = n;
        const uint32_t nvec = (n - head) >> 2, tail0 = head + 4u * nvec;
        if (tid < head) consider(tid, x[tid]);
        const float4* xv = reinterpret_cast<const float4*>(x + head);
        for (uint32_t v = tid; v < nvec; v += PT) {
            const float4 q = xv[v];
            const uint32_t i = head + 4u * v;
            consider(i, q.x); consider(i + 1u, q.y); consider(i + 2u, q.z); consider(i + 3u, q.w);
        }
        if (tail0 + tid < n) consider(tail0 + tid, x[tail0 + tid]);            // fewer than 4 elements
    }
    phase_sync<Global>();
    const uint32_t count = cnt;
    if (tid == 0) a.ncells[f] = (int32_t)count;
    if (count == 0u || count > a.max_cells) {
        if (tid == 0) a.counts[f] = 0;
        return;
    }

    // ---- 2: ascending storage order ----
    uint32_t P = 1;
    while (P < count) P <<= 1;
    for (uint32_t p = count + tid; p < P; p += PT) A[p] = ~0ull;
    phase_sync<Global>();
    prc_bitonic<PT, Global, false>(A, nullptr, P);

    // ---- 3: union-find over positions ----
    for (uint32_t p = tid; p < count; p += PT) U[p] = p;
    phase_sync<Global>();
    for (uint32_t p = tid; p < count; p += PT) {
        const uint32_t i = (uint32_t)A[p];
        const uint32_t h = i / W, w = i - h * W;
        if (w > 0u && p > 0u && (uint32_t)A[p - 1u] == i - 1u) unite<Global>(U, p, p - 1u);
        if (h > 0u) {
            const uint32_t first = i - W - (w > 0u ? 1u : 0u);       // NW, or N in the first column
            const uint32_t last = i - W + (w + 1u < W ? 1u : 0u);    // NE, or N in the last column
            for (uint32_t q = lower_bound(A, p, (u64)first); q < p; ++q) {   // at most three entries
                const uint32_t j = (uint32_t)A[q];
                if (j > last) break;
                if (a.conn8 || j == i - W) unite<Global>(U, p, q);
            }
        }
    }
    phase_sync<Global>();

    // ---- 4: members of a plot contiguous, in ascending storage order ----
    for (uint32_t p = tid; p < P; p += PT)
        B[p] = p < count ? (((u64)(uint32_t)A[find_root<Global>(U, p)] << 32) | (u64)(uint32_t)A[p]) : ~0ull;
    phase_sync<Global>();
    prc_bitonic<PT, Global, false>(B, nullptr, P);

    // ---- 5: peak per plot, then the output key at the head's position ----
    for (uint32_t p = tid; p < P; p += PT) { A[p] = 0ull; U[p] = p; }
    phase_sync<Global>();
    for (uint32_t p = tid; p < count; p += PT) {
        const u64 m = B[p];
        const uint32_t hp = lower_bound(B, p + 1u, m & 0xffffffff00000000ull);
        const uint32_t i = (uint32_t)m;
        atomicMax(A + hp, ((u64)prc_okey(x[i]) << 32) | (u64)(~i));      // the largest stat, then the smallest index
    }
    phase_sync<Global>();
    for (uint32_t p = tid; p < count; p += PT) {
        if (p > 0u && (B[p - 1u] >> 32) == (B[p] >> 32)) continue;   // not a head: A[p] stays 0
        const u64 acc = fresh<Global>(A + p);
        const uint32_t i = ~(uint32_t)acc;
        const uint32_t h = i / W, w = i - h * W;
        A[p] = (acc & 0xffffffff00000000ull) | (u64)(w * H + (H - 1u - h));      // keys of detections are > 0
        atomicAdd(&nplots, 1u);
    }
    phase_sync<Global>();
    const uint32_t np = nplots;
    if (tid == 0) a.counts[f] = (int32_t)np;

    // ---- 6: output order ----
    prc_bitonic<PT, Global, true>(A, U, P);

    // ---- 7: one fixed-order walk per stored plot ----
    const uint32_t m = np < (uint32_t)a.capacity ? np : (uint32_t)a.capacity;
    const float* wf = a.weight ? reinterpret_cast<const float*>(a.weight) + (size_t)f * (size_t)n * (a.weight_cplx ? 2u : 1u) : x;
    for (uint32_t r = tid; r < m; r += PT) {
        const uint32_t idx = (uint32_t)A[r], hp = U[r];
        const uint32_t wp = idx / H, hpk = H - 1u - (idx - wp * H);
        const uint32_t peak = hpk * W + wp;
        const u64 root = B[hp] >> 32;
        double M = 0.0, sh = 0.0, sw = 0.0;
        uint32_t nc = 0, h0 = 0, h1 = 0, w0 = W, w1 = 0;
        for (uint32_t q = hp; q < count && (B[q] >> 32) == root; ++q) {
            const uint32_t i = (uint32_t)B[q];
            const uint32_t h = i / W, w = i - h * W;
            const double g = (double)((a.weight && a.weight_cplx) ? mag(wf[2u * (size_t)i], wf[2u * (size_t)i + 1u]) : wf[i]);
            M = __dadd_rn(M, g);
            sh = __dadd_rn(sh, __dmul_rn(g, (double)h));             // the product is exact: 24 bits x < 2^24
            sw = __dadd_rn(sw, __dmul_rn(g, (double)w));
            if (nc == 0u) h0 = h;
            h1 = h;
            w0 = min(w0, w);
            w1 = max(w1, w);
            ++nc;
        }
        double hbar = (double)hpk, wbar = (double)wp;
        if (isfinite(M) && M > 0.0) {
            hbar = __ddiv_rn(sh, M);
            wbar = __ddiv_rn(sw, M);
        }
        const size_t o = (size_t)f * (size_t)a.capacity + r;
        prc_track_cand c;
        c.strength = (double)x[peak];
        c.range = __dadd_rn(__dmul_rn(wbar, a.rstep), a.rstart);
        c.doppler = __dadd_rn(__dmul_rn(__dsub_rn((double)(H - 1u), hbar), a.dstep), a.dstart);
        c.index = (int64_t)idx;
        a.cands[o] = c;
        if (a.info) {
            prc_plot_info pi;
            pi.mass = M; pi.hbar = hbar; pi.wbar = wbar;
            pi.ncells = (int32_t)nc; pi.h0 = (int32_t)h0; pi.h1 = (int32_t)h1; pi.w0 = (int32_t)w0; pi.w1 = (int32_t)w1;
            pi.peak = (int32_t)peak;
            a.info[o] = pi;
        }
    }
}

struct PlotShape { uint32_t n, max_cells, C; bool lds; };

int plots_check(prc_plots_desc* d, const prc_plots_desc* desc, int32_t nframes, PlotShape* sh, const char* who) {
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "%s: null descriptor", who);
    const int rc = prc_take_desc(d, desc, PRC_PLOTS_DESC_SIZE_MIN, who, "prc_plots_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d->H >= 2 && d->W >= 2, PRC_ESHAPE, "%s: H = %d, W = %d: a frame has at least 2 x 2 cells", who, d->H, d->W);
    PRC_REQUIRE((int64_t)d->H * d->W <= (int64_t)0x7fffffff, PRC_ESHAPE, "%s: H * W too large", who);
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "%s: nframes = %d", who, nframes);
    PRC_REQUIRE(d->connectivity == 4 || d->connectivity == 8, PRC_EINVAL, "%s: connectivity = %d, not 4 or 8", who, d->connectivity);
    PRC_REQUIRE(d->range_guard >= 0 && d->doppler_guard >= 0, PRC_EINVAL, "%s: range_guard = %d, doppler_guard = %d: not >= 0", who,
                d->range_guard, d->doppler_guard);
    PRC_REQUIRE(d->max_cells >= 1 && d->capacity >= 1, PRC_EINVAL, "%s: max_cells = %d, capacity = %d: not >= 1", who, d->max_cells,
                d->capacity);
    PRC_REQUIRE(!isnan(d->thresh), PRC_EINVAL, "%s: thresh is NaN", who);
    PRC_REQUIRE(isfinite(d->doppler_extent) && isfinite(d->range_extent), PRC_EINVAL, "%s: extents must be finite", who);
    sh->n = (uint32_t)(d->H * d->W);
    sh->max_cells = (uint32_t)d->max_cells < sh->n ? (uint32_t)d->max_cells : sh->n;     // a frame has no more detections than cells
    sh->lds = sh->max_cells <= (uint32_t)PRC_PLOTS_LDS_CELLS;
    uint32_t C = 1;
    while (C < sh->max_cells) C <<= 1;
    sh->C = C;
    return PRC_OK;
}

}  // namespace

extern "C" int prc_plots_workspace_bytes(const prc_plots_desc* desc, int32_t nframes, size_t* bytes) {
    prc_plots_desc d;
    PlotShape sh;
    const int rc = plots_check(&d, desc, nframes, &sh, "prc_plots_workspace_bytes");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(bytes != nullptr, PRC_EINVAL, "prc_plots_workspace_bytes: null pointer");
    *bytes = sh.lds ? 0 : (size_t)20 * (size_t)sh.C * (size_t)nframes;
    return PRC_OK;
}

extern "C" int prc_plots(const prc_plots_desc* desc, const float* stat, const void* weight, int32_t nframes, int32_t* counts,
                         int32_t* ncells_out, prc_track_cand* cands, prc_plot_info* info, void* workspace, void* stream) {
    PRC_RANGE("prc_plots");
    prc_plots_desc d;
    PlotShape sh;
    const int rc = plots_check(&d, desc, nframes, &sh, "prc_plots");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(weight == nullptr || d.weight_input == 0 || d.weight_input == 1, PRC_EINVAL,
                "prc_plots: weight_input = %d, not 0 (float32) or 1 (complex64)", d.weight_input);
    if (nframes == 0) return PRC_OK;
    PRC_REQUIRE(stat && counts && ncells_out && cands, PRC_EINVAL, "prc_plots: null pointer");
    PRC_REQUIRE(sh.lds || workspace, PRC_EINVAL, "prc_plots: max_cells = %d needs a workspace (prc_plots_workspace_bytes)", d.max_cells);
    PRC_REQUIRE(sh.lds || ((uintptr_t)workspace & 7u) == 0, PRC_EINVAL, "prc_plots: the workspace must be 8-byte aligned");
    PlotArgs a;
    a.stat = stat;
    a.weight = weight;
    a.weight_cplx = weight && d.weight_input == 1;
    a.H = d.H; a.W = d.W;
    a.conn8 = d.connectivity == 8;
    a.range_guard = d.range_guard; a.doppler_guard = d.doppler_guard;
    a.n = sh.n; a.max_cells = sh.max_cells; a.C = sh.C;
    a.capacity = d.capacity;
    a.thresh = d.thresh;
    // get_measurements' axes at a centroid: range = wbar * ((0 - R) / (W-1)) + R, doppler = ((H-1) - hbar) * (2 D / (H-1)) + (-D)
    a.rstart = d.range_extent;
    a.rstep = (0.0 - d.range_extent) / (double)(d.W - 1);
    a.dstart = -1.0 * d.doppler_extent;
    a.dstep = (2.0 * d.doppler_extent) / (double)(d.H - 1);
    a.counts = counts; a.ncells = ncells_out; a.cands = cands; a.info = info;
    a.workspace = (unsigned char*)workspace;
    if (sh.lds) {
        const size_t lds = (size_t)20 * sh.C;        // at most 80 KiB: above the 64 KiB a kernel gets without asking
        { const int rc_ = prc_lds_optin(reinterpret_cast<const void*>(&plots_kernel<false>), 20 * PRC_PLOTS_LDS_CELLS); if (rc_) return rc_; }
        hipLaunchKernelGGL(plots_kernel<false>, dim3(nframes), dim3(PT), lds, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(plots_kernel<true>, dim3(nframes), dim3(PT), 0, (hipStream_t)stream, a);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
