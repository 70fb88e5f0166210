// Non-coherent fusion of K illuminators' range-Doppler maps on a Cartesian position-velocity grid (include/prcore.h states
// the definition).  Per position cell and illuminator the geometry -- col, g_x, g_y -- is float64,
// every operation rounded on its own in the header's order; per velocity hypothesis j the row is five more such operations
// and the sample one gather; the hypotheses of a cell are reduced to (best, vel) under "larger S wins, ties to the lower j".
//
// One kernel body, two forms (template argument), the same bytes out:
//   both: a workgroup owns a square tile of position cells and a run of frames; TPC adjacent lanes share
//     a cell and split its hypotheses j = sub, sub + TPC, ... (each ascending, so a lane's partial is the lowest j of its
//     largest S); the partials are merged by xor-shuffles under the definition's rule.  The geometry is computed once per
//     workgroup and kept in registers for every frame of the run: K is a template argument, so no array is indexed at run time.
//   global form (8 x 8 cells, 4 lanes a cell: 256 threads): the samples are gathered from global memory, every index 64-bit.
//   LDS form (up to four illuminators 8 x 8 cells, 16 lanes a cell: 1024 threads, 16 wavefronts, four per SIMD, what
//     ds_read_b32 needs to reach its rate; above four 4 x 4 cells, 32 lanes a cell: 512 threads, the registers of 6 K values
//     of geometry a lane, and K bands narrow enough to fit): neighbouring cells see
//     neighbouring columns, so of illuminator k the tile reads only the band [cmin_k, cmax_k] of columns (over the tile's
//     in-range cells, a wave shuffle and one pass over the wavefronts' K pairs in LDS).  Where H sum_k (cmax_k - cmin_k + 1) floats fit
//     the dynamic LDS (PRC_FUSE_LDS_BYTES less the 2 KiB of the reduction and the band table), each frame's K bands are staged [H][bw_k] with
//     loads that are contiguous along a row and the gathers read LDS; a tile whose bands do not fit gathers from global
//     memory as the global form does (the decision is uniform in the workgroup and depends on the arguments alone).
//     Banks: a gather is one ds_read_b32 at (row bw_k + c): the TPC lanes of a cell read one column at neighbouring rows
//     (stride bw_k dwords), lanes that agree broadcast; the pattern is data-dependent and no padding helps all of it.
// No atomics, no allocation, nothing waits for another workgroup; every store is a plain store of a cell this workgroup owns.
#include "common.h"

#include <math.h>
#include <algorithm>

// every double operation below is spelled with its rounding; this keeps the compiler from fusing what is left
#pragma clang fp contract(off)

// tile edge (cells, log2) and lanes per cell (log2): DESIGN.md section 27 has the listing and the measurement
#ifndef FUSE_TILE_LOG2
#define FUSE_TILE_LOG2 3        // 8 x 8 cells: the global form, and the LDS form up to four illuminators
#endif
#ifndef FUSE_TILE_MANY_LOG2
#define FUSE_TILE_MANY_LOG2 2   // 4 x 4 cells: the LDS form above four illuminators (the K bands of an 8 x 8 tile rarely fit)
#endif
#ifndef FUSE_TPC_LOG2
#define FUSE_TPC_LOG2 4         // LDS form: 16 lanes a cell (32 on the 4 x 4 tile)
#endif
#ifndef FUSE_G_TPC_LOG2
#define FUSE_G_TPC_LOG2 2       // global form: 4 lanes a cell
#endif

namespace {

// lanes per cell: the LDS form runs 1024 threads up to four illuminators and 512 above (a lane holds 6 K registers of
// geometry: at 1024 threads, 128 registers a lane, five illuminators and more spilled)
constexpr int fuse_tile_log2(int K, bool lds) { return lds && K > 4 ? FUSE_TILE_MANY_LOG2 : FUSE_TILE_LOG2; }
constexpr int fuse_tpc_log2(int K, bool lds) { return lds ? (K <= 4 ? FUSE_TPC_LOG2 : FUSE_TPC_LOG2 + 1) : FUSE_G_TPC_LOG2; }
constexpr int fuse_threads(int K, bool lds) { return 1 << (2 * fuse_tile_log2(K, lds) + fuse_tpc_log2(K, lds)); }
static_assert(fuse_threads(1, true) == 1024 && fuse_threads(8, true) == 512 && fuse_threads(8, false) == 256, "tile x lanes per cell");
static_assert(FUSE_TPC_LOG2 + 1 <= 6 && FUSE_G_TPC_LOG2 <= 6, "the lanes of a cell share a wavefront");
// the head of the dynamic LDS: a copy of the illuminator rows (the geometry reads them from here: 14 K scalar registers of
// kernel arguments less at the top of the kernel) and of the K map offsets k illum_stride, the wavefronts' column ranges [16][8][2] int32, the band table [8][4] int32
constexpr int KOFF_OFF = 576, VEL_OFF = 640, ILLUM_BYTES = 704, RED_OFF = ILLUM_BYTES, TAB_OFF = RED_OFF + 1024, HEAD_BYTES = 2048;
static_assert(PRC_FUSE_MAX_ILLUM * PRC_FUSE_ILLUM_DOUBLES * 8 <= KOFF_OFF && KOFF_OFF + 8 * PRC_FUSE_MAX_ILLUM <= VEL_OFF && VEL_OFF + 32 <= ILLUM_BYTES && TAB_OFF + 8 * 4 * 4 <= HEAD_BYTES, "head of the LDS");
constexpr int FUSE_TARGET_WGS = 1024;      // workgroups a launch aims for: four per compute unit of an MI355X

struct FuseArgs {
    const float* stat;
    float* best;
    int32_t* vel;                  // or NULL
    int64_t illum_stride, frame_stride;
    int nframes, fpr;              // frames per run (blockIdx.y)
    int H, W, nx, ny, nvx, nvy, tiles_x, combine;
    int lds_floats;                // floats of the band area (LDS form)
    double x0, dx, y0, dy, z, vx0, dvx, vy0, dvy, rx[3];
    double illum[PRC_FUSE_MAX_ILLUM][PRC_FUSE_ILLUM_DOUBLES];
};

__device__ __forceinline__ double fuse_dist(double ax, double ay, double az) {
    return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ax, ax), __dmul_rn(ay, ay)), __dmul_rn(az, az)));
}
__device__ __forceinline__ double fuse_quot(double a, double d) { return d == 0.0 ? 0.0 : __ddiv_rn(a, d); }

// larger S wins, at equal S the lower j (two partials that chose nothing are both (-Inf, -1))
__device__ __forceinline__ void fuse_merge(float& S, int& j, float So, int jo) {
    if (So > S || (So == S && jo < j)) { S = So; j = jo; }
}

// The hypotheses j = sub, sub + TPC, ... of one cell against one frame: (S_best, j_best) of this lane's share.
// FROM_LDS: src is the staged image, at[k] = where this cell's column lies in it (-1: the column misses), stride[k] = bw_k;
// else src is the frame's first map, at[k] = the column (-1: it misses) and every index is formed in 64 bits.
template <int K, int TPC, bool FROM_LDS>
__device__ __forceinline__ void fuse_scan(const FuseArgs& a, const double (&gx)[K], const double (&gy)[K], const int (&at)[K],
                                          const int (&stride)[K], const double (&row0)[K], const double (&rph)[K], const int64_t (&koff)[K],
                                          const double (&vp)[4], const float* src, int sub, int nv, float& S_best, int& j_best) {
    const double hmax = (double)(a.H - 1);
    int jy = sub / a.nvx, jx = sub - jy * a.nvx;
    for (int j = sub; j < nv; j += TPC) {
        const double vx = __dadd_rn(vp[0], __dmul_rn((double)jx, vp[1]));
        const double vy = __dadd_rn(vp[2], __dmul_rn((double)jy, vp[3]));
        float S = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double fd = -__dadd_rn(__dmul_rn(gx[k], vx), __dmul_rn(gy[k], vy));
            const double r = rint(__dadd_rn(row0[k], __dmul_rn(fd, rph[k])));
            // compared in float64: a NaN or a huge row misses.  A miss loads element 0 (of the staged image / of the frame's
            // first map: always there) and drops it: no branch, so the K loads of a hypothesis are in flight together.
            const bool hit = at[k] >= 0 && r >= 0.0 && r <= hmax;
            const int row = hit ? (int)r : 0;
            float s;
            if (FROM_LDS) s = src[hit ? at[k] + row * stride[k] : 0];
            else s = src[hit ? koff[k] + (int64_t)row * a.W + at[k] : (int64_t)0];
            s = hit ? s : 0.0f;
            if (k == 0) S = s;
            else if (a.combine == PRC_FUSE_SUM) S = __fadd_rn(S, s);
            else S = s < S ? s : S;
        }
        if (S > S_best) { S_best = S; j_best = j; }
        jx += TPC;
        while (jx >= a.nvx) { jx -= a.nvx; ++jy; }
    }
}

template <int K, bool LDS>
__global__ __launch_bounds__(fuse_threads(K, LDS)) void fuse_kernel(FuseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fuse_lds[];
    constexpr int TPC_LOG2 = fuse_tpc_log2(K, LDS), TPC = 1 << TPC_LOG2, NT = fuse_threads(K, LDS), NWAVES = NT / PRC_WAVE;
    const int tid = (int)threadIdx.x, sub = tid & (TPC - 1), cell = tid >> TPC_LOG2;
    const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
    constexpr int TL = fuse_tile_log2(K, LDS);
    const int64_t ix = ((int64_t)tile_x << TL) + (cell & ((1 << TL) - 1));
    const int64_t iy = ((int64_t)tile_y << TL) + (cell >> TL);
    const bool live = ix < a.nx && iy < a.ny;
    const int H = a.H, W = a.W;

    // ---- geometry of this cell, once per run of frames ------------------------------------------------------------------
    double gx[K], gy[K], row0[K], rph[K];      // row0, rph: per lane although uniform, read from the LDS copy (see HEAD_BYTES)
    int col[K];                                 // -1: the column misses the map
    double* illum = reinterpret_cast<double*>(fuse_lds);
    int64_t* koffs = reinterpret_cast<int64_t*>(fuse_lds + KOFF_OFF);
    if (tid < K * PRC_FUSE_ILLUM_DOUBLES) illum[tid] = (&a.illum[0][0])[tid];
    if (tid < K) koffs[tid] = (int64_t)tid * a.illum_stride;
    double* vels = reinterpret_cast<double*>(fuse_lds + VEL_OFF);
    if (tid == 0) { vels[0] = a.vx0; vels[1] = a.dvx; vels[2] = a.vy0; vels[3] = a.dvy; }
    __syncthreads();
    // vx0, dvx, vy0, dvy: above four illuminators per lane too (the scalar registers run out at K = 8); up to four the lanes
    // have no registers to spare at 1024 threads and the scalar ones suffice
    double vp[4] = {a.vx0, a.dvx, a.vy0, a.dvy};
    if constexpr (K > 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) vp[i] = vels[i];
    }
    int64_t koff[K];                            // where illuminator k's map starts in a frame: per lane for the same reason
#pragma unroll
    for (int k = 0; k < K; ++k) koff[k] = koffs[k];
    {
        const double px = __dadd_rn(a.x0, __dmul_rn((double)ix, a.dx)), py = __dadd_rn(a.y0, __dmul_rn((double)iy, a.dy)), pz = a.z;
        const double rxx = __dsub_rn(px, a.rx[0]), rxy = __dsub_rn(py, a.rx[1]), rxz = __dsub_rn(pz, a.rx[2]);
        const double dr = fuse_dist(rxx, rxy, rxz);
        const double qrx = fuse_quot(rxx, dr), qry = fuse_quot(rxy, dr);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double* p = illum + k * PRC_FUSE_ILLUM_DOUBLES;
            const double tx = __dsub_rn(px, p[0]), ty = __dsub_rn(py, p[1]), tz = __dsub_rn(pz, p[2]);
            const double dt = fuse_dist(tx, ty, tz);
            const double c = rint(__dadd_rn(p[5], __dmul_rn(__dsub_rn(__dadd_rn(dt, dr), p[4]), p[6])));
            col[k] = live && c >= 0.0 && c <= (double)(W - 1) ? (int)c : -1;      // a NaN fails both comparisons
            gx[k] = __ddiv_rn(__dadd_rn(fuse_quot(tx, dt), qrx), p[3]);
            gy[k] = __ddiv_rn(__dadd_rn(fuse_quot(ty, dt), qry), p[3]);
            row0[k] = p[7];
            rph[k] = p[8];
        }
    }

    // ---- LDS form: the tile's band of columns per illuminator -----------------------------------------------------------
    // The table {cmin, bw, off} per illuminator stays in LDS (the staging loop reads it again every frame: keeping 3 K more
    // uniform values live across the scan is what made the compiler spill); a lane keeps only where ITS column lies in the
    // staged image, pos[k] = off_k + col_k - cmin_k, and the row stride bw_k.
    int pos[K] = {}, bws[K] = {};
    bool staged = false;
    float* band = reinterpret_cast<float*>(fuse_lds + HEAD_BYTES);
    int* tab = reinterpret_cast<int*>(fuse_lds + TAB_OFF);
    if constexpr (LDS) {
        int* red = reinterpret_cast<int*>(fuse_lds + RED_OFF);
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // a missing column is -1: the largest unsigned, so INT_MAX as lo, and -1 as hi (no compare: its mask would live on)
            int lo = (int)min((unsigned)col[k], 0x7fffffffu), hi = col[k];
#pragma unroll
            for (int m = 1; m < PRC_WAVE; m <<= 1) {
                lo = min(lo, __shfl_xor(lo, m));
                hi = max(hi, __shfl_xor(hi, m));
            }
            if (lane == 0) { red[(wave * 8 + k) * 2] = lo; red[(wave * 8 + k) * 2 + 1] = hi; }
        }
        __syncthreads();
        int64_t need = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int lo = 0x7fffffff, hi = -1;
            for (int w = 0; w < NWAVES; ++w) {
                lo = min(lo, red[(w * 8 + k) * 2]);
                hi = max(hi, red[(w * 8 + k) * 2 + 1]);
            }
            const int cmin = hi < 0 ? 0 : lo;
            bws[k] = hi < 0 ? 0 : hi - lo + 1;
            // the offset is used only where everything fits, and then it is below lds_floats
            pos[k] = (col[k] >> 31) | ((int)need + (col[k] - cmin));          // -1 stays -1
            if (tid == 0) { tab[4 * k] = cmin; tab[4 * k + 1] = bws[k]; tab[4 * k + 2] = (int)need; }
            need += (int64_t)H * bws[k];
        }
        staged = need <= (int64_t)a.lds_floats;
        __syncthreads();                        // the table is written
    }

    const int nv = a.nvx * a.nvy;
    const int f0 = (int)blockIdx.y * a.fpr, f1 = min(a.nframes, f0 + a.fpr);
    for (int f = f0; f < f1; ++f) {
        const float* frame = a.stat + (int64_t)f * a.frame_stride;
        if constexpr (LDS) {
            if (staged) {
                if (f != f0) __syncthreads();   // the gathers of the frame before are done
#pragma unroll 1
                for (int k = 0; k < K; ++k) {   // rolled: the K copies' pointers and counts would all be hoisted out of the frame loop
                    const int cmin = tab[4 * k], b = tab[4 * k + 1], off = tab[4 * k + 2];
                    const float* src = frame + koffs[k] + cmin;
                    const unsigned n = (unsigned)H * (unsigned)b;
                    for (unsigned i = (unsigned)tid; i < n; i += NT) {
                        const unsigned h = i / (unsigned)b, c = i - h * (unsigned)b;
                        band[off + i] = src[(int64_t)h * W + c];
                    }
                }
                __syncthreads();
            }
        }
        float S_best = -INFINITY;
        int j_best = -1;
        if (live) {
            if (LDS && staged) fuse_scan<K, TPC, true>(a, gx, gy, pos, bws, row0, rph, koff, vp, band, sub, nv, S_best, j_best);
            else fuse_scan<K, TPC, false>(a, gx, gy, col, bws, row0, rph, koff, vp, frame, sub, nv, S_best, j_best);
        }
#pragma unroll
        for (int m = 1; m < TPC; m <<= 1) {
            const float So = __shfl_xor(S_best, m);
            const int jo = __shfl_xor(j_best, m);
            fuse_merge(S_best, j_best, So, jo);
        }
        if (live && sub == 0) {
            const int64_t o = ((int64_t)f * a.ny + iy) * a.nx + ix;
            a.best[o] = S_best;
            if (a.vel) a.vel[o] = j_best;
        }
    }
}

template <int K>
int fuse_launch(const FuseArgs& a, bool lds, unsigned tiles, unsigned runs, hipStream_t stream) {
    if (lds) {
        const int rc = prc_lds_optin(reinterpret_cast<const void*>(&fuse_kernel<K, true>), PRC_FUSE_LDS_BYTES);
        if (rc) return rc;
        hipLaunchKernelGGL((fuse_kernel<K, true>), dim3(tiles, runs), dim3(fuse_threads(K, true)), PRC_FUSE_LDS_BYTES, stream, a);
    } else {
        hipLaunchKernelGGL((fuse_kernel<K, false>), dim3(tiles, runs), dim3(fuse_threads(K, false)), ILLUM_BYTES, stream, a);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

// maps [H][W] at k illum_stride + f frame_stride, k < K, f < nframes, pairwise disjoint: one of the two strides steps over
// everything the other spans (a stride over a single map is not looked at)
bool fuse_strides_ok(int64_t HW, int K, int64_t is, int nframes, int64_t fs) {
    const auto span = [HW](int64_t stride, int n) -> __int128 { return (__int128)stride * (n - 1) + HW; };
    if (K > 1 && is < HW) return false;
    if (nframes > 1 && fs < HW) return false;
    if (K == 1 || nframes == 1) return true;
    return (__int128)is >= span(fs, nframes) || (__int128)fs >= span(is, K);
}

}  // namespace

extern "C" int prc_fuse(const prc_fuse_desc* desc, const double* illum_host, const float* stat, int64_t illum_stride,
                        int64_t frame_stride, int32_t nframes, float* best, int32_t* vel, void* stream) {
    PRC_RANGE("prc_fuse");
    PRC_REQUIRE(desc != nullptr, PRC_EINVAL, "prc_fuse: null descriptor");
    prc_fuse_desc d;
    const int rc = prc_take_desc(&d, desc, PRC_FUSE_DESC_SIZE_MIN, "prc_fuse", "prc_fuse_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d.nillum >= 1 && d.nillum <= PRC_FUSE_MAX_ILLUM, PRC_EINVAL, "prc_fuse: nillum = %d outside 1 .. %d", d.nillum,
                PRC_FUSE_MAX_ILLUM);
    PRC_REQUIRE(d.H >= 1 && d.W >= 1, PRC_EINVAL, "prc_fuse: H = %d, W = %d: a map has at least one cell", d.H, d.W);
    PRC_REQUIRE((int64_t)d.H * d.W <= (int64_t)0x7fffffff, PRC_EINVAL, "prc_fuse: H * W = %lld above 2^31 - 1",
                (long long)((int64_t)d.H * d.W));
    PRC_REQUIRE(d.nx >= 1 && d.ny >= 1, PRC_EINVAL, "prc_fuse: nx = %d, ny = %d: the grid has at least one cell", d.nx, d.ny);
    PRC_REQUIRE((int64_t)d.nx * d.ny <= (int64_t)0x7fffffff, PRC_EINVAL, "prc_fuse: nx * ny = %lld above 2^31 - 1",
                (long long)((int64_t)d.nx * d.ny));
    const bool lds = d.form != PRC_FUSE_FORM_GLOBAL;  // the shipped choice is the LDS form (its tiles fall back one by one)
    // the limit is that of the smallest tile, whatever runs: one workgroup a tile, 2^22 x 1024 threads stay below 2^32
    const int64_t tmin = ceil_div64(d.nx, 1 << FUSE_TILE_MANY_LOG2) * ceil_div64(d.ny, 1 << FUSE_TILE_MANY_LOG2);
    PRC_REQUIRE(tmin <= (int64_t)1 << 22, PRC_EINVAL, "prc_fuse: nx = %d, ny = %d: %lld tiles of %d x %d cells, above 2^22", d.nx, d.ny,
                (long long)tmin, 1 << FUSE_TILE_MANY_LOG2, 1 << FUSE_TILE_MANY_LOG2);
    const int tl = fuse_tile_log2(d.nillum, lds);
    const int64_t tx = ceil_div64(d.nx, 1 << tl), ty = ceil_div64(d.ny, 1 << tl), tiles = tx * ty;
    PRC_REQUIRE(d.nvx >= 1 && d.nvy >= 1, PRC_EINVAL, "prc_fuse: nvx = %d, nvy = %d: at least one hypothesis", d.nvx, d.nvy);
    PRC_REQUIRE((int64_t)d.nvx * d.nvy <= (int64_t)0x7fffffff, PRC_EINVAL, "prc_fuse: nvx * nvy = %lld above 2^31 - 1",
                (long long)((int64_t)d.nvx * d.nvy));
    PRC_REQUIRE(d.combine == PRC_FUSE_SUM || d.combine == PRC_FUSE_MIN, PRC_EINVAL, "prc_fuse: combine = %d is neither PRC_FUSE_SUM nor "
                "PRC_FUSE_MIN", d.combine);
    PRC_REQUIRE(d.form >= PRC_FUSE_FORM_AUTO && d.form <= PRC_FUSE_FORM_LDS, PRC_EINVAL, "prc_fuse: form = %d outside 0 .. 2", d.form);
    const double grid[] = {d.x0, d.dx, d.y0, d.dy, d.z, d.vx0, d.dvx, d.vy0, d.dvy, d.rx[0], d.rx[1], d.rx[2]};
    for (double v : grid) PRC_REQUIRE(isfinite(v), PRC_EINVAL, "prc_fuse: a grid, velocity or receiver parameter is not finite");
    PRC_REQUIRE(illum_host != nullptr, PRC_EINVAL, "prc_fuse: null illum_host");
    for (int k = 0; k < d.nillum; ++k) {
        for (int i = 0; i < PRC_FUSE_ILLUM_DOUBLES; ++i)
            PRC_REQUIRE(isfinite(illum_host[k * PRC_FUSE_ILLUM_DOUBLES + i]), PRC_EINVAL, "prc_fuse: illuminator %d, parameter %d is not "
                        "finite", k, i);
        PRC_REQUIRE(illum_host[k * PRC_FUSE_ILLUM_DOUBLES + 3] > 0.0, PRC_EINVAL, "prc_fuse: illuminator %d: wavelength %g, not > 0", k,
                    illum_host[k * PRC_FUSE_ILLUM_DOUBLES + 3]);
    }
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_fuse: nframes = %d", nframes);
    PRC_REQUIRE(fuse_strides_ok((int64_t)d.H * d.W, d.nillum, illum_stride, std::max(nframes, 1), frame_stride), PRC_EINVAL,
                "prc_fuse: illum_stride = %lld, frame_stride = %lld let the %d x %d maps of %d x %d elements overlap",
                (long long)illum_stride, (long long)frame_stride, d.nillum, nframes, d.H, d.W);
    if (nframes == 0) return PRC_OK;
    PRC_REQUIRE(stat && best, PRC_EINVAL, "prc_fuse: null pointer");

    FuseArgs a;
    memset(&a, 0, sizeof(a));
    a.stat = stat; a.best = best; a.vel = vel;
    a.illum_stride = d.nillum > 1 ? illum_stride : 0;
    a.frame_stride = nframes > 1 ? frame_stride : 0;
    a.nframes = nframes;
    a.H = d.H; a.W = d.W; a.nx = d.nx; a.ny = d.ny; a.nvx = d.nvx; a.nvy = d.nvy; a.combine = d.combine;
    a.lds_floats = (PRC_FUSE_LDS_BYTES - HEAD_BYTES) / 4;
    a.x0 = d.x0; a.dx = d.dx; a.y0 = d.y0; a.dy = d.dy; a.z = d.z;
    a.vx0 = d.vx0; a.dvx = d.dvx; a.vy0 = d.vy0; a.dvy = d.dvy;
    for (int i = 0; i < 3; ++i) a.rx[i] = d.rx[i];
    memcpy(a.illum, illum_host, sizeof(double) * PRC_FUSE_ILLUM_DOUBLES * (size_t)d.nillum);
    a.tiles_x = (int)tx;
    // runs of frames: enough workgroups to fill the device, and the geometry is shared by the frames of a run
    int64_t runs = std::min<int64_t>(std::max<int64_t>((FUSE_TARGET_WGS + tiles - 1) / tiles, 1), nframes);
    a.fpr = (int)((nframes + runs - 1) / runs);
    runs = ((int64_t)nframes + a.fpr - 1) / a.fpr;   // <= FUSE_TARGET_WGS: inside gridDim.y
    switch (d.nillum) {
        case 1: return fuse_launch<1>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 2: return fuse_launch<2>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 3: return fuse_launch<3>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 4: return fuse_launch<4>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 5: return fuse_launch<5>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 6: return fuse_launch<6>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        case 7: return fuse_launch<7>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
        default: return fuse_launch<8>(a, lds, (unsigned)tiles, (unsigned)runs, (hipStream_t)stream);
    }
}
