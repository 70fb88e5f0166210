// Target tracking on device: get_measurements and multitarget_tracker (target_detection.py:164-537).
//
// prc_track_measure: one 1024-thread workgroup per frame.
//   pass 1   mean |v| over the whole frame (fp64);
//   pass 2-4 x(k) exactly by radix select on the masked values' order-preserving keys: histograms of the top 11 bits,
//            then of the next 11 / 10 among the keys that share the prefix found so far;
//   pass 5   (only when x(k+1) != x(k)) the smallest key above x(k);
//   pass 6   candidates v/mean >= threshold, collected into LDS as (key << 32 | flat index) and bitonic-sorted there.
// A frame with more candidates than fit LDS (a threshold on a run of ties: up to n) sorts in its own slice of the
// output array instead; one with more candidates than the plan's capacity first selects the top `capacity` of them
// (two more radix selects: strength, then flat index).  Division by the positive mean does not reorder float32
// values in fp64, so every select runs on the raw values and only x(k), x(k+1) and the outputs are normalised.
//
// prc_track_run: ONE wavefront walks every frame in order.  Phase A (association) is sequential over tracks in the
// order fixed at the start of the frame (confirmed, preliminary, free); each track gates the remaining candidates with
// lane-parallel compares and a 64-bit ballot, and removed candidates are masked (one bit each, in LDS), never
// compacted.  Phase B (Kalman and status updates) runs one lane per track.  fp64 throughout, 2x2 inverses in closed form.
#include "common.h"
#include "order_select.h"
#include "wave.h"

#include <math.h>

namespace {

constexpr int MT = 1024;           // threads per measure workgroup
constexpr int MW = MT / PRC_WAVE;  // wavefronts per measure workgroup
constexpr int NBINS = PRC_RADIX_BINS;
constexpr int LDS_CAP = 4096;      // candidates sorted in LDS
constexpr int LDS_ALIVE_CAPACITY = 1 << 19;   // up to here the tracker's alive bits (capacity / 64 words, 64 KiB) sit
                                              // in LDS; above, in a workspace of the plan

struct MeasureArgs {
    const float* frames;
    int H, W, n, capacity;
    uint32_t k;          // numpy's floor(q (n-1)) (n-1 above the last index)
    double t;            // its fraction
    double rstart, rstep, rstop, dstart, dstep, dstop;   // numpy 2.x linspace of range / Doppler coordinates
    int32_t* counts;
    prc_track_cand* cands;
};

// value of storage cell i = h*W + w after the reference's masks (fliplr(frame.T): range row w, Doppler column H-1-h)
// and its flat index w*H + (H-1-h) in that orientation
struct Cell {
    float v;
    uint32_t idx;
};
__device__ __forceinline__ Cell cell(const MeasureArgs& a, const float* x, int i) {
    const int h = i / a.W;
    const int w = i - h * a.W;
    const int c = a.H - 1 - h;
    const int c0 = a.H / 2;
    const bool masked = w < 8 || w >= a.W - 8 || (c >= c0 - 4 && c < c0 + 4);
    Cell r;
    r.v = masked ? 0.0f : x[i];
    r.idx = (uint32_t)(w * a.H + c);
    return r;
}

struct MeasureLds {
    uint32_t hist[NBINS];
    unsigned long long keys[LDS_CAP];
    double dred[MW];
    uint32_t ured[MW];
    uint32_t sel[4];
    uint32_t cnt;
};

// The rank-r (0-based, ascending) key among the cells where pred(cell, key) holds, by the digits of PrcKeys32.
// Returns the key; *less / *eq = how many participating keys lie below / equal it.
template <class Pred>
__device__ uint32_t block_select(MeasureLds& L, const MeasureArgs& a, const float* x, uint32_t r, Pred pred,
                                 uint32_t* less, uint32_t* eq) {
    uint32_t prefix = 0, pmask = 0, below = 0, in_bin = 0;
    for (int p = 0; p < PrcKeys32::passes; ++p) {
        const int shift = PrcKeys32::shift(p), width = PrcKeys32::width(p);
        const uint32_t dm = (1u << width) - 1u;
        for (int b = threadIdx.x; b < NBINS; b += MT) L.hist[b] = 0u;
        __syncthreads();
        for (int i = threadIdx.x; i < a.n; i += MT) {
            const Cell c = cell(a, x, i);
            uint32_t key;
            if (pred(c, &key) && (key & pmask) == prefix) atomicAdd(&L.hist[(key >> shift) & dm], 1u);
        }
        __syncthreads();
        prc_resolve_digit(L.hist, 1 << width, r, L.ured, L.sel);
        const uint32_t bin = L.sel[0], bef = L.sel[1];
        in_bin = L.sel[2];
        __syncthreads();
        prefix |= bin << shift;
        pmask |= dm << shift;
        r -= bef;
        below += bef;
    }
    *less = below;
    *eq = in_bin;
    return prefix;
}

__device__ __forceinline__ double coord(uint32_t i, uint32_t last, double start, double step, double stop) {
    // numpy 2.x linspace: arange * step + start (two roundings, no FMA), the last point set to stop
    return i == last ? stop : __dadd_rn(__dmul_rn((double)i, step), start);
}

__device__ __forceinline__ prc_track_cand make_cand(const MeasureArgs& a, unsigned long long key, double mean) {
    const uint32_t idx = (uint32_t)(key & 0xffffffffull);
    const float v = prc_key_value((uint32_t)(key >> 32));
    const uint32_t r = idx / (uint32_t)a.H, c = idx - r * (uint32_t)a.H;
    prc_track_cand o;
    o.strength = (double)v / mean;
    o.range = coord(r, a.W - 1, a.rstart, a.rstep, a.rstop);
    o.doppler = coord(c, a.H - 1, a.dstart, a.dstep, a.dstop);
    o.index = idx;
    return o;
}

__global__ __launch_bounds__(MT) void track_measure_kernel(MeasureArgs a) {
    __shared__ MeasureLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = blockIdx.x;
    const float* x = a.frames + (size_t)f * (size_t)a.n;
    prc_track_cand* out = a.cands + (size_t)f * (size_t)a.capacity;

    // ---- mean |v| over the whole frame (before masking), fp64 ----
    double s = 0.0;
    for (int i = tid; i < a.n; i += MT) s += fabs((double)x[i]);
    s = wave_sum(s);
    if (lane == 0) L.dred[wv] = s;
    if (tid == 0) L.cnt = 0u;
    __syncthreads();
    double sum = 0.0;
    for (int q = 0; q < MW; ++q) sum += L.dred[q];
    const double mean = sum / (double)a.n;
    if (!(mean > 0.0) || isinf(mean)) {          // NaN / Inf in the frame, or all zeros: no candidates
        if (tid == 0) a.counts[f] = 0;
        return;
    }

    // ---- threshold: x(k), x(k+1) exactly, then numpy's _lerp ----
    auto all = [](const Cell& c, uint32_t* key) { *key = prc_okey(c.v); return true; };
    uint32_t less, eq;
    const uint32_t ka = block_select(L, a, x, a.k, all, &less, &eq);
    const uint32_t k1 = a.k + 1 < (uint32_t)a.n ? a.k + 1 : a.k;
    uint32_t kb = ka;
    if (k1 != a.k && less + eq <= k1) {          // x(k+1) is the smallest key above x(k)
        uint32_t m = 0xffffffffu;
        for (int i = tid; i < a.n; i += MT) {
            const uint32_t key = prc_okey(cell(a, x, i).v);
            if (key > ka) m = min(m, key);
        }
        m = wave_min(m);
        if (lane == 0) L.ured[wv] = m;
        __syncthreads();
        kb = 0xffffffffu;
        for (int q = 0; q < MW; ++q) kb = min(kb, L.ured[q]);
        __syncthreads();
    }
    const double xa = (double)prc_key_value(ka) / mean, xb = (double)prc_key_value(kb) / mean;
    const double thr = prc_np_lerp(xa, xb, a.t);

    // ---- candidates: count them, keep the first LDS_CAP keys ----
    auto is_cand = [mean, thr](const Cell& c) { return (double)c.v / mean >= thr; };
    for (int i = tid; i < a.n; i += MT) {
        const Cell c = cell(a, x, i);
        if (is_cand(c)) {
            const uint32_t pos = atomicAdd(&L.cnt, 1u);
            if (pos < (uint32_t)LDS_CAP) L.keys[pos] = ((unsigned long long)prc_okey(c.v) << 32) | c.idx;
        }
    }
    __syncthreads();
    const uint32_t count = L.cnt;
    __syncthreads();        // every wavefront has read the counter before any path below resets it
    if (tid == 0) a.counts[f] = (int32_t)count;
    const uint32_t m = count < (uint32_t)a.capacity ? count : (uint32_t)a.capacity;
    if (m == 0) return;

    const bool need_cut = count > (uint32_t)a.capacity;
    const bool in_lds = m <= (uint32_t)LDS_CAP;
    if (need_cut || !in_lds) {
        // the top m in (strength, flat index) order: select the cut-off key, then the cut-off index among its ties
        uint32_t kv = 0, ki = 0;
        if (need_cut) {
            const uint32_t rank = count - m;     // ascending rank of the smallest kept candidate
            auto cand_key = [&](const Cell& c, uint32_t* key) { *key = prc_okey(c.v); return is_cand(c); };
            uint32_t lv, ev;
            kv = block_select(L, a, x, rank, cand_key, &lv, &ev);
            auto tie_idx = [&](const Cell& c, uint32_t* key) { *key = c.idx; return is_cand(c) && prc_okey(c.v) == kv; };
            uint32_t li, ei;
            ki = block_select(L, a, x, rank - lv, tie_idx, &li, &ei);
        }
        unsigned long long* dst = in_lds ? L.keys : reinterpret_cast<unsigned long long*>(out);
        if (tid == 0) L.cnt = 0u;
        __syncthreads();
        for (int i = tid; i < a.n; i += MT) {
            const Cell c = cell(a, x, i);
            if (!is_cand(c)) continue;
            const uint32_t key = prc_okey(c.v);
            if (need_cut && !(key > kv || (key == kv && c.idx >= ki))) continue;
            const uint32_t pos = atomicAdd(&L.cnt, 1u);
            if (pos < m) dst[pos] = ((unsigned long long)key << 32) | c.idx;
        }
        __syncthreads();
    }

    int P = 1;
    while (P < (int)m) P <<= 1;
    if (in_lds) {
        for (int i = (int)m + tid; i < P; i += MT) L.keys[i] = 0ull;   // real keys are > 0: padding sorts last
        __syncthreads();
        prc_bitonic<MT, false, true>(L.keys, nullptr, (uint32_t)P);
        for (int i = tid; i < (int)m; i += MT) out[i] = make_cand(a, L.keys[i], mean);
        return;
    }
    // oversize: keys sorted in this frame's own slice of the output (P * 8 < 2 m * 8 <= capacity * 32 bytes), then
    // expanded in place from the top down: record i overwrites keys 4i .. 4i+3, all >= i, already read
    unsigned long long* g = reinterpret_cast<unsigned long long*>(out);
    for (int i = (int)m + tid; i < P; i += MT) g[i] = 0ull;
    __threadfence();
    __syncthreads();
    prc_bitonic<MT, true, true>(g, nullptr, (uint32_t)P);
    for (int base = (((int)m - 1) / MT) * MT; base >= 0; base -= MT) {
        const int i = base + tid;
        const unsigned long long key = i < (int)m ? g[i] : 0ull;
        __threadfence();
        __syncthreads();
        if (i < (int)m) out[i] = make_cand(a, key, mean);
        __threadfence();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// tracker
__constant__ double kF1[16] = {1, 0, -0.003, 0, 0, 0, -0.003, -0.003, 0, 0, 1, 1, 0, 0, 0, 1};
__constant__ double kF2[16] = {1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1};
__constant__ double kQ[4] = {4.0, 0.03, 0.2, 0.08};
__constant__ double kP0[4] = {5.0, 0.0225, 0.04, 0.1};
constexpr uint32_t kHist0 = 0x3e1u;     // initialize_track: hist[0] = 1, hist[5:10] = 1
constexpr uint32_t kHistMask = 0xfffffu;

struct Track {
    int status, life;
    uint32_t hist;            // bit i = measurement_history[i]
    double mr, md, er, ed;    // last measurement / estimate
    double x[4], P[16], S[4];
};

__device__ void track_init(Track& t, int status, double r, double f) {
    // initialize_track (:333-387): its swapped (estimate, measurement) tuple order is harmless, both hold [r, f]
    t.status = status;
    t.life = 1;
    t.hist = kHist0;
    t.mr = t.er = r;
    t.md = t.ed = f;
    t.x[0] = r; t.x[1] = 0.0; t.x[2] = f; t.x[3] = -1.0;
    for (int i = 0; i < 16; ++i) t.P[i] = (i % 5 == 0) ? kP0[i / 5] : 0.0;
    t.S[0] = 1.0; t.S[1] = 0.0; t.S[2] = 0.0; t.S[3] = 1.0;
}

__device__ __forceinline__ void inv2(const double* S, double* Si) {
    const double det = S[0] * S[3] - S[1] * S[2];
    Si[0] = S[3] / det; Si[1] = -S[1] / det; Si[2] = -S[2] / det; Si[3] = S[0] / det;
}

// update_track (:389-453) with a measurement (got) or without
__device__ void track_update(Track& t, bool got, double zr, double zd) {
    double x[4], FP[16], P[16];
    for (int i = 0; i < 4; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 4; ++j) acc += kF1[4 * i + j] * t.x[j];
        x[i] = acc;
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += kF2[4 * i + q] * t.P[4 * q + j];
            FP[4 * i + j] = acc;
        }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            for (int q = 0; q < 4; ++q) acc += FP[4 * i + q] * kF2[4 * j + q];
            P[4 * i + j] = acc + (i == j ? kQ[i] : 0.0);
        }
    // S = H P H^T + R * scale; H picks state components 0 and 2
    const double scale = got ? (zr - t.mr) * (zr - t.mr) + (zd - t.md) * (zd - t.md) : 1.0;   // adaptive R
    double S[4] = {P[0] + 5.0 * scale, P[2], P[8], P[10] + 2.0 * scale};
    if (got) {
        double Si[4], K[8];
        inv2(S, Si);
        for (int i = 0; i < 4; ++i) {           // K = P H^T S^-1
            K[2 * i] = P[4 * i] * Si[0] + P[4 * i + 2] * Si[2];
            K[2 * i + 1] = P[4 * i] * Si[1] + P[4 * i + 2] * Si[3];
        }
        const double y0 = zr - x[0], y1 = zd - x[2];
        for (int i = 0; i < 4; ++i) x[i] += K[2 * i] * y0 + K[2 * i + 1] * y1;
        double NP[16];                          // (I - K H) P
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                NP[4 * i + j] = P[4 * i + j] - (K[2 * i] * P[j] + K[2 * i + 1] * P[8 + j]);
        for (int i = 0; i < 16; ++i) P[i] = NP[i];
        t.mr = zr;
        t.md = zd;
    }   // else: extrapolate and keep the last measurement (intentional, as the reference)
    for (int i = 0; i < 4; ++i) t.x[i] = x[i];
    for (int i = 0; i < 16; ++i) t.P[i] = P[i];
    for (int i = 0; i < 4; ++i) t.S[i] = S[i];
    t.er = x[0];
    t.ed = x[2];
    // kill / promote read the history from BEFORE its shift (intentional, as the reference)
    const int s10 = __popc(t.hist & 0x3ffu), s20 = __popc(t.hist & kHistMask);
    if (t.status == 1) {
        if (t.life > 4 && s10 < 6) t.status = 0;
        if (t.life > 4 && s10 > 8) t.status = 2;
    } else if (t.status == 2) {
        if (t.life > 4 && s20 < 4) t.status = 0;
    }
    t.hist = ((t.hist << 1) | (got ? 1u : 0u)) & kHistMask;
    t.life += 1;
}

__device__ __forceinline__ double bcast(double v, int src) { return __shfl(v, src, PRC_WAVE); }

struct Assoc {
    bool got;
    double r, d;
};

// associate_measurements (:231-331) for one track, uniform over the wavefront.  alive: one bit per candidate.
__device__ Assoc associate(int status, double mr, double md, double er, double ed, const double* S,
                           const prc_track_cand* C, int m, unsigned long long* alive, int words, int* nalive) {
    const int lane = threadIdx.x;
    Assoc res{false, 0.0, 0.0};
    double Si[4];
    if (status == 2) inv2(S, Si);
    int jbest = -1;
    if (status == 0) {
        // free track: the overall strongest remaining candidate (intentional, as the reference)
        for (int w = 0; w < words && jbest < 0; ++w)
            if (alive[w]) jbest = w * 64 + __ffsll((long long)alive[w]) - 1;
    } else if (status == 1) {
        // preliminary: argmin sqrt(r^2 + d^2) over the gated candidates -- the ABSOLUTE norm, not the distance to the
        // track (intentional, as the reference); ties go to the first occurrence
        double best = INFINITY;
        int bi = 0x7fffffff;
        for (int w = 0; w < words; ++w) {
            const int j = w * 64 + lane;
            if (j < m && ((alive[w] >> lane) & 1ull)) {
                const double r = C[j].range, d = C[j].doppler;
                if (fabs(r - mr) < 5.0 && fabs(d - md) < 24.0) {
                    const double nrm = sqrt(__dadd_rn(__dmul_rn(r, r), __dmul_rn(d, d)));
                    if (nrm < best) { best = nrm; bi = j; }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, PRC_WAVE);
            const int oi = __shfl_xor(bi, o, PRC_WAVE);
            if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (bi != 0x7fffffff) jbest = bi;
    } else {
        // confirmed: early gate on the last ESTIMATE (4 km, 20 Hz), Mahalanobis gate (< 6) with the last MEASUREMENT
        // and the stored S, the strongest validated candidate (intentional, as the reference)
        for (int w = 0; w < words && jbest < 0; ++w) {
            const int j = w * 64 + lane;
            bool v = false;
            if (j < m && ((alive[w] >> lane) & 1ull)) {
                const double r = C[j].range, d = C[j].doppler;
                if (fabs(r - er) < 4.0 && fabs(d - ed) < 20.0) {
                    const double z0 = mr - r, z1 = md - d;
                    const double u0 = __dadd_rn(__dmul_rn(z0, Si[0]), __dmul_rn(z1, Si[2]));
                    const double u1 = __dadd_rn(__dmul_rn(z0, Si[1]), __dmul_rn(z1, Si[3]));
                    v = __dadd_rn(__dmul_rn(u0, z0), __dmul_rn(u1, z1)) < 6.0;
                }
            }
            const unsigned long long b = __ballot(v);
            if (b) jbest = w * 64 + __ffsll((long long)b) - 1;
        }
    }
    if (jbest < 0) return res;                   // nothing found: the candidate list is left unchanged
    res.got = true;
    res.r = C[jbest].range;
    res.d = C[jbest].doppler;
    // remove: free -> |dr| < 10 and |dd| < 12 around the chosen one (all of them when it was the only one);
    // preliminary -> its gate; confirmed -> its EARLY gate, not the validation gate (intentional, as the reference)
    const bool single = status == 0 && *nalive == 1;
    int removed = 0;
    for (int w = 0; w < words; ++w) {
        const int j = w * 64 + lane;
        bool g = false;
        if (j < m && ((alive[w] >> lane) & 1ull)) {
            const double r = C[j].range, d = C[j].doppler;
            if (status == 0) g = single || (fabs(r - res.r) < 10.0 && fabs(d - res.d) < 12.0);
            else if (status == 1) g = fabs(r - mr) < 5.0 && fabs(d - md) < 24.0;
            else g = fabs(r - er) < 4.0 && fabs(d - ed) < 20.0;
        }
        const unsigned long long b = __ballot(g);
        removed += __popcll(b);
        __syncthreads();
        if (lane == 0) alive[w] &= ~b;
        __syncthreads();
    }
    *nalive -= removed;
    return res;
}

template <bool GlobalAlive>
__global__ __launch_bounds__(PRC_WAVE) void track_run_kernel(const int32_t* counts, const prc_track_cand* cands,
                                                              int nframes, int capacity, int ntracks,
                                                              prc_track_record* records, unsigned long long* alive_ws) {
    extern __shared__ unsigned long long alive_lds[];
    unsigned long long* alive = GlobalAlive ? alive_ws : alive_lds;
    const int lane = threadIdx.x;
    const bool mine = lane < ntracks;
    Track t;
    track_init(t, 0, 0.0, 0.0);
    for (int f = 0; f < nframes; ++f) {
        const int cnt = counts[f];
        const int m = cnt < capacity ? cnt : capacity;
        const prc_track_cand* C = cands + (size_t)f * (size_t)capacity;
        const int mw = (m + 63) / 64;
        for (int w = lane; w < mw; w += PRC_WAVE) {
            const int left = m - w * 64;
            alive[w] = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
        }
        __syncthreads();
        int nalive = m;
        // phase A: the order is fixed at the start of the frame: confirmed, preliminary, free, each in index order
        const unsigned long long conf = __ballot(mine && t.status == 2);
        const unsigned long long pre = __ballot(mine && t.status == 1);
        const unsigned long long fre = __ballot(mine && t.status == 0);
        bool touched = false, got = false;
        double zr = 0.0, zd = 0.0;
        for (int pass = 0; pass < 3; ++pass) {
            unsigned long long set = pass == 0 ? conf : (pass == 1 ? pre : fre);
            const int st = 2 - pass;
            while (set) {
                const int i = __ffsll((long long)set) - 1;
                set &= set - 1;
                // free tracks: when the candidates run out the loop `break`s -- the free tracks left are not touched
                // and do not age (intentional, as the reference)
                if (st == 0 && nalive == 0) break;
                const double S[4] = {bcast(t.S[0], i), bcast(t.S[1], i), bcast(t.S[2], i), bcast(t.S[3], i)};
                const Assoc as = associate(st, bcast(t.mr, i), bcast(t.md, i), bcast(t.er, i), bcast(t.ed, i), S, C, m,
                                           alive, mw, &nalive);
                if (lane == i) { touched = true; got = as.got; zr = as.r; zd = as.d; }
            }
        }
        // phase B: one lane per track; no update depends on another track's update within the frame
        if (mine && touched) {
            if (t.status == 0) track_init(t, 1, zr, zd);
            else track_update(t, got, zr, zd);
        }
        if (mine) {
            prc_track_record* o = records + (size_t)f * (size_t)ntracks + lane;
            o->status = t.status;
            o->lifetime = t.life;
            o->measurement[0] = t.mr; o->measurement[1] = t.md;
            o->estimate[0] = t.er; o->estimate[1] = t.ed;
            for (int i = 0; i < 4; ++i) o->x[i] = t.x[i];
            for (int i = 0; i < 16; ++i) o->P[i] = t.P[i];
            for (int i = 0; i < 4; ++i) o->S[i] = t.S[i];
            for (int i = 0; i < 20; ++i) o->history[i] = (uint8_t)((t.hist >> i) & 1u);
            o->overflow = cnt > capacity ? 1 : 0;
        }
        __syncthreads();
    }
}

}  // namespace

struct prc_track_plan {
    prc_track_desc d;
    std::mutex mu;
    unsigned long long* alive = nullptr;   // the tracker's alive bits when capacity > LDS_ALIVE_CAPACITY
};

extern "C" int prc_track_plan_create(prc_track_plan** plan, const prc_track_desc* desc) {
    PRC_REQUIRE(plan && desc, PRC_EINVAL, "prc_track_plan_create: null argument");
    prc_track_desc d;
    int rc = prc_take_desc(&d, desc, PRC_TRACK_DESC_SIZE_610, "prc_track_plan_create", "prc_track_desc");
    if (rc != PRC_OK) return rc;
    PRC_REQUIRE(d.H >= 8 && d.W >= 17, PRC_EINVAL,
                "prc_track_plan_create: H = %d, W = %d: the reference's masks need H >= 8 and W >= 17", d.H, d.W);
    PRC_REQUIRE((int64_t)d.H * d.W <= (int64_t)0x7fffffff, PRC_EINVAL, "prc_track_plan_create: H * W too large");
    PRC_REQUIRE(d.ntracks >= 1 && d.ntracks <= 64, PRC_EINVAL, "prc_track_plan_create: ntracks = %d, not 1 .. 64",
                d.ntracks);
    PRC_REQUIRE(d.capacity >= 1, PRC_EINVAL, "prc_track_plan_create: capacity = %d, not >= 1", d.capacity);
    PRC_REQUIRE(d.percentile >= 0.0 && d.percentile <= 100.0, PRC_EINVAL,
                "prc_track_plan_create: percentile = %g, not in [0, 100]", d.percentile);
    PRC_REQUIRE(isfinite(d.doppler_extent) && isfinite(d.range_extent), PRC_EINVAL,
                "prc_track_plan_create: extents must be finite");
    void* ws = nullptr;
    if (d.capacity > LDS_ALIVE_CAPACITY) PRC_HIP(hipMalloc(&ws, (size_t)((d.capacity + 63) / 64) * 8));
    prc_track_plan* p = new prc_track_plan();
    p->d = d;
    p->alive = (unsigned long long*)ws;
    *plan = p;
    return PRC_OK;
}

extern "C" int prc_track_plan_destroy(prc_track_plan* plan) {
    if (plan && plan->alive) PRC_HIP(hipFree(plan->alive));
    delete plan;
    return PRC_OK;
}

extern "C" int prc_track_measure(prc_track_plan* plan, const float* frames, int32_t nframes, int32_t* counts,
                                 prc_track_cand* cands, void* stream) {
    PRC_RANGE("prc_track_measure");
    PRC_REQUIRE(plan && frames && counts && cands, PRC_EINVAL, "prc_track_measure: null argument");
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_track_measure: nframes = %d", nframes);
    if (nframes == 0) return PRC_OK;
    std::lock_guard<std::mutex> g(plan->mu);
    const prc_track_desc& d = plan->d;
    MeasureArgs a;
    a.frames = frames;
    a.H = d.H;
    a.W = d.W;
    a.n = d.H * d.W;
    a.capacity = d.capacity;
    prc_percentile_rank(d.percentile, (uint32_t)a.n, &a.k, &a.t);
    // rpts = np.linspace(R, 0, W), dpts = np.linspace(-D, D, H) (:196-197): step = (stop - start) / (num - 1)
    a.rstart = d.range_extent;
    a.rstop = 0.0;
    a.rstep = (0.0 - d.range_extent) / (double)(d.W - 1);
    a.dstart = -1.0 * d.doppler_extent;
    a.dstop = d.doppler_extent;
    a.dstep = (d.doppler_extent - a.dstart) / (double)(d.H - 1);
    a.counts = counts;
    a.cands = cands;
    hipLaunchKernelGGL(track_measure_kernel, dim3(nframes), dim3(MT), 0, (hipStream_t)stream, a);
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}

extern "C" int prc_track_run(prc_track_plan* plan, const int32_t* counts, const prc_track_cand* cands, int32_t nframes,
                             prc_track_record* records, void* stream) {
    PRC_RANGE("prc_track_run");
    PRC_REQUIRE(plan && counts && cands && records, PRC_EINVAL, "prc_track_run: null argument");
    PRC_REQUIRE(nframes >= 0, PRC_EINVAL, "prc_track_run: nframes = %d", nframes);
    if (nframes == 0) return PRC_OK;
    std::lock_guard<std::mutex> g(plan->mu);
    if (plan->alive) {
        hipLaunchKernelGGL(track_run_kernel<true>, dim3(1), dim3(PRC_WAVE), 0, (hipStream_t)stream, counts, cands,
                           nframes, plan->d.capacity, plan->d.ntracks, records, plan->alive);
    } else {
        const int words = (plan->d.capacity + 63) / 64;
        hipLaunchKernelGGL(track_run_kernel<false>, dim3(1), dim3(PRC_WAVE), (size_t)words * 8, (hipStream_t)stream,
                           counts, cands, nframes, plan->d.capacity, plan->d.ntracks, records, nullptr);
    }
    PRC_LAUNCH_CHECK();
    return PRC_OK;
}
