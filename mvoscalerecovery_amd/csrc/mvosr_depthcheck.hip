// mvosr_depthcheck.hip — the reference's pairwise depth-order check (depth_check, /root/reference/script/data_check.py:19-34) on
// the device: over a frame's points below the camera (y > 0), for EVERY ordered pair (i, j), the diagonal included,
//     q = (z_j - z_i) / ((y_j / z_j - y_i / z_i) + 0.000001)                                                        (:23-28)
// and of the n x n values the histogram over np.array(range(-40, 20)) * 50 (:30-31), what lies outside it, and np.max (:32).
//
// A feature carries one level as in mvosr_featdist.hip (0 below the vanishing row, 1 also kept by the vote, 2 also selected); a pair
// belongs to population p iff min(level_i, level_j) >= p, so one pass over the pairs of population 0 serves all three.
//
// The work is n^2 per frame and n is ragged, so a frame spans many workgroups (mvosr_depthcheck_plan.hpp): a workgroup keeps a
// row block of 256 points in registers, one a thread, and streams its share of the frame's j tiles through LDS; every lane reads
// the same j, so the tile reads are broadcasts.  The division is IEEE (the file is built with -ffp-contract=off: every operation
// below is an operation of its own), the bin is decided against the integer edges (depthcheck_slot).
//
// The hot spot is the histogram update: a lane produces one of 3 x 62 words and most lanes of a wavefront meet in a few of them.
// The LDS histogram is striped: kDcCopies copies, the copy index fastest, a lane adds to copy lane % kDcCopies — at most two lanes of
// a wavefront add to one word, and the lanes of one bin spread over the banks (LABNOTES has the A/B against per-wave copies and
// ballot counting).
//
// Accumulation is by integer atomics only — LDS u32, then one global 64-bit add per non-zero word and workgroup; the maximum travels
// as an order-preserving integer key through a 64-bit atomic max over the non-NaN values.  The result does not depend on the order of
// arrival.  Three launches on the context's stream: dc_zero_kernel clears the frames' outputs, depthcheck_kernel adds per LEVEL,
// dc_finish_kernel turns levels into populations (p: the levels >= p), keys into doubles, writes the status and adds the frame
// to the sequence tables.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_depthcheck_plan.hpp"

namespace mvosr {

static_assert(kDcBins == MVOSR_DC_BINS && kDcSlots == MVOSR_DC_TABLE_WORDS && kDcPops == MVOSR_FD_POPULATIONS, "mvosr.h");
static_assert(kDcRows % kWave == 0 && kDcTile % kDcRows == 0 && kWave % kDcCopies == 0, "the tile is loaded by whole passes of the block");
constexpr int kDcUnselected = 255;            // the level of a thread whose i is no point of population 0
constexpr int kDcFinishBlock = 192;           // one thread per (population, word) of a frame: 186
static_assert(kDcFinishBlock >= kDcPops * kDcSlots, "dc_finish_kernel");

struct DepthCheckArgs {
    int64_t n_frames;
    const int64_t *off; const int32_t *cnt;   // cnt == nullptr: off has n_frames + 1 entries
    const double *y, *z; const uint8_t *level;
    int32_t max_feat, j_split;
    unsigned long long *hist;                 // [F][3][59]
    unsigned long long *below, *above, *nan;  // [F][3]
    unsigned long long *max_key;              // [F][3]: the output `max`, holding keys until dc_finish_kernel
    unsigned long long *n;                    // [F][3]
    int32_t *status;                          // [F]
    unsigned long long *tables;               // optional [3][62], added to
};

// a double's pattern, made to order like the double (negative values: all bits flipped; others: the sign bit set), and back; no key
// of a number is 0
__device__ __forceinline__ unsigned long long dc_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double dc_unkey(unsigned long long k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
}

// a frame the launch's grid was not sized for, or that no launch of this library describes, is refused before anything of it is read
__device__ __forceinline__ bool dc_frame(const DepthCheckArgs &a, int64_t f, int64_t &base, int64_t &len) {
    base = a.off[f];
    len = a.cnt ? (int64_t)a.cnt[f] : a.off[f + 1] - base;
    return base >= 0 && len >= 0 && len <= (int64_t)a.max_feat;
}

// where word `slot` of (frame, level or population) lives
__device__ __forceinline__ unsigned long long *dc_word(const DepthCheckArgs &a, int64_t row, int slot) {
    if (slot < kDcBins) return a.hist + row * kDcBins + slot;
    return (slot == kDcBelow ? a.below : slot == kDcAbove ? a.above : a.nan) + row;
}

__global__ __launch_bounds__(kDcFinishBlock) void dc_zero_kernel(const DepthCheckArgs a) {
    const int64_t f = blockIdx.x;
    const int t = threadIdx.x;
    if (t < kDcPops * kDcSlots) *dc_word(a, f * kDcPops + t / kDcSlots, t % kDcSlots) = 0ull;
    if (t < kDcPops) { a.max_key[f * kDcPops + t] = 0ull; a.n[f * kDcPops + t] = 0ull; }
    if (t == 0) a.status[f] = 0;
}

// One pair into the workgroup's LDS histogram, striped: copy lane % kDcCopies, the copy index fastest — two lanes a word at most,
// one bin's lanes over all banks.  word < 0: none (a lane without a point).
__device__ __forceinline__ void dc_count(unsigned int *hist, int word) {
    if (word >= 0) atomicAdd(&hist[word * kDcCopies + (lane_id() & (kDcCopies - 1))], 1u);
}

__global__ __launch_bounds__(kDcRows) void depthcheck_kernel(const DepthCheckArgs a) {
    __shared__ double tile_z[kDcTile], tile_v[kDcTile];
    __shared__ int tile_l[kDcTile];
    __shared__ unsigned int hist[kDcPops * kDcSlots * kDcCopies];
    __shared__ int tile_n;
    const int64_t f = blockIdx.x;
    const int rb = (int)blockIdx.y / a.j_split, js = (int)blockIdx.y - rb * a.j_split;
    const int tid = threadIdx.x, lane = lane_id();
    int64_t base, len;
    if (!dc_frame(a, f, base, len) || (int64_t)rb * kDcRows >= len) return;          // (uniform: the whole workgroup leaves)
    const double *Y = a.y + base, *Z = a.z + base;
    const uint8_t *LV = a.level + base;

    for (int k = tid; k < kDcPops * kDcSlots * kDcCopies; k += kDcRows) hist[k] = 0u;

    // ---- the i side: one point a thread
    const int64_t i = (int64_t)rb * kDcRows + tid;
    int lvi = kDcUnselected;
    double zi = 0.0, vi = 0.0;
    if (i < len) {
        const int lv = (int)LV[i];
        const double y = Y[i];
        if (lv > 2) {
            if (js == 0) atomicOr(&a.status[f], 1);                                  // dc_finish_kernel refuses the frame
        } else if (y > 0.0) {                                                        // :20 (a NaN y: not selected)
            lvi = lv;
            zi = Z[i];                                                               // :21
            vi = y / zi;                                                             // :23
        }
    }
    const bool sel_i = lvi != kDcUnselected;
    if (js == 0) {
        for (int m = 0; m < kDcPops; ++m) {
            const int c = __popcll(__ballot(lvi == m));
            if (lane == 0 && c) atomicAdd(&a.n[f * kDcPops + m], (unsigned long long)c);
        }
    }
    const bool wave_has_i = __ballot(sel_i) != 0ull;
    const double ninf = __longlong_as_double((long long)0xFFF0000000000000ull);
    double mx0 = ninf, mx1 = ninf, mx2 = ninf;                                       // of the pairs of level >= 0, 1, 2 (fmax skips a NaN)

    // ---- the j side: this workgroup's tiles through LDS, the selected points only (in any order: counts and maxima do not care)
    for (int64_t t0 = (int64_t)js * kDcTile; t0 < len; t0 += (int64_t)a.j_split * kDcTile) {
        __syncthreads();
        if (tid == 0) tile_n = 0;
        __syncthreads();
        for (int k = tid; k < kDcTile; k += kDcRows) {
            const int64_t j = t0 + k;
            int lj = 0;
            double zj = 0.0, vj = 0.0;
            bool sel_j = false;
            if (j < len) {
                lj = (int)LV[j];
                const double y = Y[j];
                sel_j = lj <= 2 && y > 0.0;
                if (sel_j) { zj = Z[j]; vj = y / zj; }
            }
            const unsigned long long mask = __ballot(sel_j);
            int at = 0;
            if (lane == 0 && mask) at = atomicAdd(&tile_n, __popcll(mask));
            at = __shfl(at, 0) + __popcll(mask & ((1ull << lane) - 1ull));
            if (sel_j) { tile_z[at] = zj; tile_v[at] = vj; tile_l[at] = lj; }
        }
        __syncthreads();
        const int kn = tile_n;
        if (wave_has_i) {
#pragma unroll 4
            for (int k = 0; k < kn; ++k) {
                const int lj = tile_l[k];
                const double d_minus = tile_z[k] - zi;                               // :27
                const double v_minus = tile_v[k] - vi;                               // :26
                const double q = d_minus / (v_minus + 0.000001);                     // :28
                const int m = lvi < lj ? lvi : lj;
                dc_count(hist, sel_i ? m * kDcSlots + depthcheck_slot(q) : -1);
                mx0 = fmax(mx0, q);
                mx1 = fmax(mx1, m >= 1 ? q : ninf);
                mx2 = fmax(mx2, m >= 2 ? q : ninf);
            }
        }
    }
    __syncthreads();

    // ---- flush: the copies summed (thread t starts at copy t: 32 threads, 32 banks), one 64-bit add per non-zero word
    if (tid < kDcPops * kDcSlots) {
        unsigned long long s = 0ull;
        for (int c = 0; c < kDcCopies; ++c) s += hist[tid * kDcCopies + ((c + tid) & (kDcCopies - 1))];
        if (s) atomicAdd(dc_word(a, f * kDcPops + tid / kDcSlots, tid % kDcSlots), s);
    }
    // the maxima of the wave's non-NaN values by key; -inf, the start, is below every value: a population that has pairs and no NaN
    // has a value of its own, every other population's maximum is NaN whatever is here
    if (wave_has_i) {
        unsigned long long key[kDcPops] = {dc_key(sel_i ? mx0 : ninf), dc_key(sel_i ? mx1 : ninf), dc_key(sel_i ? mx2 : ninf)};
        for (int m = 0; m < kDcPops; ++m) {
            unsigned long long k = key[m];
            for (int s = 1; s < kWave; s <<= 1) {
                const unsigned long long o = __shfl_xor(k, s);
                k = o > k ? o : k;
            }
            if (lane == 0) atomicMax(&a.max_key[f * kDcPops + m], k);
        }
    }
}

// levels -> populations, keys -> doubles, the status, the sequence tables.  One workgroup a frame, after depthcheck_kernel.
__global__ __launch_bounds__(kDcFinishBlock) void dc_finish_kernel(const DepthCheckArgs a) {
    const int64_t f = blockIdx.x;
    const int t = threadIdx.x, p = t / kDcSlots, slot = t % kDcSlots;
    int64_t base, len;
    const bool refused = !dc_frame(a, f, base, len) || a.status[f] != 0;
    const bool word = t < kDcPops * kDcSlots;
    unsigned long long v = 0ull, n = 0ull, nan = 0ull, key = 0ull, n0 = 0ull;
    if (word) for (int m = p; m < kDcPops; ++m) v += *dc_word(a, f * kDcPops + m, slot);
    if (t < kDcPops) {
        for (int m = t; m < kDcPops; ++m) {
            n += a.n[f * kDcPops + m];
            nan += a.nan[f * kDcPops + m];
            const unsigned long long k = a.max_key[f * kDcPops + m];
            key = k > key ? k : key;
        }
        for (int m = 0; m < kDcPops; ++m) n0 += a.n[f * kDcPops + m];
    }
    __syncthreads();                                                                 // every level is read before a population is written
    if (word) {
        if (refused) v = 0ull;
        *dc_word(a, f * kDcPops + p, slot) = v;
        if (a.tables && v) atomicAdd(&a.tables[p * kDcSlots + slot], v);
    }
    if (t < kDcPops) {
        if (refused) n = 0ull;
        a.n[f * kDcPops + t] = n;
        // np.max (:32): NaN where a pair is NaN — or where there is no pair —, else the largest value; a zero maximum is +0.0, the
        // diagonal's own value
        double mx = __longlong_as_double(0x7FF8000000000000ll);
        if (n > 0ull && nan == 0ull && key != 0ull) {
            mx = dc_unkey(key);
            if (mx == 0.0) mx = 0.0;
        }
        reinterpret_cast<double *>(a.max_key)[f * kDcPops + t] = mx;
        if (t == 0) a.status[f] = refused ? MVOSR_ST_ERR_MASK : (n0 == 0ull ? MVOSR_ST_DC_NO_POINT : 0);
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_depth_check_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *off, const int32_t *cnt, const double *y,
                                       const double *z, const uint8_t *level, const mvosr_depth_check_params *params,
                                       const mvosr_depth_check_outputs *o, int64_t *tables) {
    if (!ctx || !off || !y || !z || !level || !params || !o || !o->hist || !o->below || !o->above || !o->nan || !o->max || !o->n || !o->status)
        return set_error(MVOSR_ERR_ARG, "depth_check: null argument");
    if (params->max_feat < 0) return set_error(MVOSR_ERR_ARG, "depth_check: max_feat < 0");
    if (n_frames <= 0) return MVOSR_OK;
    if (n_frames > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "depth_check: more than 2^31-1 frames in one launch");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    const DepthCheckGrid g = depthcheck_grid(n_frames, (int64_t)params->max_feat, (int64_t)ctx->n_cu);
    if (g.row_blocks * g.j_split > 65535)
        return set_error(MVOSR_ERR_TOO_LARGE, "depth_check: a frame of %d features needs more than 65535 workgroups", params->max_feat);
    DepthCheckArgs a = {};
    a.n_frames = n_frames; a.off = off; a.cnt = cnt; a.y = y; a.z = z; a.level = level;
    a.max_feat = params->max_feat; a.j_split = (int32_t)g.j_split;
    a.hist = reinterpret_cast<unsigned long long *>(o->hist);
    a.below = reinterpret_cast<unsigned long long *>(o->below);
    a.above = reinterpret_cast<unsigned long long *>(o->above);
    a.nan = reinterpret_cast<unsigned long long *>(o->nan);
    a.max_key = reinterpret_cast<unsigned long long *>(o->max);
    a.n = reinterpret_cast<unsigned long long *>(o->n);
    a.status = o->status;
    a.tables = reinterpret_cast<unsigned long long *>(tables);
    hipStream_t s = ctx_stream(ctx);
    hipLaunchKernelGGL(dc_zero_kernel, dim3((unsigned)n_frames), dim3(kDcFinishBlock), 0, s, a);
    rc = check_launch("dc_zero_kernel");
    if (rc) return rc;
    if (g.row_blocks > 0) {
        hipLaunchKernelGGL(depthcheck_kernel, dim3((unsigned)n_frames, (unsigned)(g.row_blocks * g.j_split)), dim3(kDcRows), 0, s, a);
        rc = check_launch("depthcheck_kernel");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(dc_finish_kernel, dim3((unsigned)n_frames), dim3(kDcFinishBlock), 0, s, a);
    return check_launch("dc_finish_kernel");
}
