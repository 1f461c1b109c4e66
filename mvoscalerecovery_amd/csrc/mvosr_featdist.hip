// mvosr_featdist.hip — the reference's feature-distribution analysis (check_full_distribution, skewness_analysis, mode_analysis,
// plot_distribution: /root/reference/src/scale_calculator.py:486-599) on the device: what those methods COMPUTE of the three
// populations of a frame — every feature below the vanishing row (:564-567), the ones the reliability vote keeps (:575-580), the
// ones feature_selection_by_tri selects (:588-593) — and of the sequence (:569, :582, :595: the populations scaled and accumulated).
//
// A feature carries one level: 0 = below the vanishing row only, 1 = also kept, 2 = also selected; population p is the features
// with level >= p, in packed order — the order of the reference's boolean-mask and np.unique indexing, which NumPy's sums follow.
// Per frame and population:
//     n
//     hist      np.histogram(y, np.array(range(0,170))*0.1) (:492), then the number of y equal to edge 29, 49 and 99: the narrower
//               histograms of :514-536, :506 are its first counts with that number added to their last (their last bin is closed)
//     hist_s    the same of y * scale (one multiply; :569), which also goes into the sequence tables
//     mean, std, median   as np.mean / np.std / np.median give them, to the last bit (:487-496)
//
// One workgroup per frame, one wavefront per population; the waves never meet (no barrier), each works in its own LDS slice
// (mvosr_featdist_plan.hpp).
//   pass 1   the frame's levels and y are read once, 64 a step: a member's y goes to the wave's list at the position the ballot
//            gives it, and into the two histograms by LDS atomics (the bin: device.hpp's bin_of, by comparison with the edges).
//   sums     NumPy's pairwise order (mvosr_npsum.hpp states it) in parallel: the tree above the leaves is fixed by n, so one uniform
//            walk lists the leaves; then eight leaves at a time, eight lanes a leaf — a lane is one of the eight strided
//            accumulators, a chain of at most 16 additions — combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) by three lane shifts,
//            the remainder added one by one; a second uniform walk adds the leaves' sums up the tree.  Twice: y, then (y - mean)^2.
//   median   the radix select of mvosr_select.hpp over the list in LDS (keys: the doubles' patterns made to order like them).
//   tables   the scaled histogram's non-zero words are added to the sequence tables with one 64-bit atomic each: integers, so
//            the order of arrival changes nothing.
// The file is built with -ffp-contract=off: every operation here is an IEEE operation of its own.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_npsum.hpp"
#include "mvosr_select.hpp"
#include "mvosr_featdist_plan.hpp"

#include <math.h>

namespace mvosr {

constexpr int kFdBlock = kFdPops * kWave;
static_assert(kFdBins == kBins && kFdHistWords == MVOSR_FD_HIST_WORDS && kFdPops == MVOSR_FD_POPULATIONS, "mvosr.h");
static_assert(kFdMaxFeatures <= kNpBufSize, "np.add.reduce chunks a list above 8192 values: the tree below states one chunk");

struct FeatDistArgs {
    int64_t n_frames;
    const int64_t *off; const int32_t *cnt;  // cnt == nullptr: off has n_frames + 1 entries
    const double *y; const uint8_t *level;   // [features]
    const double *scale;                     // [F]
    int32_t max_feat;
    int32_t *n;                              // [F][3]
    int32_t *hist, *hist_scaled;             // [F][3][kFdHistWords]
    double *stats;                           // [F][3][3] mean, std, median
    int32_t *status;                         // [F]
    unsigned long long *seq;                 // optional [3][kFdHistWords], added to
};

// LDS instructions of a wavefront execute in order: a write by one lane is seen by a later read of another lane of the SAME wave
// without a barrier — only the compiler must keep the order (as in mvosr_qhull.hip).
__device__ __forceinline__ void fd_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// a double's pattern, made to order like the double (negative values: all bits flipped; others: the sign bit set), and back
__device__ __forceinline__ unsigned long long fd_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double fd_unkey(unsigned long long k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
}

struct FdWave {
    double *list, *leaf_sum, *left;
    int *hist, *hist_s, *leaf_off, *size, *state;
};

__device__ __forceinline__ double fd_term(const double *a, int i, double shift, bool sq) { return np_term(a, i, shift, sq); }

// The walk over np.add.reduce's pairwise tree of n > 128 ... or one leaf (8 <= n <= 128): a node above 128 values splits into its
// first half rounded down to a multiple of 8 and the rest; leaf(offset, size) gives a leaf's value, left to right, and a node's
// value is left + right.  Uniform: every lane walks the same tree and keeps the frames in the wave's LDS stack.
template <class Leaf>
__device__ __forceinline__ double fd_tree(const FdWave &w, int n, Leaf leaf) {
    int d = 0, at = 0;
    w.size[0] = n;
    w.state[0] = 0;
    fd_lds_sync();
    double ret = 0.0;
    for (;;) {
        const int m = w.size[d];
        if (m > 128) {                                             // (a fresh node: down its left half)
            int n2 = m / 2;
            n2 -= n2 % 8;
            w.state[d] = 1;
            w.size[d + 1] = n2;
            w.state[d + 1] = 0;
            fd_lds_sync();
            ++d;
            continue;
        }
        ret = leaf(at, m);
        at += m;
        // back up: a node whose left half just returned goes down its right half; one whose right half returned adds and returns
        for (;;) {
            if (--d < 0) return ret;
            if (w.state[d] == 1) {
                const int mm = w.size[d];
                int n2 = mm / 2;
                n2 -= n2 % 8;
                w.left[d] = ret;
                w.state[d] = 2;
                w.size[d + 1] = mm - n2;
                w.state[d + 1] = 0;
                fd_lds_sync();
                ++d;
                break;
            }
            ret = w.left[d] + ret;
        }
    }
}

// the leaves of the tree of a list of n >= 8 values -> w.leaf_off[0..K], K returned
__device__ __forceinline__ int fd_list_leaves(const FdWave &w, int n) {
    int k = 0;
    fd_tree(w, n, [&](int at, int) { w.leaf_off[k] = at; ++k; return 0.0; });
    w.leaf_off[k] = n;
    fd_lds_sync();
    return k;
}

// np.add.reduce over the wave's list (sq: over (a[i] - shift)^2), in NumPy's order; every lane returns the same sum
__device__ __forceinline__ double fd_np_sum(const FdWave &w, int n, int n_leaves, double shift, bool sq) {
    const double *a = w.list;
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += fd_term(a, i, shift, sq);
        return res;
    }
    const int lane = lane_id(), j = lane & 7;
    for (int k0 = 0; k0 < n_leaves; k0 += 8) {
        const int k = k0 + (lane >> 3);
        const bool active = k < n_leaves;
        const int o = active ? w.leaf_off[k] : 0;
        const int m = active ? w.leaf_off[k + 1] - o : 0;
        const int body = m - (m % 8);
        double r = 0.0;
        if (active) {
            r = fd_term(a, o + j, shift, sq);
            for (int i = 8; i < body; i += 8) r += fd_term(a, o + i + j, shift, sq);
        }
        r += __shfl_down(r, 1);                                    // lanes j = 0, 2, 4, 6: r0+r1, r2+r3, r4+r5, r6+r7
        r += __shfl_down(r, 2);                                    // lanes j = 0, 4: (r0+r1)+(r2+r3), (r4+r5)+(r6+r7)
        r += __shfl_down(r, 4);                                    // lane j = 0
        if (active && j == 0) {
            for (int i = body; i < m; ++i) r += fd_term(a, o + i, shift, sq);
            w.leaf_sum[k] = r;
        }
    }
    fd_lds_sync();
    int k = 0;
    return fd_tree(w, n, [&](int, int) { return w.leaf_sum[k++]; });
}

__global__ __launch_bounds__(kFdBlock) void featdist_kernel(const FeatDistArgs a) {
    extern __shared__ __align__(16) unsigned char fd_smem[];
    const int64_t f = blockIdx.x;
    const int p = wave_id(), lane = lane_id();
    const auto lds = featdist_plan<uint32_t>((uint32_t)a.max_feat);
    unsigned char *mine = fd_smem + (uint32_t)p * lds.per_wave;
    FdWave w;
    w.list = reinterpret_cast<double *>(mine + lds.list);
    w.leaf_sum = reinterpret_cast<double *>(mine + lds.leaf_sum);
    w.left = reinterpret_cast<double *>(mine + lds.stack_left);
    w.hist = reinterpret_cast<int *>(mine + lds.hist);
    w.hist_s = reinterpret_cast<int *>(mine + lds.hist_s);
    w.leaf_off = reinterpret_cast<int *>(mine + lds.leaf_off);
    w.size = reinterpret_cast<int *>(mine + lds.stack_size);
    w.state = reinterpret_cast<int *>(mine + lds.stack_state);

    const int64_t base = a.off[f];
    const int64_t len64 = a.cnt ? (int64_t)a.cnt[f] : a.off[f + 1] - base;
    // a frame the launch's LDS was not sized for, or that no launch of this library describes: refused before anything of it is read
    const bool shaped = base >= 0 && len64 >= 0 && len64 <= (int64_t)a.max_feat;
    const int len = shaped ? (int)len64 : 0;
    const double *Y = a.y + (shaped ? base : 0);
    const uint8_t *LV = a.level + (shaped ? base : 0);
    const double sc = a.scale[f];

    for (int k = lane; k < kFdHistWords; k += kWave) { w.hist[k] = 0; w.hist_s[k] = 0; }
    fd_lds_sync();

    // ---- pass 1: the population compacted in order, the two histograms
    int n = 0;
    bool bad = false, has_nan = false;
    for (int i0 = 0; i0 < len; i0 += kWave) {
        const int i = i0 + lane;
        const int lv = i < len ? (int)LV[i] : -1;
        bad = bad || lv > 2;
        const bool member = lv >= p && lv <= 2;
        const unsigned long long mask = __ballot(member);
        if (member) {
            const double y = Y[i];
            w.list[n + __popcll(mask & ((1ull << lane) - 1ull))] = y;
            has_nan = has_nan || y != y;
            const double ys = y * sc;                              // :569, :582, :595 (column 1 of feature * scale)
            const int b = bin_of(y), bs = bin_of(ys);
            if (b >= 0) atomicAdd(&w.hist[b], 1);
            if (bs >= 0) atomicAdd(&w.hist_s[bs], 1);
            if (y == bin_edge(29)) atomicAdd(&w.hist[kFdBins + 0], 1);
            if (y == bin_edge(49)) atomicAdd(&w.hist[kFdBins + 1], 1);
            if (y == bin_edge(99)) atomicAdd(&w.hist[kFdBins + 2], 1);
            if (ys == bin_edge(29)) atomicAdd(&w.hist_s[kFdBins + 0], 1);
            if (ys == bin_edge(49)) atomicAdd(&w.hist_s[kFdBins + 1], 1);
            if (ys == bin_edge(99)) atomicAdd(&w.hist_s[kFdBins + 2], 1);
        }
        n += __popcll(mask);
    }
    const bool refused = !shaped || __ballot(bad) != 0ull;
    has_nan = __ballot(has_nan) != 0ull;
    fd_lds_sync();
    if (refused) n = 0;

    // ---- the statistics
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double mean = nan, sd = nan, median = nan;
    if (n > 0) {
        const int n_leaves = n >= 8 ? fd_list_leaves(w, n) : 0;
        mean = fd_np_sum(w, n, n_leaves, 0.0, false) / (double)n;               // np.mean: add.reduce, then one division
        sd = sqrt(fd_np_sum(w, n, n_leaves, mean, true) / (double)n);           // np.std: x = a - mean; x = x * x; sqrt(sum / n)
        if (!has_nan) {                                                         // (np.median of a list that holds a NaN: NaN)
            unsigned long long lo, hi;
            const double *L = w.list;
            wave_middle_keys([&](auto visit) {
                for (int i0 = 0; i0 < n; i0 += kWave) {
                    const int i = i0 + lane;
                    const bool counted = i < n;
                    visit(counted, counted ? fd_key(L[i]) : 0ull);
                }
            }, n, lo, hi);
            // np.median ends in np.mean of the one or two middle values: a sum that starts at 0.0 (so -0.0 comes out 0.0)
            median = (n & 1) ? (0.0 + fd_unkey(lo)) / 1.0 : ((0.0 + fd_unkey(lo)) + fd_unkey(hi)) / 2.0;
        }
    }

    // ---- results
    const int64_t row = f * kFdPops + p;
    for (int k = lane; k < kFdHistWords; k += kWave) {
        const int h = refused ? 0 : w.hist[k], hs = refused ? 0 : w.hist_s[k];
        a.hist[row * kFdHistWords + k] = h;
        a.hist_scaled[row * kFdHistWords + k] = hs;
        if (a.seq && hs != 0) atomicAdd(&a.seq[p * kFdHistWords + k], (unsigned long long)hs);
    }
    if (lane == 0) {
        a.n[row] = n;
        a.stats[row * 3 + 0] = mean;
        a.stats[row * 3 + 1] = sd;
        a.stats[row * 3 + 2] = median;
        if (p == 0) a.status[f] = refused ? MVOSR_ST_ERR_MASK : 0;
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_featdist_max_features(void) { return kFdMaxFeatures; }

extern "C" int mvosr_feature_distribution_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *off, const int32_t *cnt, const double *y,
                                                const uint8_t *level, const double *scale, int32_t max_feat, int32_t *n_out,
                                                int32_t *hist, int32_t *hist_scaled, double *stats, int32_t *status, int64_t *seq_tables) {
    if (!ctx || !off || !y || !level || !scale || !n_out || !hist || !hist_scaled || !stats || !status)
        return set_error(MVOSR_ERR_ARG, "feature_distribution: null argument");
    if (max_feat < 0) return set_error(MVOSR_ERR_ARG, "feature_distribution: max_feat < 0");
    if (max_feat > kFdMaxFeatures)
        return set_error(MVOSR_ERR_TOO_LARGE, "feature_distribution: a frame of %d features does not fit LDS (at most %d)", max_feat, kFdMaxFeatures);
    if (n_frames <= 0) return MVOSR_OK;
    if (n_frames > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "feature_distribution: more than 2^31-1 frames in one launch");
    const size_t lds = featdist_plan<size_t>((size_t)max_feat).total;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "feature_distribution: frame of %d features needs %zu B of LDS (> %d)", max_feat, lds, ctx->max_lds_per_block);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(featdist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    FeatDistArgs a = {};
    a.n_frames = n_frames; a.off = off; a.cnt = cnt; a.y = y; a.level = level; a.scale = scale; a.max_feat = max_feat;
    a.n = n_out; a.hist = hist; a.hist_scaled = hist_scaled; a.stats = stats; a.status = status;
    a.seq = reinterpret_cast<unsigned long long *>(seq_tables);
    hipLaunchKernelGGL(featdist_kernel, dim3((unsigned)n_frames), dim3(kFdBlock), lds, ctx_stream(ctx), a);
    return check_launch("featdist_kernel");
}
