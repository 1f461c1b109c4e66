// mvosr_featdist_plan.hpp — the LDS layout of featdist_kernel (mvosr_featdist.hip), by the convention of
// mvosr_rescale_plan.hpp: the kernel takes every LDS pointer from the plan, the launcher requests its `total`, both evaluated at
// the launch's max_feat; the offsets' type is a template parameter (uint32_t in the kernel, size_t in the launcher).
//
// One workgroup per frame, one wavefront per population; the three waves never meet, so each owns one `per_wave` slice:
//     list      double[N rounded up to even]   the population's y, compacted in packed order
//     hist      int[kFdHistWords]              the 169 bins of y, then how many y equal edge 29, 49, 99 (the closing edges of the
//                                              narrower histograms)
//     hist_s    int[kFdHistWords]              the same of y * scale
//     leaf_sum  double[N / 64 + 1]             the sums of the leaves of NumPy's pairwise tree (a leaf of a list above 128 values
//                                              has at least 64)
//     leaf_off  int[N / 64 + 2]                where each leaf starts; one more entry: n
//     stack     the tree walk's frames: int size[16], int state[16], double left[16] (the tree is at most 8 deep below 8192)
// The cap on a frame's features is the largest multiple of 8 whose three slices fit 160 KiB.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include "mvosr_rescale_plan.hpp"

namespace mvosr {

constexpr int kFdPops = 3;                    // every feature below the vanishing row; kept by the vote; selected as road
constexpr int kFdBins = 169;                  // MVOSR_HIST_BINS
constexpr int kFdEdges = 3;                   // the closing edges counted: 29, 49, 99
constexpr int kFdHistWords = kFdBins + kFdEdges;   // MVOSR_FD_HIST_WORDS
constexpr int kFdStack = 16;
constexpr int kFdLeafMin = 64;                // the smallest leaf of a list above 128 values (129 = 64 + 65)
constexpr int kFdLdsBytes = 160 * 1024;       // gfx950: LDS per workgroup

template <typename U> struct FeatDistPlan {
    U list, hist, hist_s, leaf_sum, leaf_off, stack_size, stack_state, stack_left;
    U per_wave;     // one population's slice
    U total;        // kFdPops slices
};
template <typename U> MVOSR_HD inline constexpr FeatDistPlan<U> featdist_plan(U max_feat) {
    FeatDistPlan<U> p{};
    const U leaves = max_feat / (U)kFdLeafMin + 1;
    p.list = 0;
    p.leaf_sum = p.list + 8u * ((max_feat + 1) & ~(U)1);
    p.stack_left = p.leaf_sum + 8u * leaves;
    p.hist = p.stack_left + 8u * (U)kFdStack;
    p.hist_s = p.hist + 4u * (U)kFdHistWords;
    p.leaf_off = p.hist_s + 4u * (U)kFdHistWords;
    p.stack_size = p.leaf_off + 4u * (leaves + 1);
    p.stack_state = p.stack_size + 4u * (U)kFdStack;
    p.per_wave = (p.stack_state + 4u * (U)kFdStack + 15u) & ~(U)15;
    p.total = (U)kFdPops * p.per_wave;
    return p;
}

// the largest frame the plan holds: MVOSR_ERR_TOO_LARGE above it (mvosr_featdist_max_features)
MVOSR_HD inline constexpr int featdist_max_features() {
    int n = kFdLdsBytes / (8 * kFdPops);
    n -= n % 8;
    while (featdist_plan<size_t>((size_t)n).total > (size_t)kFdLdsBytes) n -= 8;
    return n;
}
constexpr int kFdMaxFeatures = featdist_max_features();
static_assert(kFdMaxFeatures >= 6000 && kFdMaxFeatures < 8192, "a list stays below NumPy's 8192-element chunk: one pairwise tree");

}  // namespace mvosr
