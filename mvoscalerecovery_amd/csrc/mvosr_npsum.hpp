// mvosr_npsum.hpp — NumPy's summation order on the device, shared by the kernels that must reproduce np.mean / np.std to the
// last bit (mvosr_kernels.hip: height_level, the skewness decision; mvosr_trigraph.hip: height_level; mvosr_scalescore.hip and
// mvosr_heightpitch_tail.hip: block_np_sum).  The text below was moved here from mvosr_kernels.hip and
// mvosr_scalescore.hip unchanged, but for block_np_sum's guard that lets a workgroup be larger than the recursion has nodes.
#pragma once

#include "mvosr_device.hpp"

namespace mvosr {

// np.add.reduce's summation order for a 1-D float64 array (numpy/core/src/umath/loops_utils.h.src,
// @TYPE@_pairwise_sum: below 8 values a plain loop; up to 128 eight strided accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and the remainder added one by one; above that the halves —
// the first rounded down to a multiple of 8 — summed recursively).  With sq the terms are
// (a[i]-shift)^2, as in np.std's  x = arr - mean; x = x*x; sum(x).  Every lane of the wavefront runs it
// redundantly on the same packed list; it is the cold path behind the skewness decision (road_wave).
__device__ __forceinline__ double np_term(const double *a, int i, double shift, bool sq) {
    const double v = a[i];
    if (!sq) return v;
    const double d = v - shift;
    return d * d;
}
__device__ double np_leaf_sum(const double *a, int n, double shift, bool sq) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += np_term(a, i, shift, sq);
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = np_term(a, j, shift, sq);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += np_term(a, i + j, shift, sq);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += np_term(a, i, shift, sq);
    return res;
}
constexpr int kNpDepth = 8;                                  // a chunk has <= 8192 elements, a leaf <= 128: at most 7 levels

// np.add.reduce hands its inner loop at most `bufsize` (8192, np.getbufsize()) elements at a time and adds the
// chunks' pairwise sums up from left to right (checked against NumPy 2.2 for lists of 10^4 - 2*10^5 elements: a single
// pairwise recursion over the whole list differs in the last bits from 10291 elements on).
constexpr int kNpBufSize = 8192;
constexpr int kNpNodes = 1 << kNpDepth;                      // nodes of one chunk's recursion by heap index (np_heap_node)

// The node with heap index h (the root is 0, the halves of node h are 2h + 1 and 2h + 2) of the recursion over m <= kNpBufSize
// elements: its slice [lo, lo + len), or len = 0 where the tree has no such node (an ancestor is a leaf).  A slice at depth d
// has at most m / 2^d + 15 elements, so the leaves lie at depth 7 at the latest: h < kNpNodes.
__device__ __forceinline__ void np_heap_node(int h, int m, int &lo, int &len) {
    const int depth = 31 - __clz(h + 1);
    lo = 0;
    len = m;
    for (int d = depth - 1; d >= 0; --d) {                      // the bits of h + 1 below the leading one: 0 the first half, 1 the second
        if (len <= 128) { len = 0; return; }
        int m2 = len / 2;
        m2 -= m2 % 8;
        if (((h + 1) >> d) & 1) { lo += m2; len -= m2; } else len = m2;
    }
}

// np.add.reduce(a[0 : n]) by a workgroup of at least kNpNodes threads; `node`: kNpNodes doubles of LDS, `slot`: one.
// Workgroup-uniform call; what `a` holds was written before a barrier.  Per chunk, thread h is node h of the recursion: the
// leaves are summed side by side, then every inner node adds its two halves, the deepest first — the recursion's own additions,
// none of them in another order.
__device__ __forceinline__ double block_np_sum(const double *a, int64_t n, double *node, double *slot) {
    const int t = threadIdx.x;
    const int depth = 31 - __clz(t + 1);
    if (t == 0) *slot = 0.0;                                     // the reduction starts from add's identity
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += kNpBufSize) {
        const int m = (int)((n - c0) < (int64_t)kNpBufSize ? (n - c0) : (int64_t)kNpBufSize);
        int lo = 0, len = 0;
        if (t < kNpNodes) np_heap_node(t, m, lo, len);
        if (len > 0 && len <= 128) node[t] = np_leaf_sum(a + c0 + lo, len, 0.0, false);
        __syncthreads();
        for (int d = kNpDepth - 2; d >= 0; --d) {
            if (len > 128 && depth == d && 2 * t + 2 < kNpNodes) node[t] = node[2 * t + 1] + node[2 * t + 2];
            __syncthreads();
        }
        if (t == 0) *slot = *slot + node[0];
        __syncthreads();
    }
    const double res = *slot;
    __syncthreads();
    return res;
}

}  // namespace mvosr
