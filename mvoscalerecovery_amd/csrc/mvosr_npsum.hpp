// mvosr_npsum.hpp — NumPy's summation order on the device, shared by the kernels that must reproduce np.mean / np.std to the
// last bit (mvosr_kernels.hip: height_level, the skewness decision; mvosr_trigraph.hip: height_level).  The text below was
// moved here from mvosr_kernels.hip unchanged.
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

}  // namespace mvosr
